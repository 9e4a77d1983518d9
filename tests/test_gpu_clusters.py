"""Flat clusters and the scores of a labelling on the GPU (cluster_scores_kernel and its driver in
csrc/clusters.hip, the host cut in csrc/linkage.hip).  Every comparison is against something other than the code
under test: the long-double yardstick of tests/test_clusters_host.py (which also pins that no neighbour or medoid of
the random cases hangs on rounding), sklearn's silhouette_samples, scipy's fcluster, numpy on the distance matrices the
earlier entries return."""
import ctypes as C

import numpy as np
import pytest
from scipy.cluster.hierarchy import fcluster
from scipy.cluster.hierarchy import linkage as scipy_linkage

from conftest import GOLDEN, read_fasta
from diverseseq_amd import _lib, apps, cluster, distance, engine
from test_clusters_host import (GAP_FACTOR, METHODS, SCORE_CASES, assert_cuts_match_scipy, bound, cut_matrix,
                                first_appearance, random_matrix, sklearn_silhouettes, smallest_relative_gaps, tie_case,
                                truth_cluster_scores)
from test_cross_host import FAMILY_CASES, family_split

pytestmark = pytest.mark.gpu

FLOATS = ("within", "a", "b", "silhouette", "cluster_silhouette")
INTS = ("labels", "neighbour", "sizes", "medoids")


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context()


def same_bits(a, b) -> bool:
    """equal shapes, NaN in the same cells, the same bits everywhere else"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return bool((a[ok].view(np.uint64) == b[ok].view(np.uint64)).all())


def assert_same_scores(x, y, what=""):
    for f in FLOATS:
        assert same_bits(getattr(x, f), getattr(y, f)), (what, f)
    for f in INTS:
        assert np.array_equal(getattr(x, f), getattr(y, f)), (what, f)
    assert same_bits([x.mean_silhouette], [y.mean_silhouette]), what


def assert_scores(got, D, labels, what="", with_sklearn=True):
    """a ClusterScores against the yardstick over D (and sklearn, where it takes the labels)"""
    lab = np.asarray(labels)
    n = lab.size
    t = truth_cluster_scores(D, lab)
    for f in ("within", "a", "b", "silhouette"):
        v = getattr(got, f)
        assert v.dtype == np.float64 and v.shape == (n,), (what, f)
        assert np.array_equal(np.isnan(v), np.isnan(t[f])), (what, f)
    ok = lambda f: ~np.isnan(t[f])  # noqa: E731
    worst = {}
    for f in ("within", "a", "b"):
        err = np.abs(getattr(got, f).astype(np.longdouble) - t[f])[ok(f)]
        ref = np.abs(t[f])[ok(f)]
        worst[f] = float((err / np.where(ref > 0, ref, 1)).max()) if err.size else 0.0
        assert (err <= bound(n) * ref).all(), (what, f, worst[f])
    err = np.abs(got.silhouette.astype(np.longdouble) - t["silhouette"])[ok("silhouette")]
    worst["silhouette"] = float(err.max()) if err.size else 0.0
    assert (err <= bound(n)).all(), (what, worst)
    print(f"{what}: largest errors in units of the bound {({f: round(w / bound(n), 4) for f, w in worst.items()})}")
    for f in ("neighbour", "medoids", "sizes"):
        assert getattr(got, f).dtype == np.int64, (what, f)
        np.testing.assert_array_equal(getattr(got, f), t[f], err_msg=f"{what} {f}")
    np.testing.assert_array_equal(got.labels, lab)
    # the means per cluster and overall are the host's, from the n silhouettes
    for c, size in enumerate(t["sizes"]):
        members = got.silhouette[lab == c]
        if size == 0:
            assert np.isnan(got.cluster_silhouette[c])
        elif not np.isnan(members).any():
            assert abs(got.cluster_silhouette[c] - members.astype(np.longdouble).mean()) <= bound(n)
    if not np.isnan(got.silhouette).any():
        assert abs(got.mean_silhouette - got.silhouette.astype(np.longdouble).mean()) <= bound(n)
    k_used = int((t["sizes"] > 0).sum())
    Dz = np.array(D, dtype=np.float64)
    np.fill_diagonal(Dz, 0.0)  # (sklearn insists on a zero diagonal; nothing here reads it)
    if with_sklearn and 2 <= k_used <= n - 1 and not np.isnan(Dz).any():
        sk = sklearn_silhouettes(Dz, lab)
        assert (np.abs(got.silhouette - sk) <= bound(n)).all(), (what, float(np.abs(got.silhouette - sk).max()))
    return t


# ------------------------------------------------------------------ 1. sizes and label shapes, a caller's host matrix
@pytest.mark.parametrize("name", list(SCORE_CASES))
def test_sizes_and_label_shapes_against_the_yardstick(ctx, name):
    D, lab = SCORE_CASES[name]
    got = cluster.cluster_scores(D, lab, ctx=ctx)
    assert_scores(got, D, lab, name)
    if name.endswith("singletons"):
        assert (got.within == 0).all() and (got.a == 0).all() and (got.silhouette == 0).all()
        assert np.array_equal(got.medoids[lab], np.arange(lab.size))
    if name.endswith("-one"):
        assert (got.neighbour == -1).all() and np.isnan(got.b).all() and got.sizes.tolist() == [lab.size]
        assert (got.silhouette == 0).all() if lab.size == 1 else np.isnan(got.silhouette).all()
    if name == "empty-label-in-the-middle":
        assert got.sizes[2] == 0 and got.medoids[2] == -1 and not (got.neighbour == 2).any()


# ------------------------------------------------------------------ 2. the tie case
@pytest.mark.parametrize("wide", [False, True], ids=["labels012", "labels015"])
def test_tie_case_is_exact_and_goes_to_the_lower(ctx, wide):
    """every sum is exact, so every float is the float64 evaluation of the definitions bit for bit; labels 0, 1, 5 put
    the tied clusters into one wave's share (1 and 5), labels 0, 1, 2 into two waves'"""
    D, lab = tie_case()
    if wide:
        lab = np.where(lab == 2, 5, lab)
    got = cluster.cluster_scores(D, lab, ctx=ctx)
    exact = truth_cluster_scores(D, lab, dtype=np.float64)
    for f in ("within", "a", "b", "silhouette"):
        assert same_bits(getattr(got, f), exact[f]), f
    for f in ("neighbour", "medoids", "sizes"):
        np.testing.assert_array_equal(getattr(got, f), exact[f])
    assert got.neighbour[0] == 1 and got.b[0] == 10 / 8 / 4
    assert got.medoids[lab[9]] == 9 and got.within[9] == got.within[10] == 6 / 8
    assert_scores(got, D, lab, "tie case")


# ------------------------------------------------------------------ 3. the same bits
def test_two_calls_give_the_same_bits(ctx):
    for name in ("n600-giant", "sizes-1-63-64-65-300"):
        D, lab = SCORE_CASES[name]
        assert_same_scores(cluster.cluster_scores(D, lab, ctx=ctx), cluster.cluster_scores(D, lab, ctx=ctx), name)


@pytest.mark.parametrize("strip", [1, 7, 64])
def test_strip_height_does_not_change_a_bit(ctx, monkeypatch, strip):
    D, lab = SCORE_CASES["sizes-1-63-64-65-300"]
    rng = np.random.default_rng(4)
    seqs = [rng.integers(0, 4, size=int(rng.integers(100, 900)), dtype=np.uint8) for _ in range(130)]
    seqs[17] = np.full(40, 4, np.uint8)  # no valid k-mer: NaN cells in the jsd and euclidean strips
    slab = SCORE_CASES["empty-label-in-the-middle"][1]
    m = ctx.build_matrix(seqs, 4, 4)
    sk = distance.Sketches([s if i != 17 else seqs[3] for i, s in enumerate(seqs)], 8, 50, ctx=ctx)
    try:
        def run():
            out = {"host": cluster.cluster_scores(D, lab, ctx=ctx), "mash": sk.cluster_scores(slab)}
            for mode in ("jsd", "euclidean"):
                out[mode] = distance.matrix_cluster_scores(m, slab, mode)
            return out

        whole = run()
        monkeypatch.setenv("DVS_CROSS_STRIP_ROWS", str(strip))
        for what, got in run().items():
            assert_same_scores(got, whole[what], f"{what}, strips of {strip}")
        assert_scores(whole["host"], D, lab, "host")
    finally:
        m.close()
        sk.close()


def test_device_tensor_and_its_host_copy_give_the_same_bits(ctx):
    """(where this is the first test of a process to put a tensor on the device, its time is torch's initialisation)"""
    torch = pytest.importorskip("torch")
    D, lab = SCORE_CASES["n257-giant"]
    t = torch.from_numpy(D).to("cuda:0")
    got = cluster.cluster_scores(t, lab, ctx=ctx)
    assert np.array_equal(t.cpu().numpy(), D)  # read, not overwritten
    assert_same_scores(got, cluster.cluster_scores(D, lab, ctx=ctx), "device tensor")
    assert_scores(got, D, lab, "device tensor")


# ------------------------------------------------------------------ 4. the three modes over their own strips
def _mode_seqs(seed=21, n=80):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 4, size=int(rng.integers(200, 1500)), dtype=np.uint8) for _ in range(n)]


def _mode_rows_and_labels():
    rng = np.random.default_rng(22)
    rows = rng.permutation(80)[:65]  # permutes, and drops 15 rows
    return rows, rng.integers(0, 5, size=65)


def _assert_mode_equals_matrix_path(ctx, got, d, labels, what):
    """the strips' scores against cluster.cluster_scores on the matrix the cross entry returns for the same rows, its
    diagonal overwritten: cell (i, i) is not read into a sum"""
    d = d.copy()
    np.fill_diagonal(d, 7.0)
    assert_same_scores(got, cluster.cluster_scores(d, labels, ctx=ctx), what)
    assert_scores(got, d, labels, what)


@pytest.mark.parametrize("mode", ["jsd", "euclidean"])
@pytest.mark.parametrize("width", [2, 4, 0], ids=["u16", "u32", "f64"])
def test_count_modes_same_bits_as_the_matrix_path(ctx, monkeypatch, mode, width):
    import oracle

    seqs, (rows, labels) = _mode_seqs(), _mode_rows_and_labels()
    k = 3
    if width == 4:
        monkeypatch.setenv("DVS_COUNTS_U32", "1")
    if width == 0:
        m = ctx.matrix_from_freqs(np.stack([oracle.to_kfreqs(s, 4, k)[0] for s in seqs]))
    else:
        m = ctx.build_matrix(seqs, k, 4)
    try:
        assert m.count_bytes == width
        got = distance.matrix_cluster_scores(m, labels, mode, rows=rows)
        d = distance.matrix_cross_distances(m, m, mode, q_rows=rows, r_rows=rows)
        _assert_mode_equals_matrix_path(ctx, got, d, labels, f"{mode} width {width}")
        # every row, no list
        lab80 = np.arange(80) % 7
        d80 = distance.matrix_cross_distances(m, m, mode)
        _assert_mode_equals_matrix_path(ctx, distance.matrix_cluster_scores(m, lab80, mode), d80, lab80, f"{mode} all rows")
    finally:
        m.close()


@pytest.mark.parametrize("canonical", [False, True], ids=["plain", "canonical"])
def test_mash_same_bits_as_the_matrix_path(ctx, canonical):
    seqs, (rows, labels) = _mode_seqs(), _mode_rows_and_labels()
    sk = distance.Sketches(seqs, 9, 120, 4, canonical, ctx=ctx)
    try:
        got = sk.cluster_scores(labels, rows=rows)
        d = sk.cross_distances(sk, rows=rows, other_rows=rows)
        _assert_mode_equals_matrix_path(ctx, got, d, labels, f"mash canonical={canonical}")
    finally:
        sk.close()
    pub = distance.cluster_scores(seqs, np.arange(80) % 3, "mash", k=9, sketch_size=120, mash_canonical=canonical, ctx=ctx)
    d = distance.mash_distances(seqs, 9, 120, 4, canonical, ctx=ctx)
    _assert_mode_equals_matrix_path(ctx, pub, d, np.arange(80) % 3, "distance.cluster_scores mash")


def test_public_function_over_sequences_count_modes(ctx):
    seqs = _mode_seqs(23, 40)
    lab = np.arange(40) % 4
    for mode in ("jsd", "euclidean"):
        got = distance.cluster_scores(seqs, lab, mode, k=4, ctx=ctx)
        _assert_mode_equals_matrix_path(ctx, got, distance.MODES[mode][0](seqs, 4, 4, ctx=ctx), lab, mode)


# ------------------------------------------------------------------ 5. rows without a valid k-mer
def test_nan_rows_are_never_taken(ctx):
    """jsd with sequences without a valid k-mer: the rectangular cells of such a row are NaN, its own cell included (no
    diagonal is forced to zero), and that cell is never read"""
    seqs = _mode_seqs(24, 30)
    seqs[7] = np.full(50, 4, np.uint8)
    m = ctx.build_matrix(seqs, 3, 4)
    try:
        d = distance.matrix_cross_distances(m, m, "jsd")
        assert np.isnan(d[7]).all() and np.isnan(d[:, 7]).all() and np.isnan(d).sum() == 59
        # (a) with others in cluster 1
        lab = np.arange(30) % 3
        got = distance.matrix_cluster_scores(m, lab, "jsd")
        t = assert_scores(got, d, lab, "NaN row among others")
        assert all(np.isnan(getattr(got, f)[7]) for f in ("within", "a", "b", "silhouette")) and got.neighbour[7] == -1
        assert not (got.neighbour == 1).any() and got.medoids[1] == -1  # (every member of cluster 1 sums a NaN cell)
        others = lab != 1
        assert np.isfinite(got.a[others]).all() and np.isfinite(got.b[others]).all() and np.isfinite(got.within[others]).all()
        assert got.medoids[0] >= 0 and got.medoids[2] >= 0 and 7 not in got.medoids
        assert np.isnan(got.mean_silhouette) and np.isnan(got.cluster_silhouette[1]) and np.isfinite(got.cluster_silhouette[0])
        # (b) alone in cluster 3: its sum is empty -- 0, not NaN: cell (7, 7), the one NaN it could have met, is never
        # added -- so by the definitions it is its cluster's medoid, with silhouette 0 (sklearn's rule for a cluster of
        # one) and no neighbour; nobody takes cluster 3 as a neighbour
        lab = np.arange(30) % 3
        lab[7] = 3
        got = distance.matrix_cluster_scores(m, lab, "jsd")
        assert_scores(got, d, lab, "NaN row alone")
        assert got.within[7] == 0 and got.a[7] == 0 and np.isnan(got.b[7]) and got.neighbour[7] == -1
        assert got.silhouette[7] == 0 and got.medoids[3] == 7 and not (got.neighbour == 3).any()
        assert np.isfinite(np.delete(got.a, 7)).all() and np.isfinite(np.delete(got.b, 7)).all()
    finally:
        m.close()
    # (c) a cluster of nothing but such rows, two of them: no member has a number for its sum -- medoid -1
    seqs[12] = np.full(30, 4, np.uint8)
    m = ctx.build_matrix(seqs, 3, 4)
    try:
        d = distance.matrix_cross_distances(m, m, "jsd")
        lab = np.arange(30) % 3
        lab[[7, 12]] = 3
        got = distance.matrix_cluster_scores(m, lab, "jsd")
        assert_scores(got, d, lab, "a cluster of two NaN rows")
        assert got.medoids[3] == -1 and np.isnan(got.within[[7, 12]]).all() and not (got.neighbour == 3).any()
        assert np.isfinite(np.delete(got.a, [7, 12])).all() and (got.medoids[:3] >= 0).all()
    finally:
        m.close()


# ------------------------------------------------------------------ 6. end to end
def test_cut_tree_on_device_built_trees(ctx):
    for method in METHODS:
        for tied in (False, True):
            n = 97
            d = np.zeros((n, n))
            d[np.triu_indices(n, 1)] = cut_matrix(n, tied, 9 + len(method))
            assert_cuts_match_scipy(cluster.linkage(d + d.T, method, ctx=ctx))


@pytest.mark.parametrize("by", ["n_clusters", "height"])
def test_ctree_clusters_recovers_the_families(ctx, by):
    nfam, per, length, seed, k = min(FAMILY_CASES, key=lambda c: c[0] * c[1])
    assert k == 6
    ref_names, refs, query_names, queries = family_split(nfam, per, length, seed)
    seqs = dict(zip(ref_names + query_names, refs + queries))
    names, arrays = list(seqs), list(seqs.values())
    n = len(names)
    Z_ref = distance.jsd_linkage(arrays, k, ctx=ctx)
    if by == "n_clusters":
        kw = dict(n_clusters=nfam)
    else:
        lo, hi = Z_ref[n - nfam - 1, 2], Z_ref[n - nfam, 2]
        assert lo < hi
        kw = dict(height=(lo + hi) / 2)
    newick, Z, sc = cluster.ctree_clusters(seqs, distance_mode="jsd", k=k, sketch_size=None, **kw)
    assert np.array_equal(Z, Z_ref) and newick == cluster.linkage_to_newick(names, Z_ref)
    families = first_appearance([int(name.split("_m")[0][3:]) for name in names])
    np.testing.assert_array_equal(sc.labels, families)
    np.testing.assert_array_equal(sc.labels, first_appearance(fcluster(Z, nfam, "maxclust")))
    d = distance.jsd_distances(arrays, k, ctx=ctx)
    assert (np.abs(sc.silhouette - sklearn_silhouettes(d, sc.labels)) <= bound(n)).all()
    t = assert_scores(sc, d, sc.labels, f"families by {by}")
    np.testing.assert_array_equal(sc.medoids, t["medoids"])
    assert sc.mean_silhouette > 0 and sc.sizes.tolist() == [per] * nfam


def test_dvs_clusters_app_on_brca1(ctx, brca1):
    raw = read_fasta(GOLDEN / "brca1.fasta")
    text = {n: s.replace("-", "").replace("?", "") for n, s in raw.items()}
    names = list(text)
    out = apps.dvs_clusters(3, distance_mode="mash", k=12)(text)
    assert set(out) == {"tree", "clusters", "medoids", "silhouette", "mean_silhouette"}
    # the same on the host: the mash matrix, scipy's tree and cut, the yardstick's medoids, sklearn's silhouettes
    arrays = [brca1[n] for n in names]
    d = distance.mash_distances(arrays, 12, 3000, ctx=ctx)
    Z = scipy_linkage(d[np.triu_indices(len(names), 1)], "average")
    lab = first_appearance(fcluster(Z, 3, "maxclust"))
    t = truth_cluster_scores(d, lab)
    g_mean, g_within = smallest_relative_gaps(t, lab)
    assert g_within > GAP_FACTOR * bound(len(names))  # (no medoid of this case hangs on rounding)
    assert out["tree"] == cluster.ctree({n: brca1[n] for n in names}, k=12, sketch_size=3000)
    assert out["clusters"] == {c: [n for n, l in zip(names, lab) if l == c] for c in range(int(lab.max()) + 1)}
    assert out["medoids"] == {c: names[i] for c, i in enumerate(t["medoids"])}
    assert list(out["silhouette"]) == names and all(isinstance(v, float) for v in out["silhouette"].values())
    sil = np.array([out["silhouette"][n] for n in names])
    assert (np.abs(sil.astype(np.longdouble) - t["silhouette"]) <= bound(len(names))).all()
    if 2 <= lab.max() + 1 <= len(names) - 1:
        assert (np.abs(sil - sklearn_silhouettes(d, lab)) <= bound(len(names))).all()
    assert isinstance(out["mean_silhouette"], float) and abs(out["mean_silhouette"] - sil.mean()) <= bound(len(names))


# ------------------------------------------------------------------ 7. errors
def test_errors(ctx):
    torch = pytest.importorskip("torch")
    D, lab = SCORE_CASES["n65-two"]
    for kw in ({}, dict(n_clusters=2, height=0.5)):
        with pytest.raises(ValueError, match="exactly one"):
            cluster.ctree_clusters({"a": np.zeros(30, np.uint8), "b": np.ones(30, np.uint8)}, **kw)
    for bad in (lab[:-1], np.concatenate([lab, [0]])):
        with pytest.raises(ValueError, match="labels"):
            cluster.cluster_scores(D, bad, ctx=ctx)
    with pytest.raises(ValueError, match="label out of range"):
        cluster.cluster_scores(D, np.where(np.arange(65) == 3, -1, lab), ctx=ctx)
    with pytest.raises(ValueError, match="square"):
        cluster.cluster_scores(D[:, :-1], lab, ctx=ctx)
    with pytest.raises(ValueError, match="square, contiguous float64"):
        cluster.cluster_scores(torch.zeros((65, 65), dtype=torch.float32, device="cuda:0"), lab, ctx=ctx)
    with pytest.raises(ValueError, match="square, contiguous float64"):
        cluster.cluster_scores(torch.zeros((65, 64), dtype=torch.float64, device="cuda:0"), lab, ctx=ctx)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="on device 1"):
            cluster.cluster_scores(torch.from_numpy(D).to("cuda:1"), lab, ctx=ctx)
    # the C entries' own checks
    L = ctx._L
    u32 = lambda a: _lib.ptr(a, C.c_uint32)  # noqa: E731
    f64 = lambda a: _lib.ptr(a, C.c_double)  # noqa: E731
    labels = np.ascontiguousarray(lab, dtype=np.uint32)
    within, med = np.zeros(65), np.zeros(2, np.uint32)

    def host(n, lab_, k, dist=D, on_device=0, within_=within):
        given = distance.make_source(_lib.SRC_GIVEN, dist.ctypes.data, n, on_device=on_device)
        return L.dvs_cluster_scores(ctx._h, given, u32(lab_), k, f64(within_), None, None, None, None, u32(med))

    assert host(65, labels, 2) == _lib.OK  # every output but `within` and the medoids left out
    t = truth_cluster_scores(D, lab)
    assert (np.abs(within.astype(np.longdouble) - t["within"]) <= bound(65) * t["within"]).all()
    assert med.tolist() == t["medoids"].tolist()
    assert host(65, labels, 1) == _lib.ERR_VALUE      # a label >= n_clusters
    assert host(65, labels, 0) == _lib.ERR_VALUE      # no clusters for 65 rows
    assert host(0, labels, 0) == _lib.OK              # nothing to do
    assert host(65, labels, 2, within_=None) == _lib.ERR_VALUE
    assert host(65, labels, 2, on_device=1) == _lib.ERR_VALUE  # a host array is not device memory
    big = 65535 * 8 + 1
    assert host(big, np.zeros(big, np.uint32), 1, within_=np.zeros(big)) == _lib.ERR_UNSUPPORTED
    seqs = _mode_seqs(25, 10)
    m = ctx.build_matrix(seqs, 3, 4)
    try:
        l10 = np.zeros(10, np.uint32)
        w10 = np.zeros(11)
        for kind in (_lib.SRC_JSD, _lib.SRC_EUCLIDEAN):
            def f(n, lab_, k, rows=None):
                return L.dvs_cluster_scores(ctx._h, distance.make_source(kind, m._h, n, rows), u32(lab_), k, f64(w10), None, None,
                                            None, None, None)

            assert f(10, l10, 1) == _lib.OK
            assert f(11, np.zeros(11, np.uint32), 1) == _lib.ERR_VALUE
            assert f(2, l10, 1, np.array([0, 10], np.uint32)) == _lib.ERR_VALUE
            assert f(10, l10 + 1, 1) == _lib.ERR_VALUE
            assert f(0, l10, 0) == _lib.OK
        with pytest.raises(ValueError, match="row list"):
            distance.matrix_cluster_scores(m, [0, 0], "jsd", rows=[0, 10])
        with pytest.raises(ValueError, match="Unexpected distance"):
            distance.matrix_cluster_scores(m, l10, "mash")
        assert distance.matrix_cluster_scores(m, l10, "jsd").sizes.tolist() == [10]  # the context is usable afterwards
    finally:
        m.close()
    rng = np.random.default_rng(2)
    short = [np.zeros(3, np.uint8), rng.integers(0, 4, 80, dtype=np.uint8), np.zeros(4, np.uint8)]
    sk = distance.Sketches(short, 8, 10, ctx=ctx)
    try:
        with pytest.raises(ZeroDivisionError):  # two empty sketches meet
            sk.cluster_scores([0, 0, 1])
        # one empty sketch is enough: the strips visit every cell, a row against itself included (as
        # cross_distances(sk, rows, rows) does); without it the call goes through
        with pytest.raises(ZeroDivisionError):
            sk.cluster_scores([0, 0], rows=[0, 1])
        assert sk.cluster_scores([0], rows=[1]).within.tolist() == [0.0]
    finally:
        sk.close()
