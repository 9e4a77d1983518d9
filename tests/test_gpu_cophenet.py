"""The cophenetic correlation on the GPU (cophenet_kernel and its consumer in csrc/cophenet.hip, the in-order walk in
csrc/linkage.hip).  Every comparison is against something other than the code under test: the long-double yardstick of
tests/test_cophenet_host.py (which also pins that float64 raw moments miss the bound by more than 100 x on the saturated
cases, so meeting it there takes the shift), scipy's cophenet for the cophenetic matrix bit for bit and for r, numpy on
the distance matrices the earlier entries return."""
import ctypes as C

import numpy as np
import pytest
from scipy.cluster.hierarchy import cophenet as scipy_cophenet
from scipy.cluster.hierarchy import linkage as scipy_linkage
from scipy.spatial.distance import squareform

from conftest import GOLDEN, read_fasta
from diverseseq_amd import _lib, apps, cluster, distance, engine
from test_cophenet_host import (GPU_SIZES, KINDS, METHODS, bound, case_matrix, condensed, truth_correlation,
                                truth_row_sums)
from test_cross_host import FAMILY_CASES
from test_gpu_linkage import family_seqs

pytestmark = pytest.mark.gpu


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
    assert same_bits([x.correlation], [y.correlation]), what
    assert same_bits(x.row_sums, y.row_sums), what
    assert (x.cophenetic is None) == (y.cophenetic is None), what
    if x.cophenetic is not None:
        assert same_bits(x.cophenetic, y.cophenetic), what


def assert_scores(got, D, Z, what="") -> float:
    """a CopheneticScores against the yardstick over D and against scipy; -> the error of r in units of the bound"""
    n = np.asarray(D).shape[0]
    Z = np.asarray(Z, dtype=np.float64)
    assert isinstance(got.correlation, float) and got.row_sums.dtype == np.float64 and got.row_sums.shape == (5, n), what
    if got.cophenetic is not None:
        assert got.cophenetic.dtype == np.float64
        assert same_bits(got.cophenetic, squareform(scipy_cophenet(Z))), what
    truth, mags = truth_row_sums(D, Z)
    err = np.abs(got.row_sums.astype(np.longdouble) - truth)
    lim = (n + 8) * 2.0 ** -52 * mags
    worst_sum = float((err / np.where(lim > 0, lim, 1)).max())
    assert (err <= lim).all(), (what, worst_sum)
    r = truth_correlation(D, Z)
    Dz = np.array(D, dtype=np.float64)
    np.fill_diagonal(Dz, 0.0)  # (scipy's squareform insists on a zero diagonal; nothing here reads it)
    with np.errstate(invalid="ignore", divide="ignore"):
        sp = float(scipy_cophenet(Z, condensed(Dz))[0])
    assert np.isnan(got.correlation) == np.isnan(r), (what, got.correlation, r)
    if np.isnan(r):
        print(f"{what}: r is NaN, as the yardstick's; row sums {worst_sum:.3g} x their bound")
        return 0.0
    e_truth, e_scipy = abs(got.correlation - r) / bound(n), abs(got.correlation - sp) / bound(n)
    print(f"{what}: |r - truth| = {e_truth:.3g} x bound, |r - scipy| = {e_scipy:.3g} x bound, row sums {worst_sum:.3g} x theirs")
    assert e_truth <= 1 and e_scipy <= 1, (what, e_truth, e_scipy)
    return e_truth


# ------------------------------------------------------------------ 1. a caller's host matrix
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", GPU_SIZES)
def test_host_matrix_against_the_yardstick_and_scipy(ctx, n, kind):
    D = case_matrix(n, kind)
    for method in METHODS:
        Z = cluster.linkage(D, method, ctx=ctx)
        got = cluster.cophenet(Z, D, matrix=True, ctx=ctx)
        assert_scores(got, D, Z, f"n={n} {kind} {method}")
        assert (np.diag(got.cophenetic) == 0).all()
        if n == 2:
            assert np.isnan(got.correlation)


@pytest.mark.parametrize("method", ["centroid", "median"])
def test_foreign_non_monotone_tree(ctx, method):
    D = case_matrix(65, "random")
    Z = scipy_linkage(condensed(D), method)
    assert (np.diff(Z[:, 2]) < 0).any()  # heights that decrease: dvs_linkage_cut would refuse this tree
    assert_scores(cluster.cophenet(Z, D, matrix=True, ctx=ctx), D, Z, f"scipy's {method} tree")
    swapped = Z.copy()
    swapped[::2, :2] = swapped[::2, 1::-1]
    assert_scores(cluster.cophenet(swapped, D, matrix=True, ctx=ctx), D, swapped, f"{method}, children swapped")


def test_degenerate_matrices_give_nan(ctx):
    for n, value in ((5, 0.75), (65, 0.5), (300, 0.5)):
        D = value * (1.0 - np.eye(n))
        for method in METHODS:  # (ward's heights vary over a constant matrix: x is constant and not zero)
            Z = cluster.linkage(D, method, ctx=ctx)
            got = cluster.cophenet(Z, D, matrix=True, ctx=ctx)
            assert np.isnan(truth_correlation(D, Z)) and np.isnan(got.correlation), (n, method, got.correlation)
            assert same_bits(got.cophenetic, squareform(scipy_cophenet(Z)))


# ------------------------------------------------------------------ 2. the same bits
def _mode_seqs(seed=21, n=80):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 4, size=int(rng.integers(200, 1500)), dtype=np.uint8) for _ in range(n)]


@pytest.mark.parametrize("strip", [1, 7, 64])
def test_strip_height_does_not_change_a_bit(ctx, monkeypatch, strip):
    D = case_matrix(300, "saturated")
    Z = cluster.linkage(D, "average", ctx=ctx)
    seqs = _mode_seqs(4, 130)
    m = ctx.build_matrix(seqs, 4, 4)
    sk = distance.Sketches(seqs, 8, 50, ctx=ctx)
    try:
        trees = {mode: cluster.linkage(distance.matrix_cross_distances(m, m, mode), "ward", ctx=ctx) for mode in ("jsd", "euclidean")}
        trees["mash"] = sk.linkage("complete")

        def run():
            out = {"host": cluster.cophenet(Z, D, matrix=True, ctx=ctx), "mash": sk.cophenet(trees["mash"], matrix=True)}
            for mode in ("jsd", "euclidean"):
                out[mode] = distance.matrix_cophenet(m, trees[mode], mode, matrix=True)
            return out

        whole = run()
        monkeypatch.setenv("DVS_CROSS_STRIP_ROWS", str(strip))
        for what, got in run().items():
            assert_same_scores(got, whole[what], f"{what}, strips of {strip}")
        assert_scores(whole["host"], D, Z, "host")
    finally:
        m.close()
        sk.close()


def test_two_calls_and_a_device_tensor_give_the_same_bits(ctx):
    """(where this is the first test of a process to put a tensor on the device, its time is torch's initialisation)"""
    torch = pytest.importorskip("torch")
    D = case_matrix(257, "random")
    Z = cluster.linkage(D, "weighted", ctx=ctx)
    first = cluster.cophenet(Z, D, matrix=True, ctx=ctx)
    assert_same_scores(first, cluster.cophenet(Z, D, matrix=True, ctx=ctx), "two calls")
    t = torch.from_numpy(D).to("cuda:0")
    got = cluster.cophenet(Z, t, matrix=True, ctx=ctx)
    assert np.array_equal(t.cpu().numpy(), D)  # read, not overwritten
    assert_same_scores(got, first, "device tensor")
    plain = cluster.cophenet(Z, D, ctx=ctx)  # without the matrix: the same sums
    assert plain.cophenetic is None and same_bits(plain.row_sums, first.row_sums)
    assert same_bits([plain.correlation], [first.correlation])


def _assert_mode_equals_matrix_path(ctx, got, d, Z, what):
    """the strips' sums against cluster.cophenet on the matrix the cross entry returns for the same rows, its diagonal
    overwritten: cell (i, i) is never read"""
    d = d.copy()
    np.fill_diagonal(d, 7.0)
    assert_same_scores(got, cluster.cophenet(Z, d, matrix=got.cophenetic is not None, ctx=ctx), what)
    assert_scores(got, d, Z, what)


def test_handle_entries_same_bits_as_the_matrix_path(ctx):
    seqs = _mode_seqs()
    rows = np.random.default_rng(22).permutation(80)[:65]  # permutes, and drops 15 rows
    m = ctx.build_matrix(seqs, 3, 4)
    sk = distance.Sketches(seqs, 9, 120, ctx=ctx)
    try:
        for mode in ("jsd", "euclidean"):
            d = distance.matrix_cross_distances(m, m, mode, q_rows=rows, r_rows=rows)
            Z = cluster.linkage(d, "average", ctx=ctx)
            _assert_mode_equals_matrix_path(ctx, distance.matrix_cophenet(m, Z, mode, rows=rows, matrix=True), d, Z, mode)
        d = sk.cross_distances(sk, rows=rows, other_rows=rows)
        Z = cluster.linkage(d, "average", ctx=ctx)
        _assert_mode_equals_matrix_path(ctx, sk.cophenet(Z, rows=rows, matrix=True), d, Z, "mash")
    finally:
        m.close()
        sk.close()


# ------------------------------------------------------------------ 3. the three modes over the family sequences
@pytest.mark.parametrize("case", FAMILY_CASES, ids=["k4", "k6"])
def test_modes_over_family_sequences(ctx, case):
    nfam, per, length, seed, k = case
    seqs = list(family_seqs(nfam, per, length, seed).values())
    n = len(seqs)
    rows = np.random.default_rng(seed).permutation(n)[: n - 7]
    sub = [seqs[i] for i in rows]
    for mode, kw in (("jsd", dict(k=k)), ("euclidean", dict(k=k)), ("mash", dict(k=12, sketch_size=200))):
        d = distance.MODES[mode][0](seqs, *distance.mode_args(mode, kw["k"], kw.get("sketch_size"), 4, False), ctx=ctx)
        # every row, through the public function
        Z = cluster.linkage(d, "average", ctx=ctx)
        assert_scores(distance.cophenet(seqs, Z, mode, ctx=ctx, **kw), d, Z, f"{mode} k={kw['k']} all rows")
        # a row list, through the handle
        ds = d[np.ix_(rows, rows)]
        Zs = cluster.linkage(ds, "complete", ctx=ctx)
        with distance.device_side(seqs, mode, *distance.mode_args(mode, kw["k"], kw.get("sketch_size"), 4, False), ctx=ctx) as dev:
            got = dev.cophenet(Zs, rows=rows)
            assert_scores(got, ds, Zs, f"{mode} k={kw['k']} row list")
            whole = dev.cophenet(Z)
        assert_same_scores(whole, distance.cophenet(seqs, Z, mode, ctx=ctx, **kw), f"{mode} DeviceSide.cophenet")
        assert_same_scores(got, distance.cophenet(sub, Zs, mode, ctx=ctx, **kw), f"{mode} the listed rows as a batch")


def test_an_empty_sketch_is_a_zero_division(ctx):
    rng = np.random.default_rng(2)
    short = [np.zeros(3, np.uint8), rng.integers(0, 4, 80, dtype=np.uint8), rng.integers(0, 4, 90, dtype=np.uint8)]
    Z3, Z2 = np.array([[1, 2, 0.5, 2], [0, 3, 1.0, 3]]), np.array([[0, 1, 1.0, 2]])
    sk = distance.Sketches(short, 8, 10, ctx=ctx)
    try:
        with pytest.raises(ZeroDivisionError):
            sk.cophenet(Z3)
        with pytest.raises(ZeroDivisionError):  # one is enough: the strips hold a row against itself
            sk.cophenet(Z2, rows=[0, 1])
        assert np.isnan(sk.cophenet(Z2, rows=[1, 2]).correlation)  # without it the call goes through (n = 2: NaN)
    finally:
        sk.close()
    with pytest.raises(ZeroDivisionError):
        distance.cophenet(short, Z3, "mash", k=8, sketch_size=10, ctx=ctx)


# ------------------------------------------------------------------ 4. end to end on BRCA1
def test_ctree_cophenet_compare_linkages_and_the_app_on_brca1(ctx, brca1):
    raw = read_fasta(GOLDEN / "brca1.fasta")
    text = {n: s.replace("-", "").replace("?", "") for n, s in raw.items()}
    names = list(text)
    seqs = {n: brca1[n] for n in names}
    n = len(names)
    d = distance.mash_distances([seqs[x] for x in names], 12, 3000, ctx=ctx)  # the host-copied matrix
    both = cluster.compare_linkages(seqs)
    assert list(both) == list(METHODS)
    for method in METHODS:
        newick, Z, sc = cluster.ctree_cophenet(seqs, linkage=method)
        assert newick == cluster.ctree(seqs, linkage=method)
        assert_scores(sc, d, Z, f"brca1 mash {method}")
        assert sc.cophenetic is None
        Zc, rc = both[method]
        assert np.array_equal(Zc, Z) and same_bits([rc], [sc.correlation]), method  # five separate calls, bit for bit
    with_matrix = cluster.ctree_cophenet(seqs, linkage="average", matrix=True)[2]
    assert same_bits(with_matrix.cophenetic, squareform(scipy_cophenet(both["average"][0])))
    out = apps.dvs_cophenet(distance_mode="mash", k=12)(text)
    assert set(out) == {"best", "correlation", "tree"}
    assert out["correlation"] == {method: both[method][1] for method in METHODS}
    assert all(isinstance(v, float) for v in out["correlation"].values())
    with np.errstate(invalid="ignore", divide="ignore"):
        sp = {method: float(scipy_cophenet(both[method][0], condensed(d))[0]) for method in METHODS}
    ranked = sorted(sp.values())
    assert ranked[-1] - ranked[-2] > 1000 * bound(n)  # (the best method of this case does not hang on rounding)
    assert out["best"] == max(sp, key=sp.get) and out["tree"] == cluster.ctree(seqs, linkage=out["best"])
    # another mode through the same calls
    newick, Z, sc = cluster.ctree_cophenet(seqs, linkage="ward", distance_mode="jsd", k=5, sketch_size=None)
    dj = distance.jsd_distances([seqs[x] for x in names], 5, ctx=ctx)
    assert newick == cluster.ctree(seqs, linkage="ward", distance_mode="jsd", k=5, sketch_size=None)
    assert_scores(sc, dj, Z, "brca1 jsd ward")
    one = apps.dvs_cophenet("ward", distance_mode="jsd", k=5)(text)
    assert one["best"] == "ward" and one["correlation"] == {"ward": sc.correlation} and one["tree"] == newick


# ------------------------------------------------------------------ 5. errors
def test_errors(ctx):
    torch = pytest.importorskip("torch")
    D = case_matrix(65, "random")
    Z = scipy_linkage(condensed(D), "average")
    for bad in (Z[:-1], Z[:, :3], np.zeros((0, 4))):
        with pytest.raises(ValueError, match="shape"):
            cluster.cophenet(bad, D, ctx=ctx)
    with pytest.raises(ValueError, match="square"):
        cluster.cophenet(Z, D[:, :-1], ctx=ctx)
    with pytest.raises(ValueError, match="square, contiguous float64"):
        cluster.cophenet(Z, torch.zeros((65, 65), dtype=torch.float32, device="cuda:0"), ctx=ctx)
    with pytest.raises(ValueError, match="square, contiguous float64"):
        cluster.cophenet(Z, torch.zeros((65, 64), dtype=torch.float64, device="cuda:0"), ctx=ctx)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="on device 1"):
            cluster.cophenet(Z, torch.from_numpy(D).to("cuda:1"), ctx=ctx)
    twice = Z.copy()
    twice[1, :2] = twice[0, :2]
    with pytest.raises(ValueError, match="not two clusters that exist"):
        cluster.cophenet(twice, D, ctx=ctx)
    empty = cluster.cophenet(np.zeros((0, 4)), np.zeros((0, 0)), matrix=True, ctx=ctx)  # n = 0: empty outputs
    assert np.isnan(empty.correlation) and empty.row_sums.shape == (5, 0) and empty.cophenetic.shape == (0, 0)
    # the C entries' own checks
    L = ctx._L
    u32 = lambda a: _lib.ptr(a, C.c_uint32)  # noqa: E731
    f64 = lambda a: _lib.ptr(a, C.c_double)  # noqa: E731
    pairs, heights = np.ascontiguousarray(Z[:, :2], dtype=np.uint32).reshape(-1), np.ascontiguousarray(Z[:, 2])
    corr = C.c_double(-2.0)

    def host(n, p=pairs, on_device=0, corr_=C.byref(corr)):
        given = distance.make_source(_lib.SRC_GIVEN, D.ctypes.data, n, on_device=on_device)
        return L.dvs_cophenet(ctx._h, given, u32(p), f64(heights), corr_, None, None)

    assert host(65) == _lib.OK  # every output but the correlation left out
    assert abs(corr.value - truth_correlation(D, Z)) <= bound(65)
    corr.value = -2.0
    assert host(0) == _lib.OK and corr.value == -2.0  # nothing to do, nothing written
    assert host(1) == _lib.ERR_VALUE                  # one leaf has no tree
    assert host(65, corr_=None) == _lib.ERR_VALUE
    assert host(65, np.ascontiguousarray(twice[:, :2], dtype=np.uint32).reshape(-1)) == _lib.ERR_VALUE
    assert host(65, on_device=1) == _lib.ERR_VALUE    # a host array is not device memory
    big = 65535 * 8 + 1
    assert L.dvs_cophenet(ctx._h, distance.make_source(_lib.SRC_GIVEN, D.ctypes.data, big), u32(np.zeros(2 * big, np.uint32)),
                          f64(np.zeros(big)), C.byref(corr), None, None) == _lib.ERR_UNSUPPORTED
    seqs = _mode_seqs(25, 10)
    m = ctx.build_matrix(seqs, 3, 4)
    try:
        Z10 = scipy_linkage(condensed(case_matrix(10, "random")), "average")
        p10, h10 = np.ascontiguousarray(Z10[:, :2], dtype=np.uint32).reshape(-1), np.ascontiguousarray(Z10[:, 2])
        for kind in (_lib.SRC_JSD, _lib.SRC_EUCLIDEAN):
            def f(n, p, h, rows=None):
                return L.dvs_cophenet(ctx._h, distance.make_source(kind, m._h, n, rows), u32(p), f64(h), C.byref(corr), None, None)

            assert f(10, p10, h10) == _lib.OK
            assert f(11, np.r_[p10, 0, 18].astype(np.uint32), np.r_[h10, 2.0]) == _lib.ERR_VALUE  # 11 rows of a handle that holds 10
            assert f(2, np.array([0, 1], np.uint32), h10, np.array([0, 10], np.uint32)) == _lib.ERR_VALUE
            assert f(0, p10, h10) == _lib.OK
        with pytest.raises(ValueError, match="row list"):
            distance.matrix_cophenet(m, Z10[:1], "jsd", rows=[0, 10])
        with pytest.raises(ValueError, match="Unexpected distance"):
            distance.matrix_cophenet(m, Z10, "mash")
        with pytest.raises(ValueError, match="shape"):
            distance.matrix_cophenet(m, Z10[:-1], "jsd")
        assert np.isfinite(distance.matrix_cophenet(m, Z10, "jsd").correlation)  # the context is usable afterwards
    finally:
        m.close()
