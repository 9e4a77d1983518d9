"""Flat clusters of a tree and the scores of a labelling, without a GPU: the public names, `cluster.cut_tree` (host
code) against scipy's fcluster as partitions, the long-double yardstick of the scores (`truth_cluster_scores`, straight
from the definitions in include/dvs_hip.h "flat clusters"), sklearn's silhouettes against it, and the cases of
tests/test_gpu_clusters.py with their preconditions pinned here: on the random cases no neighbour and no medoid is
decided by rounding (every runner-up is more than GAP_FACTOR x the bound away), and the tie case's sums are exact."""
import numpy as np
import pytest
from scipy.cluster.hierarchy import fcluster
from scipy.cluster.hierarchy import linkage as scipy_linkage

from diverseseq_amd import _lib, apps, cluster, distance
from test_cross_host import GAP_FACTOR, _NoContext

METHODS = ("single", "complete", "average", "weighted", "ward")
CUT_SIZES = (2, 3, 5, 33, 97, 300)


def bound(n: int) -> float:
    """(n + 8) 2^-52: at most n - 1 additions and three roundings (a quotient, a difference, a quotient) per quantity;
    relative for within, a and b, absolute for the silhouette (which lies in [-1, 1])"""
    return (n + 8) * 2.0 ** -52


def first_appearance(labels) -> np.ndarray:
    """a labelling renumbered by first appearance: equal results <=> equal partitions"""
    seen: dict = {}
    return np.array([seen.setdefault(int(l), len(seen)) for l in labels], dtype=np.int64)


# ------------------------------------------------------------------ the names
def test_public_names_exist():
    for name in ("ClusterScores", "cluster_scores", "matrix_cluster_scores"):
        assert hasattr(distance, name), name
    assert callable(distance.Sketches.cluster_scores)
    for name in ("cut_tree", "cluster_scores", "ctree_clusters"):
        assert callable(getattr(cluster, name, None)), name
    assert callable(apps.dvs_clusters) and "dvs_clusters" in apps.__all__
    assert distance.ClusterScores._fields == ("labels", "within", "a", "b", "neighbour", "silhouette", "sizes", "medoids",
                                              "cluster_silhouette", "mean_silhouette")
    new = {"dvs_linkage_cut", "dvs_cluster_scores"}  # one entry for the scores: the mode travels in the dvs_source
    assert new <= set(_lib.EXPORTS)
    lib = _lib.load()
    for name in new:
        assert getattr(lib, name).argtypes is not None, name
    assert lib.dvs_abi_version() == 5


# ------------------------------------------------------------------ cut_tree against scipy
def cut_matrix(n: int, tied: bool, seed: int) -> np.ndarray:
    """the condensed euclidean distances of n random points; tied: rounded to quarters (never to 0)"""
    rng = np.random.default_rng(seed)
    x = rng.random((n, 3)) * 2.0
    d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2))[np.triu_indices(n, 1)]
    return np.maximum(np.round(d * 4.0), 1.0) / 4.0 if tied else d


def cut_values(Z: np.ndarray):
    """(the K of the issue, its heights) for a linkage matrix"""
    n = Z.shape[0] + 1
    ks = sorted({k for k in (1, 2, 3, n // 2, n - 1, n, n + 5) if k >= 1})
    h = np.unique(Z[:, 2])
    ts = [0.0, *h[:6].tolist(), float(np.median(Z[:, 2])), float(Z[-1, 2]), 2.0 * float(Z[-1, 2])]
    return ks, ts


def assert_cuts_match_scipy(Z: np.ndarray) -> int:
    ks, ts = cut_values(Z)
    n = Z.shape[0] + 1
    for K in ks:
        got = cluster.cut_tree(Z, n_clusters=K)
        assert got.dtype == np.int64 and got.shape == (n,) and got[0] == 0
        np.testing.assert_array_equal(got, first_appearance(fcluster(Z, K, "maxclust")), err_msg=f"n={n} K={K}")
        np.testing.assert_array_equal(got, first_appearance(got))  # numbered by first appearance
        assert got.max() + 1 <= K
    for t in ts:
        got = cluster.cut_tree(Z, height=t)
        np.testing.assert_array_equal(got, first_appearance(fcluster(Z, t, "distance")), err_msg=f"n={n} t={t}")
    return len(ks) + len(ts)


@pytest.mark.parametrize("tied", [False, True], ids=["untied", "tied"])
@pytest.mark.parametrize("method", METHODS)
def test_cut_tree_is_scipys_partition(method, tied):
    cuts = 0
    for n in CUT_SIZES:
        Z = scipy_linkage(cut_matrix(n, tied, 100 * n + len(method)), method)
        if tied and n >= 33:
            assert np.unique(Z[:, 2]).size < n - 1  # (there are merges of equal height to keep together)
        cuts += assert_cuts_match_scipy(Z)
    assert cuts >= 6 * 12


def test_cut_tree_keeps_equal_heights_together():
    Z = np.array([[0, 1, 1.0, 2], [2, 3, 1.0, 2], [4, 5, 2.0, 4]])
    assert cluster.cut_tree(Z, n_clusters=3).tolist() == [0, 0, 1, 1]  # (never three: the two merges share a height)
    assert cluster.cut_tree(Z, n_clusters=4).tolist() == [0, 1, 2, 3]
    assert cluster.cut_tree(Z, n_clusters=2).tolist() == [0, 0, 1, 1]
    assert cluster.cut_tree(Z, n_clusters=1).tolist() == [0, 0, 0, 0]
    assert cluster.cut_tree(Z, height=0.5).tolist() == [0, 1, 2, 3]
    assert cluster.cut_tree(Z, height=1.0).tolist() == [0, 0, 1, 1]


def test_cut_tree_argument_errors():
    Z = scipy_linkage(cut_matrix(6, False, 1), "average")
    for kw in ({}, dict(n_clusters=2, height=1.0)):
        with pytest.raises(ValueError, match="exactly one"):
            cluster.cut_tree(Z, **kw)
    for bad in (0, -1, 1.5, "2", True):
        with pytest.raises(ValueError, match="n_clusters"):
            cluster.cut_tree(Z, n_clusters=bad)
    with pytest.raises(ValueError, match="NaN"):
        cluster.cut_tree(Z, height=float("nan"))
    for shape in ((5, 3), (0, 4), (4,)):
        with pytest.raises(ValueError, match="shape"):
            cluster.cut_tree(np.zeros(shape), n_clusters=2)
    down = Z.copy()
    down[3, 2] = 0.0
    with pytest.raises(ValueError, match="must not decrease"):
        cluster.cut_tree(down, n_clusters=2)
    nan_h = Z.copy()
    nan_h[0, 2] = np.nan
    with pytest.raises(ValueError, match="must not decrease"):
        cluster.cut_tree(nan_h, height=1.0)
    for where, value in (((0, 0), 40.0), ((0, 1), -1.0), ((1, 0), 0.5), ((2, 1), np.inf)):
        kids = Z.copy()
        kids[where] = value
        with pytest.raises(ValueError, match="cluster ids"):
            cluster.cut_tree(kids, n_clusters=2)
    twice = Z.copy()
    twice[1, :2] = twice[0, :2]  # merges two clusters that are gone already
    with pytest.raises(ValueError, match="not two clusters that exist"):
        cluster.cut_tree(twice, n_clusters=1)
    # the C entry's own checks (no context: a NULL one only loses the message)
    C = __import__("ctypes")
    L = _lib.load()
    pairs, heights = np.ascontiguousarray(Z[:, :2], dtype=np.uint32).reshape(-1), np.ascontiguousarray(Z[:, 2])
    out, count = np.zeros(6, np.uint32), C.c_uint32()

    def raw(n, criterion, value):
        return L.dvs_linkage_cut(None, n, _lib.ptr(pairs, C.c_uint32), _lib.ptr(heights, C.c_double), criterion, value,
                                 _lib.ptr(out, C.c_uint32), C.byref(count))

    assert raw(6, _lib.CUT_NCLUSTERS, 2.0) == _lib.OK and count.value == 2
    assert raw(1, _lib.CUT_NCLUSTERS, 1.0) == _lib.ERR_VALUE
    assert raw(0, _lib.CUT_HEIGHT, 1.0) == _lib.ERR_VALUE
    assert raw(6, _lib.CUT_NCLUSTERS, 0.0) == _lib.ERR_VALUE
    assert raw(6, _lib.CUT_NCLUSTERS, 2.5) == _lib.ERR_VALUE
    assert raw(6, _lib.CUT_NCLUSTERS, float("nan")) == _lib.ERR_VALUE
    assert raw(6, _lib.CUT_HEIGHT, float("nan")) == _lib.ERR_VALUE
    assert raw(6, 2, 1.0) == _lib.ERR_VALUE
    assert raw(6, _lib.CUT_NCLUSTERS, 11.0) == _lib.OK and count.value == 6 and out.tolist() == list(range(6))


def test_score_argument_errors_need_no_context():
    ctx = _NoContext()
    a = [np.zeros(30, np.uint8), np.ones(30, np.uint8), np.arange(30, dtype=np.uint8) % 4]
    with pytest.raises(ValueError, match="Unexpected distance 'manhattan'"):
        distance.cluster_scores(a, [0, 0, 1], "manhattan", k=3, ctx=ctx)
    with pytest.raises(ValueError, match="Expected sketch size"):
        distance.cluster_scores(a, [0, 0, 1], "mash", k=3, ctx=ctx)
    with pytest.raises(ValueError, match="Sketch size"):
        distance.cluster_scores(a, [0, 0, 1], "jsd", k=3, sketch_size=10, ctx=ctx)
    d = np.zeros((3, 3))
    for fn in (lambda l: distance.cluster_scores(a, l, "jsd", k=3, ctx=ctx), lambda l: cluster.cluster_scores(d, l, ctx=ctx)):
        for bad in ([0, 1], [0, 1, 2, 3], [[0, 1, 2]], [0.0, 1.0, 2.0]):
            with pytest.raises(ValueError, match="labels"):
                fn(bad)
        for bad in ([0, -1, 1], [0, 1, 2 ** 32 - 1]):
            with pytest.raises(ValueError, match="label out of range"):
                fn(bad)
    for shape in ((3, 4), (9,), (2, 2, 2)):
        with pytest.raises(ValueError, match="square"):
            cluster.cluster_scores(np.zeros(shape), [0, 1, 2], ctx=ctx)
    empty = cluster.cluster_scores(np.zeros((0, 0)), [], ctx=ctx)  # nothing to compute: no device work either
    assert empty.within.shape == (0,) and empty.sizes.shape == (0,) and np.isnan(empty.mean_silhouette)
    seqs = {"a": a[0], "b": a[1], "c": a[2]}
    for kw in ({}, dict(n_clusters=2, height=0.5)):
        with pytest.raises(ValueError, match="exactly one"):
            cluster.ctree_clusters(seqs, **kw)
        with pytest.raises(ValueError, match="exactly one"):
            apps.dvs_clusters(**kw)
    with pytest.raises(ValueError, match="Unexpected distance 'manhattan'"):
        apps.dvs_clusters(2, distance_mode="manhattan")
    with pytest.raises(ValueError, match="Expected sketch size for mash distance measure"):
        apps.dvs_clusters(2, sketch_size=None)
    with pytest.raises(ValueError, match="Canonical kmers only supported for dna sequences"):
        apps.dvs_clusters(2, moltype="protein", mash_canonical_kmers=True)
    with pytest.raises(ValueError, match="not built on the device"):
        apps.dvs_clusters(2, linkage="centroid")
    with pytest.raises(ValueError, match="n_clusters"):
        apps.dvs_clusters(0)


# ------------------------------------------------------------------ the yardstick
def truth_cluster_scores(D, labels, n_clusters=None, dtype=np.longdouble) -> dict:
    """The scores of a labelling straight from their definitions, in `dtype` arithmetic (long double: the yardstick;
    float64: what the device must return bit for bit where every sum is exact, as in the tie case).

    within_i = sum of D(i, j) over the other members j of i's cluster (cell (i, i) is never added, whatever it holds);
    a_i = within_i / (n_c - 1), 0 in a cluster of one; b_i = the least S(i, c) / n_c over the non-empty clusters c other
    than i's own, neighbour_i that c (a tie to the lower c, a NaN mean never taken; nothing to take: NaN and -1);
    silhouette_i = 0 in a cluster of one or when a = b = 0, else (b - a) / max(a, b); medoid_c = the member of c with the
    least within (a tie to the lowest row, NaN never taken, -1 where there is none)."""
    lab = np.asarray(labels, dtype=np.int64)
    n = lab.size
    K = int(lab.max()) + 1 if n_clusters is None else n_clusters
    Dz = np.array(D, dtype=dtype).reshape(n, n)
    np.fill_diagonal(Dz, 0)
    sizes = np.bincount(lab, minlength=K).astype(np.int64)
    order = np.argsort(lab, kind="stable")
    nonempty = np.flatnonzero(sizes)
    starts = np.concatenate([[0], np.cumsum(sizes)])[nonempty]
    S = np.full((n, K), np.nan, dtype=dtype)  # S(i, c); NaN in the column of an empty cluster
    S[:, nonempty] = np.add.reduceat(Dz[:, order], starts, axis=1)
    rows = np.arange(n)
    within = S[rows, lab].copy()
    own = sizes[lab]
    a = np.where(own > 1, within / np.maximum(own - 1, 1).astype(dtype), dtype(0))
    with np.errstate(invalid="ignore", divide="ignore"):
        means = S / sizes.astype(dtype)[None, :]
    means[rows, lab] = np.nan
    b = np.full(n, np.nan, dtype=dtype)
    neighbour = np.full(n, -1, dtype=np.int64)
    for i in rows:
        ok = np.flatnonzero(~np.isnan(means[i]))
        if ok.size:
            c = ok[np.argmin(means[i][ok])]  # (the first of equal minima: the lower cluster)
            neighbour[i], b[i] = c, means[i][c]
    with np.errstate(invalid="ignore", divide="ignore"):
        sil = (b - a) / np.where(a > b, a, b)
    sil[(a == 0) & (b == 0)] = 0
    sil[own == 1] = 0
    medoids = np.full(K, -1, dtype=np.int64)
    for c in nonempty:
        members = np.flatnonzero(lab == c)
        members = members[~np.isnan(within[members])]
        if members.size:
            medoids[c] = members[np.argmin(within[members])]
    return dict(within=within, a=a, b=b, neighbour=neighbour, silhouette=sil, sizes=sizes, medoids=medoids, means=means)


def smallest_relative_gaps(truth: dict, labels) -> tuple:
    """(the smallest relative gap between a row's best and second-best cluster mean, the smallest between the two
    least `within` of a cluster), over every row and every cluster that has a runner-up: inf where none has"""
    lab = np.asarray(labels)
    g_mean = g_within = np.inf
    for row in truth["means"]:
        v = np.sort(row[~np.isnan(row)])
        if v.size >= 2:
            g_mean = min(g_mean, float((v[1] - v[0]) / v[1]))
    for c in np.flatnonzero(truth["sizes"] >= 2):
        w = truth["within"][lab == c]
        w = np.sort(w[~np.isnan(w)])
        if w.size >= 2:
            g_within = min(g_within, float((w[1] - w[0]) / w[1]))
    return g_mean, g_within


def random_matrix(n: int, seed: int) -> np.ndarray:
    """cells in [0.05, 1), a zero diagonal; NOT symmetric: a row's sums read that row only (as sklearn's do), and in a
    symmetric matrix the two members of a cluster of two would tie for its medoid with one and the same cell"""
    d = np.random.default_rng(seed).uniform(0.05, 1.0, (n, n))
    np.fill_diagonal(d, 0.0)
    return d


def sklearn_silhouettes(D, labels) -> np.ndarray:
    from sklearn.metrics import silhouette_samples

    return silhouette_samples(np.asarray(D, dtype=np.float64), np.asarray(labels), metric="precomputed")


# ------------------------------------------------------------------ sklearn against the yardstick
@pytest.mark.parametrize("n", [5, 64, 65, 300, 1000])
def test_sklearn_lies_within_the_bound_of_the_yardstick(n):
    rng = np.random.default_rng(n)
    D = random_matrix(n, 7 * n)
    labels = rng.integers(0, max(2, min(n // 3, 12)), size=n)
    labels[labels == labels[0]] = labels.max() + 2  # (renamed, so that the next line makes row 0 ...)
    labels[0] = labels.max() + 1                    # ... the one member of a cluster of its own
    truth = truth_cluster_scores(D, labels)
    assert truth["sizes"][labels[0]] == 1 and truth["silhouette"][0] == 0
    err = np.abs(sklearn_silhouettes(D, labels).astype(np.longdouble) - truth["silhouette"])
    print(f"n={n}: sklearn's largest |silhouette - truth| = {float(err.max()):.3g} = {float(err.max()) / bound(n):.3g} x bound")
    assert (err <= bound(n)).all()


# ------------------------------------------------------------------ the random cases of the GPU test
SCORE_SIZES = (1, 2, 3, 63, 64, 65, 257, 600)  # on both sides of one wave (64) and of one unrolled pass (256), several passes


def label_shapes(n: int, seed: int) -> dict:
    """the label shapes of the issue that n rows can carry; every one interleaved (shuffled over the rows)"""
    rng = np.random.default_rng(seed)
    shapes = {"one": np.zeros(n, dtype=np.int64), "singletons": rng.permutation(n)}
    if n >= 2:
        shapes["two"] = rng.permutation(np.arange(n) % 2)
    if n >= 3:
        giant = np.zeros(n, dtype=np.int64)
        loose = rng.choice(n, size=max(1, n // 8), replace=False)
        giant[loose] = 1 + np.arange(loose.size)
        shapes["giant"] = giant
    return shapes


def _sized(sizes, seed, gap_at=None):
    lab = np.concatenate([np.full(s, c) for c, s in enumerate(sizes)])
    if gap_at is not None:
        lab[lab >= gap_at] += 1  # a label in the middle that nobody carries
    return np.random.default_rng(seed).permutation(lab)


def score_cases() -> dict:
    """name -> (D, labels): random matrices under the label shapes of every size, and the mixed-size cases"""
    cases = {}
    for n in SCORE_SIZES:
        for shape, lab in label_shapes(n, 31 * n).items():
            cases[f"n{n}-{shape}"] = (random_matrix(n, n), lab)
    cases["sizes-1-63-64-65-300"] = (random_matrix(493, 11), _sized((1, 63, 64, 65, 300), 12))
    cases["empty-label-in-the-middle"] = (random_matrix(130, 13), _sized((40, 1, 24, 65), 14, gap_at=2))
    # the kernel's own threshold: a wave's 64 lanes take 4 positions each in one unrolled pass of the stride loop, 256
    # positions; clusters of 255, 256 and 257 members lie on both sides of it
    cases["sizes-255-256-257"] = (random_matrix(768, 15), _sized((255, 256, 257), 16))
    return cases


SCORE_CASES = score_cases()


def test_random_cases_are_decided_by_no_rounding():
    """every neighbour and every medoid of every random case may be compared exactly: no row is left out"""
    worst_mean = worst_within = np.inf
    for name, (D, lab) in SCORE_CASES.items():
        n = lab.size
        truth = truth_cluster_scores(D, lab)
        g_mean, g_within = smallest_relative_gaps(truth, lab)
        assert g_mean > GAP_FACTOR * bound(n) and g_within > GAP_FACTOR * bound(n), (name, g_mean, g_within)
        worst_mean, worst_within = min(worst_mean, g_mean), min(worst_within, g_within)
        assert np.array_equal(truth["sizes"], np.bincount(lab, minlength=truth["sizes"].size))
    print(f"smallest relative gaps over {len(SCORE_CASES)} cases: means {worst_mean:.3g}, within {worst_within:.3g}")
    assert "n1-one" in SCORE_CASES and "n600-giant" in SCORE_CASES and len(SCORE_CASES) >= 8 * 2 + 3
    lab = SCORE_CASES["empty-label-in-the-middle"][1]
    assert 2 not in lab and lab.max() == 4


# ------------------------------------------------------------------ the tie case
def tie_case():
    """(D 12 x 12 of multiples of 1/8, labels of three clusters of four): every sum is exact in any order; row 0 has
    exactly equal means to clusters 1 and 2, rows 9 and 10 exactly equal -- and least -- `within` in cluster 2"""
    rng = np.random.default_rng(5)
    u = rng.integers(9, 17, size=(12, 12)).astype(np.float64) / 8.0
    D = np.triu(u, 1)
    D[0, 4:8] = np.array([1, 2, 3, 4]) / 8.0
    D[0, 8:12] = np.array([4, 3, 2, 1]) / 8.0
    D[9, 10], D[8, 9], D[9, 11] = 1 / 8, 2 / 8, 3 / 8
    D[8, 10], D[10, 11] = 3 / 8, 2 / 8
    D[8, 11] = 1.0
    D = D + D.T
    return D, np.repeat(np.arange(3), 4)


def test_tie_case_expects_the_lower_cluster_and_the_lower_row():
    D, lab = tie_case()
    assert np.array_equal(D * 8, np.round(D * 8)) and np.array_equal(D, D.T) and D.max() <= 2.0
    exact, truth = truth_cluster_scores(D, lab, dtype=np.float64), truth_cluster_scores(D, lab)
    for key in ("within", "b"):  # sums of at most 11 multiples of 1/8, and quarters of them: exact in either arithmetic
        assert np.array_equal(exact[key].astype(np.longdouble), truth[key]), key
    assert exact["means"][0, 1] == exact["means"][0, 2] == 10 / 8 / 4
    assert exact["neighbour"][0] == 1  # the lower of the two
    assert exact["within"][9] == exact["within"][10] == 6 / 8 and exact["within"][8] == exact["within"][11] == 13 / 8
    assert exact["medoids"].tolist()[2] == 9  # the lower of the two
    assert np.array_equal(exact["neighbour"], truth["neighbour"]) and np.array_equal(exact["medoids"], truth["medoids"])
    # the same under labels 0, 1, 5: the tied clusters two places apart, labels 2 - 4 carried by nobody
    wide = np.where(lab == 2, 5, lab)
    e2 = truth_cluster_scores(D, wide, dtype=np.float64)
    assert e2["neighbour"][0] == 1 and e2["medoids"].tolist() == [exact["medoids"][0], exact["medoids"][1], -1, -1, -1, 9]
    assert np.array_equal(e2["silhouette"], exact["silhouette"])


def test_yardstick_rules_for_nan():
    """a NaN mean is never taken, a NaN `within` never a medoid; nothing to take: NaN / -1; the diagonal is never read"""
    D = random_matrix(6, 3)
    D[2, :] = D[:, 2] = np.nan
    np.fill_diagonal(D, 7.0)
    t = truth_cluster_scores(D, [0, 0, 1, 2, 2, 1])
    # cluster 1 holds row 2: its means are NaN for everyone else; row 2 itself has nothing to take
    assert t["neighbour"][[0, 1, 3, 4]].tolist() == [2, 2, 0, 0] and t["neighbour"][2] == -1 and t["neighbour"][5] in (0, 2)
    assert np.isnan(t["b"][2]) and np.isnan(t["silhouette"][[2, 5]]).all() and not np.isnan(t["a"][[0, 1, 3, 4]]).any()
    assert np.isnan(t["within"][[2, 5]]).all()
    assert t["within"][3] == np.longdouble(D[3, 4]) and t["within"][4] == np.longdouble(D[4, 3])  # (7.0 never added)
    assert t["medoids"].tolist() == [0 if D[0, 1] <= D[1, 0] else 1, -1, 3 if D[3, 4] <= D[4, 3] else 4]
    alone = truth_cluster_scores(D, [0, 0, 1, 2, 2, 2])  # the NaN row alone in its cluster: an empty sum
    assert alone["within"][2] == 0 and alone["a"][2] == 0 and np.isnan(alone["b"][2]) and alone["neighbour"][2] == -1
    assert alone["silhouette"][2] == 0 and alone["medoids"][1] == 2
    only = truth_cluster_scores(np.full((2, 2), np.nan), [0, 0])
    assert only["neighbour"].tolist() == [-1, -1] and only["medoids"].tolist() == [-1]
