"""Cophenetic distances and the cophenetic correlation, without a GPU: the public names, `cluster.cophenet(Z)` (host
code: the in-order walk and the range maximum of include/dvs_hip.h "cophenetic distances") against scipy's cophenet bit
for bit, the long-double yardstick of the correlation and of the five shifted row sums, and the cases of
tests/test_gpu_cophenet.py with what they must be able to tell apart pinned here: scipy's own cophenet(Z, Y) stays
within the bound on every case, and float64 raw moments miss it by more than 100 x on every saturated case of 33 leaves
or more -- so a device that meets the bound there has shifted its moments."""
import functools

import numpy as np
import pytest
from scipy.cluster.hierarchy import cophenet as scipy_cophenet
from scipy.cluster.hierarchy import linkage as scipy_linkage
from scipy.spatial.distance import squareform

from diverseseq_amd import _lib, apps, cluster, distance
from test_cross_host import _NoContext

METHODS = ("single", "complete", "average", "weighted", "ward")  # what the device builds
SCIPY_METHODS = METHODS + ("centroid", "median")                 # the last two: heights that are not monotone
HOST_SIZES = (2, 3, 5, 33, 65, 97, 257, 300)
# the GPU file's: one gap, a row at either end of the leaf order, the wave (64) and workgroup-chunk edges of the scan
# and one past them
GPU_SIZES = (2, 3, 5, 64, 65, 257, 300)
KINDS = ("random", "tied", "caterpillar", "saturated")
# The error of float64 raw moments is that of a handful of roundings magnified by the cancellation: large on the
# saturated kind, but a matter of luck case by case (over eight seeds its least figure among the cases of 33 leaves or
# more ran from 7 to 120 bounds).  The saturated matrices are the draw on which it exceeds 100 bounds on every one of
# them (test_raw_moments_miss_the_bound_on_every_saturated_case): chosen by that model alone, not by any device result.
KIND_SEED = {"saturated": 2}


def bound(n: int) -> float:
    """2 (n + 8) 2^-52, absolute on r: a row sum has at most n - 1 terms and three roundings, (n + 8) 2^-52 relative
    to the sum of its terms' magnitudes (DESIGN.md 4.10's argument); the shift keeps those magnitudes within a small
    multiple of the centred sums, and by Cauchy-Schwarz the relative errors of Sxy, Sxx and Syy reach r = Sxy /
    sqrt(Sxx Syy) as at most about twice that"""
    return 2 * (n + 8) * 2.0 ** -52


# ------------------------------------------------------------------ the matrices
def case_matrix(n: int, kind: str, seed: int = 0) -> np.ndarray:
    """a symmetric n x n matrix with a zero diagonal.  random: uniform in [0.05, 1); tied: multiples of 1/8 in [1/8, 1];
    caterpillar: |x_i - x_j| for points on a line with growing steps, in shuffled order (its single-linkage tree adds
    one leaf per merge); saturated: 1 - u / 128, u uniform in [0, 1): distances crowding under 1.0, as mash distances
    between unrelated sequences do"""
    rng = np.random.default_rng(1000 * n + 10 * KINDS.index(kind) + seed + KIND_SEED.get(kind, 0))
    if kind == "caterpillar":
        x = np.cumsum(1.0 + 0.01 * np.arange(n) + 0.001 * rng.random(n))[rng.permutation(n)]
        d = np.abs(x[:, None] - x[None, :])
    else:
        u = rng.random((n, n))
        if kind == "random":
            d = 0.05 + 0.95 * u
        elif kind == "tied":
            d = np.ceil(u * 8.0) / 8.0
            d[d == 0.0] = 0.125
        else:
            d = 1.0 - u / 128.0
        d = np.triu(d, 1)
        d = d + d.T
    np.fill_diagonal(d, 0.0)
    return d


def condensed(d: np.ndarray) -> np.ndarray:
    return d[np.triu_indices(d.shape[0], 1)]


# ------------------------------------------------------------------ the yardstick
def truth_correlation(D, Z) -> float:
    """Pearson's r between D(i, j) and scipy's cophenetic distances of Z over the upper triangle, from the definitions
    in 80-bit long double: both means first, then the centred sums.  NaN when either centred sum of squares is zero."""
    d = condensed(np.asarray(D)).astype(np.longdouble)
    c = scipy_cophenet(np.asarray(Z, dtype=np.float64)).astype(np.longdouble)
    dz, cz = d - d.sum() / d.size, c - c.sum() / c.size
    sxx, syy, sxy = (dz * dz).sum(), (cz * cz).sum(), (dz * cz).sum()
    if sxx == 0 or syy == 0:
        return float("nan")
    return float(sxy / np.sqrt(sxx * syy))


def c_bar_of(Z) -> float:
    """the mean cophenetic distance from Z alone, as the library states it: the merge of clusters of sizes s_a and s_b
    at height h holds s_a s_b pairs at h; summed in merge order in long double, divided by n (n - 1) / 2, rounded"""
    z = np.asarray(Z, dtype=np.float64)
    n = z.shape[0] + 1
    size = lambda c: 1 if c < n else int(z[int(c) - n, 3])  # noqa: E731
    total = np.longdouble(0)
    for a, b, h, _ in z:
        total += np.longdouble(size(a) * size(b)) * np.longdouble(h)
    return float(total / (np.longdouble(n) * np.longdouble(n - 1) / np.longdouble(2)))


def truth_row_sums(D, Z):
    """(the five shifted row sums [5, n] in long double: x, y, x x, y y, x y with x = D(i, j) - c_bar, y = coph(i, j) -
    c_bar over j != i; the sums of the terms' magnitudes, what a sum's rounding error is relative to)"""
    n = np.asarray(D).shape[0]
    off = ~np.eye(n, dtype=bool)
    cb = np.longdouble(c_bar_of(Z))
    x = np.where(off, np.asarray(D, dtype=np.float64).astype(np.longdouble) - cb, 0)
    y = np.where(off, squareform(scipy_cophenet(np.asarray(Z, dtype=np.float64))).astype(np.longdouble) - cb, 0)
    terms = (x, y, x * x, y * y, x * y)
    return np.stack([t.sum(axis=1) for t in terms]), np.stack([np.abs(t).sum(axis=1) for t in terms])


def correlation_from_row_sums(sums, n: int) -> float:
    """r from the 5 n row sums over the M = n (n - 1) ordered pairs, in long double (the library's host combine)"""
    s = np.asarray(sums, dtype=np.longdouble).sum(axis=1)
    M = np.longdouble(n) * np.longdouble(n - 1)
    sxx, syy, sxy = s[2] - s[0] * s[0] / M, s[3] - s[1] * s[1] / M, s[4] - s[0] * s[1] / M
    return float(sxy / np.sqrt(sxx * syy))


def raw_moments_correlation(D, Z) -> float:
    """the naive form in float64: (N sum dc - sum d sum c) / sqrt((N sum dd - (sum d)^2) (N sum cc - (sum c)^2))"""
    d, c = condensed(np.asarray(D, dtype=np.float64)), scipy_cophenet(np.asarray(Z, dtype=np.float64))
    N = float(d.size)
    sd, sc, sdd, scc, sdc = d.sum(), c.sum(), (d * d).sum(), (c * c).sum(), (d * c).sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        return float((N * sdc - sd * sc) / np.sqrt((N * sdd - sd * sd) * (N * scc - sc * sc)))


@functools.lru_cache(maxsize=None)
def gpu_case(n: int, kind: str, method: str):
    """(D, Z of scipy's linkage -- the device's `cluster.linkage` returns the same matrix bit for bit --, the yardstick's
    r): computed once, shared, left unchanged"""
    D = case_matrix(n, kind)
    Z = scipy_linkage(condensed(D), method)
    D.setflags(write=False)
    Z.setflags(write=False)
    return D, Z, truth_correlation(D, Z)


# ------------------------------------------------------------------ the names
def test_public_names_exist():
    for name in ("CopheneticScores", "cophenet", "matrix_cophenet", "DeviceSide", "check_linkage_matrix"):
        assert hasattr(distance, name), name
    assert callable(distance.DeviceSide.cophenet)
    assert callable(distance.Sketches.cophenet)
    for name in ("cophenet", "ctree_cophenet", "compare_linkages"):
        assert callable(getattr(cluster, name, None)), name
    assert callable(apps.dvs_cophenet) and "dvs_cophenet" in apps.__all__
    assert distance.CopheneticScores._fields == ("correlation", "row_sums", "cophenetic")
    new = {"dvs_linkage_cophenet", "dvs_cophenet"}  # one entry for the correlation: the mode travels in the dvs_source
    assert new <= set(_lib.EXPORTS)
    lib = _lib.load()
    for name in new:
        assert getattr(lib, name).argtypes is not None, name
    assert lib.dvs_abi_version() == 5


# ------------------------------------------------------------------ cluster.cophenet(Z) against scipy, bit for bit
def assert_cophenetic_is_scipys(Z, what=""):
    got = cluster.cophenet(Z)
    n = np.asarray(Z).shape[0] + 1
    assert got.dtype == np.float64 and got.shape == (n, n), what
    exp = squareform(scipy_cophenet(np.asarray(Z, dtype=np.float64)))
    assert np.array_equal(got.view(np.uint64), exp.view(np.uint64)), what


@pytest.mark.parametrize("tied", [False, True], ids=["untied", "tied"])
@pytest.mark.parametrize("method", SCIPY_METHODS)
def test_host_cophenetic_matrix_is_scipys(method, tied):
    non_monotone = 0
    for n in HOST_SIZES:
        Z = scipy_linkage(condensed(case_matrix(n, "tied" if tied else "random")), method)
        non_monotone += bool((np.diff(Z[:, 2]) < 0).any())
        assert_cophenetic_is_scipys(Z, f"{method} n={n} tied={tied}")
    if method in ("centroid", "median"):
        assert non_monotone >= 3  # (these trees really have heights that decrease: no monotone rule is relied on)


def test_host_cophenetic_matrix_of_a_caterpillar_and_of_swapped_children():
    for n in HOST_SIZES:
        Z = scipy_linkage(condensed(case_matrix(n, "caterpillar")), "single")
        if n >= 3:
            assert (Z[1:, :2].max(axis=1) == n + np.arange(n - 2)).all()  # every merge adds one leaf to the last cluster
        assert_cophenetic_is_scipys(Z, f"caterpillar n={n}")
        for method in ("average", "centroid"):
            Z = scipy_linkage(condensed(case_matrix(n, "random", seed=1)), method)
            swapped = Z.copy()
            swapped[::2, :2] = swapped[::2, 1::-1]  # every other merge names its children right to left
            assert not np.array_equal(swapped, Z)
            assert_cophenetic_is_scipys(swapped, f"swapped {method} n={n}")
            assert np.array_equal(cluster.cophenet(swapped), cluster.cophenet(Z))
    deep = 5000  # (iterative: no recursion limit)
    Z = np.column_stack([np.r_[0, deep + np.arange(deep - 2)], 1 + np.arange(deep - 1), 1.0 + np.arange(deep - 1),
                         2 + np.arange(deep - 1)]).astype(np.float64)
    got = cluster.cophenet(Z)
    i, j = np.triu_indices(deep, 1)
    assert np.array_equal(got[i, j], j.astype(np.float64)) and np.array_equal(got, got.T)  # leaf j joins at merge j - 1


def test_malformed_trees_are_value_errors():
    Z = scipy_linkage(condensed(case_matrix(6, "random")), "average")
    twice = Z.copy()
    twice[1, :2] = twice[0, :2]  # children that are gone already
    same = Z.copy()
    same[0, 1] = same[0, 0]  # one child twice in one merge
    early = Z.copy()
    early[0, 0] = 8.0  # merge 0 names cluster 8, which merge 2 makes
    for bad in (twice, same, early):
        with pytest.raises(ValueError, match="not two clusters that exist"):
            cluster.cophenet(bad)
    for shape in ((0, 4), (5, 3), (4,), (2, 2, 4)):  # (0, 4): the tree of one leaf
        with pytest.raises(ValueError, match="shape"):
            cluster.cophenet(np.zeros(shape))
    for where, value in (((0, 0), 40.0), ((0, 1), -1.0), ((1, 0), 0.5), ((2, 1), np.inf)):
        kids = Z.copy()
        kids[where] = value
        with pytest.raises(ValueError, match="cluster ids"):
            cluster.cophenet(kids)
    # the C entry's own checks (no context: a NULL one only loses the message)
    C = __import__("ctypes")
    L = _lib.load()
    pairs, heights = np.ascontiguousarray(Z[:, :2], dtype=np.uint32).reshape(-1), np.ascontiguousarray(Z[:, 2])
    out = np.full((6, 6), 3.0)
    raw = lambda n, p=pairs: L.dvs_linkage_cophenet(None, n, _lib.ptr(p, C.c_uint32), _lib.ptr(heights, C.c_double),  # noqa: E731
                                                    _lib.ptr(out, C.c_double))
    assert raw(1) == _lib.ERR_VALUE and raw(0) == _lib.OK and (out == 3.0).all()  # nothing written for n == 0
    assert raw(6) == _lib.OK and np.array_equal(out, squareform(scipy_cophenet(Z)))
    assert raw(6, np.ascontiguousarray(twice[:, :2], dtype=np.uint32).reshape(-1)) == _lib.ERR_VALUE


def test_argument_errors_need_no_context():
    ctx = _NoContext()
    Z = scipy_linkage(condensed(case_matrix(3, "random")), "average")
    d = case_matrix(3, "random")
    for bad in (np.zeros((3, 4)), np.zeros((2, 3)), np.zeros((0, 4)), np.zeros(8)):
        with pytest.raises(ValueError, match="shape"):
            cluster.cophenet(bad, d, ctx=ctx)
    for shape in ((3, 4), (9,), (2, 2, 2)):
        with pytest.raises(ValueError, match="square"):
            cluster.cophenet(Z, np.zeros(shape), ctx=ctx)
    with pytest.raises(ValueError, match="shape"):
        cluster.cophenet(Z, np.zeros((1, 1)), ctx=ctx)  # one leaf has no tree
    with pytest.raises(ValueError, match="0 leaves"):
        cluster.cophenet(Z, np.zeros((0, 0)), ctx=ctx)
    empty = cluster.cophenet(np.zeros((0, 4)), np.zeros((0, 0)), matrix=True, ctx=ctx)  # nothing to compute
    assert np.isnan(empty.correlation) and empty.row_sums.shape == (5, 0) and empty.cophenetic.shape == (0, 0)
    a = [np.zeros(30, np.uint8), np.ones(30, np.uint8), np.arange(30, dtype=np.uint8) % 4]
    with pytest.raises(ValueError, match="Unexpected distance 'manhattan'"):
        distance.cophenet(a, Z, "manhattan", k=3, ctx=ctx)
    with pytest.raises(ValueError, match="Expected sketch size"):
        distance.cophenet(a, Z, "mash", k=3, ctx=ctx)
    with pytest.raises(ValueError, match="Sketch size"):
        distance.cophenet(a, Z, "jsd", k=3, sketch_size=10, ctx=ctx)
    with pytest.raises(ValueError, match="shape"):
        distance.cophenet(a, Z[:1], "jsd", k=3, ctx=ctx)
    seqs = {"a": a[0], "b": a[1], "c": a[2]}
    for fn in (cluster.ctree_cophenet, cluster.compare_linkages):
        with pytest.raises(ValueError, match="Unexpected distance 'manhattan'"):
            fn(seqs, distance_mode="manhattan")
        with pytest.raises(ValueError, match="Expected sketch size"):
            fn(seqs, sketch_size=None)
        with pytest.raises(ValueError, match="at least two"):
            fn({"a": a[0]})
    with pytest.raises(ValueError, match="not built on the device"):
        cluster.ctree_cophenet(seqs, linkage="centroid")
    with pytest.raises(ValueError, match="Unexpected linkage method"):
        cluster.compare_linkages(seqs, ("average", "best"))
    with pytest.raises(ValueError, match="Unexpected distance 'manhattan'"):
        apps.dvs_cophenet(distance_mode="manhattan")
    with pytest.raises(ValueError, match="Expected sketch size for mash distance measure"):
        apps.dvs_cophenet(sketch_size=None)
    with pytest.raises(ValueError, match="Canonical kmers only supported for dna sequences"):
        apps.dvs_cophenet(moltype="protein", mash_canonical_kmers=True)
    with pytest.raises(ValueError, match="not built on the device"):
        apps.dvs_cophenet(("average", "median"))
    with pytest.raises(ValueError, match="one linkage method at least"):
        apps.dvs_cophenet(())


# ------------------------------------------------------------------ what the cases of the GPU test pin
@pytest.mark.parametrize("kind", KINDS)
def test_scipy_lies_within_the_bound_of_the_yardstick(kind):
    worst = 0.0
    for n in GPU_SIZES:
        for method in METHODS:
            D, Z, r = gpu_case(n, kind, method)
            with np.errstate(invalid="ignore", divide="ignore"):
                sp = float(scipy_cophenet(Z, condensed(D))[0])
            assert np.isnan(sp) == np.isnan(r), (n, kind, method)
            if not np.isnan(r):
                assert abs(sp - r) <= bound(n), (n, kind, method, abs(sp - r) / bound(n))
                worst = max(worst, abs(sp - r) / bound(n))
    print(f"{kind}: scipy's largest |r - truth| = {worst:.3g} x bound")


@pytest.mark.parametrize("kind", KINDS)
def test_shifted_float64_row_sums_lie_within_the_bound(kind):
    """a float64 model of the device's sums (numpy's order, not the kernel's) under the long-double combine"""
    worst = 0.0
    for n in GPU_SIZES:
        for method in METHODS:
            D, Z, r = gpu_case(n, kind, method)
            cb = c_bar_of(Z)
            off = ~np.eye(n, dtype=bool)
            x, y = np.where(off, D - cb, 0.0), np.where(off, squareform(scipy_cophenet(Z)) - cb, 0.0)
            sums = np.stack([t.sum(axis=1) for t in (x, y, x * x, y * y, x * y)])
            truth, mags = truth_row_sums(D, Z)
            assert (np.abs(sums.astype(np.longdouble) - truth) <= (n + 8) * 2.0 ** -52 * mags).all(), (n, kind, method)
            if not np.isnan(r):
                with np.errstate(invalid="ignore", divide="ignore"):
                    err = abs(correlation_from_row_sums(sums, n) - r)
                assert err <= bound(n), (n, kind, method, err / bound(n))
                worst = max(worst, err / bound(n))
    print(f"{kind}: the float64 model's largest |r - truth| = {worst:.3g} x bound")


def test_raw_moments_miss_the_bound_on_every_saturated_case():
    least = np.inf
    for n in GPU_SIZES:
        if n < 33:
            continue
        for method in METHODS:
            D, Z, r = gpu_case(n, "saturated", method)
            miss = abs(raw_moments_correlation(D, Z) - r) / bound(n)
            assert not miss <= 100, (n, method, miss)  # (a NaN from a negative variance is a miss as well)
            least = min(least, miss)
    print(f"saturated: float64 raw moments miss the truth by at least {least:.3g} x bound")


def test_degenerate_cases_are_nan_as_scipys():
    for n, D in ((2, case_matrix(2, "random")), (5, 0.75 * (1 - np.eye(5))), (65, 0.5 * (1 - np.eye(65)))):
        for method in METHODS:
            Z = scipy_linkage(condensed(D), method)
            assert np.isnan(truth_correlation(D, Z)), (n, method)
            with np.errstate(invalid="ignore", divide="ignore"):
                assert np.isnan(scipy_cophenet(Z, condensed(D))[0]), (n, method)


def test_c_bar_is_the_mean_cophenetic_distance():
    for n, kind, method in ((5, "tied", "average"), (65, "random", "ward"), (300, "saturated", "single")):
        _, Z, _ = gpu_case(n, kind, method)
        c = scipy_cophenet(Z).astype(np.longdouble)
        assert abs(c_bar_of(Z) - float(c.sum() / c.size)) <= 2.0 ** -52 * float(c.max())
