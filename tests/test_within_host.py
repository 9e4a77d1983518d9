"""Neighbours within a radius and threshold clusters, without a GPU: the public names and exports, the argument checks
that come before any device work, the two yardsticks tests/test_gpu_within.py holds the device to -- `expected_within`
(numpy's nonzero of d <= radius, row-major, as CSR) and `expected_components` (a union-find with first-appearance labels,
pinned here against scipy's connected_components and against the cut of scipy's single-linkage tree, ties at the radius
included) -- and the preconditions of the oracle's family cases: the radius of each lies in the widest gap of the
oracle's sorted cell values, farther from every cell than 1 000 x tol_derived(bins), and keeps between 1 % and 50 % of
the cells."""
import ctypes as C
import functools

import numpy as np
import pytest

from diverseseq_amd import _lib, apps, cluster, distance, engine
from test_clusters_host import first_appearance
from test_cross_host import FAMILY_CASES, GAP_FACTOR, _NoContext
from test_distance_truth_host import tol_derived
from test_gpu_linkage import family_seqs
from test_jsd_host import oracle_jsd_matrix

# the widest gap between consecutive sorted cell values of the oracle's matrix of either family case, two digits: the
# radius of the case is its middle
FAMILY_WIDEST_GAP = (4.4e-3, 1.3e-1)

NEW_EXPORTS = {"dvs_within", "dvs_pairs_destroy", "dvs_pairs_info", "dvs_pairs_get", "dvs_threshold_clusters"}


# ------------------------------------------------------------------ the yardsticks
def expected_within(d: np.ndarray, radius: float, skip_self: bool = False):
    """(row_start int64 [M + 1], index int64, distance float64) of the cells d <= radius in row-major order -- NaN
    compares false; skip_self: cell (i, i) is not looked at"""
    d = np.asarray(d, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        keep = d <= radius
    if skip_self:
        keep[np.arange(min(d.shape)), np.arange(min(d.shape))] = False
    rows, cols = np.nonzero(keep)
    row_start = np.zeros(d.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=d.shape[0]), out=row_start[1:])
    return row_start, cols.astype(np.int64), d[rows, cols]


def expected_components(d: np.ndarray, radius: float) -> np.ndarray:
    """the connected components of the graph that joins i < j when d[i, j] <= radius (the upper triangle alone; NaN
    joins nothing): int64 labels numbered by first appearance in position order"""
    n = d.shape[0]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    with np.errstate(invalid="ignore"):
        edges = np.argwhere(np.triu(np.asarray(d) <= radius, 1))
    for i, j in edges:
        a, b = find(int(i)), find(int(j))
        if a != b:
            parent[max(a, b)] = min(a, b)
    seen: dict = {}
    return np.array([seen.setdefault(find(i), len(seen)) for i in range(n)], dtype=np.int64)


def tie_matrix(n: int, seed: int) -> np.ndarray:
    """a symmetric matrix with a 0 diagonal whose other entries are the multiples 1/64 .. 64/64, every one an exact
    double: a threshold k / 64 meets many entries exactly.  P(entry <= k / 64) = (k / 64)^2, so that at n = 2 049 the
    threshold 1/64 keeps about half an edge a row (many small components) and 2/64 about two (a giant one and debris)"""
    rng = np.random.default_rng(seed)
    d = np.triu(np.maximum(np.ceil(64.0 * np.sqrt(rng.random((n, n)))), 1.0) / 64.0, 1)
    return d + d.T


@functools.lru_cache(maxsize=None)
def family_within_case(case: tuple):
    """-> (names, sequences, the oracle's jsd matrix, the radius in the middle of its widest gap, that gap)"""
    nfam, per, length, seed, k = case
    seqs = family_seqs(nfam, per, length, seed)
    names = list(seqs)
    d = oracle_jsd_matrix([seqs[n] for n in names], k)
    v = np.sort(d[np.triu_indices(len(names), 1)])
    gaps = np.diff(v)
    at = int(np.argmax(gaps))
    return names, [seqs[n] for n in names], d, float(0.5 * (v[at] + v[at + 1])), float(gaps[at])


# ------------------------------------------------------------------ names and exports
def test_public_names_and_exports():
    for name in ("Neighbours", "ThresholdClusters", "within", "neighbours", "matrix_within", "threshold_clusters",
                 "matrix_threshold_clusters", "check_radius"):
        assert hasattr(distance, name), name
    assert callable(distance.DeviceSide.within) and callable(distance.DeviceSide.threshold_clusters)
    assert callable(distance.Sketches.within) and callable(distance.Sketches.threshold_clusters)
    for name in ("within", "threshold_clusters", "dereplicate"):
        assert callable(getattr(cluster, name, None)), name
    assert callable(apps.dvs_dereplicate) and "dvs_dereplicate" in apps.__all__
    assert distance.Neighbours._fields == ("row_start", "index", "distance")
    assert distance.ThresholdClusters._fields == ("labels", "n_clusters", "sizes")
    nb = distance.Neighbours(np.array([0, 2, 2, 3]), np.array([4, 7, 1]), np.array([0.5, 0.25, 0.0]))
    assert nb.of(0)[0].tolist() == [4, 7] and nb.of(0)[1].tolist() == [0.5, 0.25]
    assert nb.of(1)[0].size == 0 and nb.of(2)[0].tolist() == [1]
    assert NEW_EXPORTS <= set(_lib.EXPORTS)
    lib = _lib.load()
    for name in NEW_EXPORTS:
        assert getattr(lib, name).argtypes is not None, name
    assert lib.dvs_abi_version() == 5
    assert _lib.WITHIN_SKIP_SELF == 1
    # no table of entries per mode any more: every operation, dense or sparse, is a method of DeviceSide over ONE entry,
    # which every mode reaches through the kind of its dvs_source
    for op in ("distances", "linkage", "nj", "cross_distances", "nearest", "cluster_scores", "cophenet", "maxmin", "within",
               "threshold_clusters"):
        assert callable(getattr(distance.DeviceSide, op)), op
        assert f"dvs_{op}" in _lib.EXPORTS and getattr(lib, f"dvs_{op}").argtypes[1] == C.POINTER(_lib.Source), op
    for op in ("within", "threshold_clusters"):
        assert not [name for name in _lib.EXPORTS if name.endswith("_" + op) and name != f"dvs_{op}"], op
    assert [_lib.SRC_MASH, _lib.SRC_EUCLIDEAN, _lib.SRC_JSD] == [distance.DeviceSide.MODE_NAMES.index(m)
                                                                 for m in ("mash", "euclidean", "jsd")]
    assert _lib.SRC_GIVEN == 3


# ------------------------------------------------------------------ argument errors come before any device work
BAD_RADII = (float("nan"), np.nan, None, "0.1", 1j, [0.1], True)


def test_argument_errors_need_no_context():
    a = [np.zeros(30, np.uint8), np.ones(30, np.uint8), np.arange(30, dtype=np.uint8) % 4]
    ctx = _NoContext()
    calls = (lambda r, mode, **kw: distance.within(a, a, r, mode, k=3, ctx=ctx, **kw),
             lambda r, mode, **kw: distance.neighbours(a, r, mode, k=3, ctx=ctx, **kw),
             lambda r, mode, **kw: distance.threshold_clusters(a, r, mode, k=3, ctx=ctx, **kw))
    for fn in calls:
        for bad in BAD_RADII:
            with pytest.raises(ValueError, match="radius"):
                fn(bad, "jsd")
        with pytest.raises(ValueError, match="Unexpected distance 'manhattan'"):
            fn(0.1, "manhattan")
        with pytest.raises(ValueError, match="Expected sketch size"):
            fn(0.1, "mash")
        for mode in ("jsd", "euclidean"):
            with pytest.raises(ValueError, match="Sketch size"):
                fn(0.1, mode, sketch_size=10)
            with pytest.raises(ValueError, match="Canonical kmers"):
                fn(0.1, mode, mash_canonical=True)
    for fn in calls[:2]:
        for bad in (0, -1, 1.5, "2", True):
            with pytest.raises(ValueError, match="max_pairs"):
                fn(0.1, "jsd", max_pairs=bad)
    # nothing to compute: no device work either
    for q, r, m in (([], a, 0), (a, [], 3)):
        nb = distance.within(q, r, 0.1, "jsd", k=3, ctx=ctx)
        assert nb.row_start.tolist() == [0] * (m + 1) and nb.index.size == nb.distance.size == 0
        assert nb.row_start.dtype == nb.index.dtype == np.int64 and nb.distance.dtype == np.float64
    assert distance.neighbours([], 0.1, "jsd", k=3, ctx=ctx).row_start.tolist() == [0]
    tc = distance.threshold_clusters([], 0.1, "jsd", k=3, ctx=ctx)
    assert tc.labels.size == 0 and tc.labels.dtype == np.int64 and tc.n_clusters == 0 and tc.sizes.size == 0


def test_handle_level_argument_errors():
    class _Matrix:  # (checked before the handle is touched)
        nrows, ctx = 5, _NoContext()

    m = _Matrix()
    for bad in BAD_RADII:
        with pytest.raises(ValueError, match="radius"):
            distance.matrix_within(m, m, bad)
        with pytest.raises(ValueError, match="radius"):
            distance.matrix_threshold_clusters(m, bad)
        with pytest.raises(ValueError, match="radius"):
            distance.DeviceSide(m, "jsd").within(distance.DeviceSide(m, "jsd"), bad)
        with pytest.raises(ValueError, match="radius"):
            distance.DeviceSide(m, "jsd").threshold_clusters(bad)
    with pytest.raises(ValueError, match="Unexpected distance 'mash'"):
        distance.matrix_within(m, m, 0.1, "mash")
    with pytest.raises(ValueError, match="Unexpected distance"):
        distance.matrix_threshold_clusters(m, 0.1, "manhattan")
    with pytest.raises(ValueError, match="max_pairs"):
        distance.matrix_within(m, m, 0.1, max_pairs=0)
    with pytest.raises(ValueError, match="against one of mode"):
        distance.DeviceSide(m, "jsd").within(distance.DeviceSide(m, "euclidean"), 0.1)
    for rows in ([5], [-1], [[0, 1]], [0.5]):
        with pytest.raises(ValueError, match="row list"):
            distance.matrix_within(m, m, 0.1, "jsd", q_rows=rows)
        with pytest.raises(ValueError, match="row list"):
            distance.matrix_within(m, m, 0.1, "jsd", r_rows=rows)
        with pytest.raises(ValueError, match="row list"):
            distance.matrix_threshold_clusters(m, 0.1, "euclidean", rows=rows)


def test_caller_matrix_argument_errors():
    ctx = _NoContext()
    d = np.zeros((4, 4))
    for bad in BAD_RADII:
        with pytest.raises(ValueError, match="radius"):
            cluster.within(d, bad, ctx=ctx)
        with pytest.raises(ValueError, match="radius"):
            cluster.threshold_clusters(d, bad, ctx=ctx)
    for fn in (cluster.within, cluster.threshold_clusters):
        with pytest.raises(ValueError, match="square"):
            fn(np.zeros((3, 4)), 0.1, ctx=ctx)
    with pytest.raises(ValueError, match="max_pairs"):
        cluster.within(d, 0.1, max_pairs=-3, ctx=ctx)
    assert cluster.within(np.zeros((0, 0)), 0.1, ctx=ctx).row_start.tolist() == [0]
    assert cluster.threshold_clusters(np.zeros((0, 0)), 0.1, ctx=ctx).n_clusters == 0
    seqs = {"a": np.zeros(30, np.uint8), "b": np.ones(30, np.uint8)}
    with pytest.raises(ValueError, match="radius"):
        cluster.dereplicate(seqs, float("nan"))
    with pytest.raises(ValueError, match="Unexpected distance"):
        cluster.dereplicate(seqs, 0.1, distance_mode="manhattan")
    with pytest.raises(ValueError, match="Expected sketch size"):
        cluster.dereplicate(seqs, 0.1, sketch_size=None)
    with pytest.raises(ValueError, match="no sequences"):
        cluster.dereplicate({}, 0.1)


def test_c_entries_refuse_their_arguments_before_any_device_work():
    """NULL arguments are refused without a context ever having been made (there is no device here to make one on), and
    *out is cleared; the dvs_pairs accessors take NULL.  The refusals that need a context -- a NaN radius, unknown flag
    bits, a row list or a size beyond the limits, host memory passed as device memory -- are in
    tests/test_gpu_within.py::test_c_entries_refuse_bad_arguments_and_leave_the_context_usable"""
    lib = _lib.load()
    out = C.c_void_p(0xDEAD)
    d = np.zeros((2, 2))
    lab, cnt = np.zeros(2, np.uint32), C.c_uint32()
    given = distance.make_source(_lib.SRC_GIVEN, d.ctypes.data, 2, keep=d)
    assert lib.dvs_within(None, given, None, 0.5, 0, 0, C.byref(out)) == _lib.ERR_VALUE
    assert not out.value  # *out is NULL after an error, whatever it held
    assert lib.dvs_threshold_clusters(None, given, 0.5, _lib.ptr(lab, C.c_uint32), C.byref(cnt)) == _lib.ERR_VALUE
    for kind, mash in ((_lib.SRC_JSD, {}), (_lib.SRC_EUCLIDEAN, {}), (_lib.SRC_MASH, {"k": 3, "sketch_size": 10})):
        null = distance.make_source(kind, None, 0, **mash)  # a NULL handle, as the typed entries were handed
        for q, r in ((null, null), (None, None)):
            out = C.c_void_p(0xDEAD)
            assert lib.dvs_within(None, q, r, 0.5, 0, 0, C.byref(out)) == _lib.ERR_VALUE
            assert not out.value
            assert lib.dvs_threshold_clusters(None, q, 0.5, None, None) == _lib.ERR_VALUE
    assert lib.dvs_pairs_info(None, None, None) == _lib.ERR_VALUE
    assert lib.dvs_pairs_get(None, None, None, None) == _lib.ERR_VALUE
    lib.dvs_pairs_destroy(None)


def test_dvs_dereplicate_constructor_checks():
    with pytest.raises(ValueError, match="Unexpected distance 'manhattan'"):
        apps.dvs_dereplicate(0.05, distance_mode="manhattan")
    with pytest.raises(ValueError, match="Expected sketch size for mash distance measure"):
        apps.dvs_dereplicate(0.05, distance_mode="mash", sketch_size=None)
    with pytest.raises(ValueError, match="Canonical kmers only supported for dna sequences"):
        apps.dvs_dereplicate(0.05, moltype="protein", mash_canonical_kmers=True)
    for bad in BAD_RADII:
        with pytest.raises(ValueError, match="radius"):
            apps.dvs_dereplicate(bad)
    a = apps.dvs_dereplicate(0.25, "jsd", k=5, sketch_size=77)
    assert (a._k, a._sketch_size, a._distance_mode, a._radius) == (5, None, "jsd", 0.25)


def test_no_public_method_was_added_to_the_engine_classes():
    for cls in (engine.Context, engine.Selection):
        assert not {"within", "neighbours", "threshold_clusters", "dereplicate"} & set(vars(cls))


# ------------------------------------------------------------------ the yardsticks themselves
def test_expected_within_is_row_major_inclusive_and_drops_nan():
    d = np.array([[0.0, 0.5, np.nan, 0.25], [0.5, -1.0, 0.5, np.inf], [np.nan] * 4])
    rs, idx, val = expected_within(d, 0.5)
    assert rs.tolist() == [0, 3, 6, 6] and idx.tolist() == [0, 1, 3, 0, 1, 2]
    assert val.tolist() == [0.0, 0.5, 0.25, 0.5, -1.0, 0.5]
    rs, idx, val = expected_within(d, 0.5, skip_self=True)
    assert rs.tolist() == [0, 2, 4, 4] and idx.tolist() == [1, 3, 0, 2]
    rs, idx, val = expected_within(d, np.nextafter(0.5, 0.0))
    assert rs.tolist() == [0, 2, 3, 3] and idx.tolist() == [0, 3, 1]
    rs, idx, val = expected_within(d, np.inf)
    assert rs.tolist() == [0, 3, 7, 7]  # every cell that is not NaN, +inf included
    assert expected_within(d, -np.inf)[0].tolist() == [0, 0, 0, 0]
    assert rs.dtype == idx.dtype == np.int64 and val.dtype == np.float64


def _tie_cases():
    """seeded symmetric matrices whose entries are multiples of 1/64, with thresholds that are entries: exact ties"""
    out = []
    for n, seed in ((2, 1), (33, 2), (200, 3), (257, 4)):
        d = tie_matrix(n, seed)
        # thresholds at which about 0.5, 1.5 and 3 edges a row pass, and the two ends
        v = np.sort(d[np.triu_indices(n, 1)])
        ts = {float(v[min(v.size - 1, int(f * n))]) for f in (0.25, 0.75, 1.5)} | {0.0, 1.0}
        out += [(d, t) for t in sorted(ts)]
    return out


def test_expected_components_against_scipy_two_ways():
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial.distance import squareform

    sizes = set()
    for d, t in _tie_cases():
        n = d.shape[0]
        assert (d[np.triu_indices(n, 1)] == t).any() or t in (0.0, 1.0)  # the threshold is an entry: a tie
        got = expected_components(d, t)
        graph = csr_matrix(np.triu(d <= t, 1))
        count, lab = connected_components(graph, directed=False)
        assert np.array_equal(got, first_appearance(lab)) and got.max() + 1 == count
        cut = fcluster(linkage(squareform(d, checks=False), "single"), t, "distance")
        assert np.array_equal(got, first_appearance(cut))
        sizes.add(int(got.max()) + 1)
    assert 1 in sizes and len(sizes) > 4  # one cluster, and several other partitions


def test_expected_components_labels_by_first_appearance_and_reads_the_upper_triangle():
    d = np.ones((6, 6))
    d[1, 4] = d[0, 5] = d[2, 3] = 0.25
    d[5, 1] = 0.0          # below the diagonal: not an edge
    d[3, 3] = np.nan       # the diagonal: not read
    d[0, 2] = np.nan       # NaN joins nothing
    lab = expected_components(d, 0.25)
    assert lab.tolist() == [0, 1, 2, 2, 1, 0]  # position 0 is in cluster 0, a new label at each first appearance
    assert np.array_equal(lab, first_appearance(lab))
    assert expected_components(d, 0.2).tolist() == list(range(6))
    assert expected_components(d, 1.0).tolist() == [0] * 6
    nan_row = np.full((4, 4), 0.5)
    nan_row[1, :] = nan_row[:, 1] = np.nan
    assert expected_components(nan_row, 0.5).tolist() == [0, 1, 0, 0]  # a row of NaN is a cluster of its own


# ------------------------------------------------------------------ the family cases of the GPU test
@pytest.mark.parametrize("case,pinned", zip(FAMILY_CASES, FAMILY_WIDEST_GAP), ids=["k4", "k6"])
def test_family_case_pair_set_does_not_depend_on_rounding(case, pinned):
    nfam, per, length, seed, k = case
    names, seqs, d, radius, gap = family_within_case(case)
    n = len(names)
    assert n == nfam * per and not np.isnan(d).any()
    off = d[~np.eye(n, dtype=bool)]
    margin = float(np.abs(off - radius).min())
    bound = tol_derived(4 ** k)
    kept = float((off <= radius).mean())
    print(f"k={k}: widest gap {gap:.3g}, radius {radius:.6g}, nearest cell {margin:.3g} = {margin / bound:.3g} x tol_derived, "
          f"{100 * kept:.1f} % of the cells kept")
    assert 0.9 * pinned <= gap <= 1.1 * pinned  # (the figure this case was chosen by)
    assert margin > GAP_FACTOR * bound
    assert 0.01 <= kept <= 0.50
    # what the radius keeps: exactly the pairs inside a family
    rs, idx, _ = expected_within(d, radius, skip_self=True)
    for i, name in enumerate(names):
        fam = name.split("_m")[0]
        mine = [names[j] for j in idx[rs[i]:rs[i + 1]]]
        assert mine == [m for m in names if m != name and m.split("_m")[0] == fam], name
    lab = expected_components(d, radius)
    assert lab.max() + 1 == nfam and all(lab[i] == i // per for i in range(n))
