"""Distances between two collections and the nearest references, without a GPU: the public names, the argument
checks that come before any device work, and the cases of tests/test_gpu_cross.py with their preconditions pinned on
the CPU -- in particular that the order the GPU test expects of a query's nearest references does not depend on
rounding: with the oracle's two-member total_jsd (test_jsd_host.pair_jsd) every gap between consecutive distinct
distances among a query's 5 nearest references exceeds 1 000 x tol_derived(bins)."""
import numpy as np
import pytest

import oracle
from conftest import synth_seqs
from diverseseq_amd import _lib, apps, distance, engine
from test_cluster import EXPECT
from test_distance_truth_host import tol_derived
from test_gpu_linkage import family_seqs
from test_jsd_host import pair_jsd

GAP_FACTOR = 1000  # a gap counts as safe from rounding at this many times the bound of a cell
TOP = 5            # ... among this many nearest references of every query

# (nfam, per, length, seed, k): references = members 0 - 5 of each family, queries = members 6 - 11
FAMILY_CASES = ((12, 12, 3000, 5, 4), (8, 12, 5000, 6, 6))
FAMILY_MIN_GAP = (3.5e-5, 4.1e-6)  # the smallest such gap of either case, two digits

# Selection.assign: nmost over synthetic sequences (nseq, length, seed, k, n)
ASSIGN_CASE = (300, 600, 41, 3, 10)

# apps.dvs_nearest on BRCA1: the references are the four species of a reference topology, the queries the rest
BRCA1_REFS = next(iter(EXPECT))
BRCA1_JSD_K = 5


def family_split(nfam, per, length, seed):
    """-> (reference names, reference sequences, query names, query sequences)"""
    seqs = family_seqs(nfam, per, length, seed)
    refs = [n for n in seqs if int(n.split("_m")[1]) < 6]
    queries = [n for n in seqs if int(n.split("_m")[1]) >= 6]
    return refs, [seqs[n] for n in refs], queries, [seqs[n] for n in queries]


def assign_case(with_order: bool):
    """-> (sequences, the stream order or None, the oracle's members as stream positions, their matrix rows)"""
    nseq, length, seed, k, n = ASSIGN_CASE
    seqs = synth_seqs(nseq, length, seed)
    order = np.random.default_rng(3).permutation(nseq).astype(np.uint32) if with_order else None
    stream = seqs if order is None else [seqs[i] for i in order]
    members = oracle.nmost(stream, n, k, 4).members()[0]
    return seqs, order, members, members if order is None else order[members]


def oracle_cross_jsd(queries, refs, k: int, num_states: int = 4) -> np.ndarray:
    """cell (i, j): pair_jsd of query i and reference j; NaN where either has no valid k-mer"""
    def side(seqs):
        return [oracle.to_kfreqs(s, num_states, k) if oracle.count_kmers(s, num_states, k).sum() > 0 else None for s in seqs]

    q, r = side(queries), side(refs)
    d = np.full((len(q), len(r)), np.nan)
    for i, a in enumerate(q):
        for j, b in enumerate(r):
            if a is not None and b is not None:
                d[i, j] = pair_jsd(*a, *b)
    return d


def expected_nearest(d: np.ndarray, kk: int):
    """the kk nearest columns of every row of d by a stable sort (a tie to the lower column), NaN cells dropped:
    (int64 [M, kk], -1 in an empty slot; float64 [M, kk], NaN there)"""
    m = d.shape[0]
    idx = np.full((m, kk), -1, dtype=np.int64)
    val = np.full((m, kk), np.nan)
    for i in range(m):
        order = np.argsort(d[i], kind="stable")
        order = order[~np.isnan(d[i][order])][:kk]
        idx[i, : order.size] = order
        val[i, : order.size] = d[i][order]
    return idx, val


def smallest_gap(d: np.ndarray, top: int = TOP) -> float:
    """the smallest gap between consecutive DISTINCT distances among the `top` nearest columns of any row"""
    worst = np.inf
    for row in d:
        v = np.sort(row[~np.isnan(row)])[:top]
        g = np.diff(v)
        g = g[g > 0]
        if g.size:
            worst = min(worst, float(g.min()))
    return worst


# ------------------------------------------------------------------ the names
def test_public_names_exist():
    for name in ("cross_distances", "nearest", "matrix_cross_distances", "matrix_nearest", "CROSS_MODES"):
        assert hasattr(distance, name), name
    assert callable(distance.Sketches.cross_distances) and callable(distance.Sketches.nearest)
    assert callable(engine.Selection.assign)
    assert callable(apps.dvs_nearest) and "dvs_nearest" in apps.__all__
    assert set(distance.CROSS_MODES) == set(distance.MODES) == {"mash", "euclidean", "jsd"}
    assert len(distance.MODES["mash"]) == 2  # (left as it is: tests and apps index its pairs)
    new = {"dvs_cross_distances", "dvs_nearest"}  # one entry per operation: the mode travels in the dvs_source
    assert new <= set(_lib.EXPORTS)
    lib = _lib.load()
    for name in new:
        assert getattr(lib, name).argtypes is not None, name
    assert lib.dvs_abi_version() == 5


# ------------------------------------------------------------------ argument errors come before any device work
class _NoContext:
    """stands in for a context: any use is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the context was used ({name}) before the arguments were checked")


def test_argument_errors_need_no_context():
    a = [np.zeros(30, np.uint8), np.ones(30, np.uint8), np.arange(30, dtype=np.uint8) % 4]
    ctx = _NoContext()
    for fn, extra in ((distance.cross_distances, ()), (distance.nearest, (1,))):
        with pytest.raises(ValueError, match="Unexpected distance 'manhattan'"):
            fn(a, a, *extra, "manhattan", k=3, ctx=ctx)
        with pytest.raises(ValueError, match="Expected sketch size"):
            fn(a, a, *extra, "mash", k=3, ctx=ctx)
        for mode in ("jsd", "euclidean"):
            with pytest.raises(ValueError, match="Sketch size"):
                fn(a, a, *extra, mode, k=3, sketch_size=10, ctx=ctx)
            with pytest.raises(ValueError, match="Canonical kmers"):
                fn(a, a, *extra, mode, k=3, mash_canonical=True, ctx=ctx)
    for mode, kw in (("jsd", {}), ("euclidean", {}), ("mash", dict(sketch_size=20))):
        for bad in (0, -1, 4, 1.5, "2", True, None):
            with pytest.raises(ValueError, match="n_nearest"):
                distance.nearest(a, a, bad, mode, k=3, ctx=ctx, **kw)
        with pytest.raises(ValueError, match="n_nearest"):
            distance.nearest(a, [], 1, mode, k=3, ctx=ctx, **kw)
        with pytest.raises(NotImplementedError, match="64 at most"):
            distance.nearest(a, a * 30, 65, mode, k=3, ctx=ctx, **kw)
    # nothing to compute: no device work either
    assert distance.cross_distances([], a, "jsd", k=3, ctx=ctx).shape == (0, 3)
    assert distance.cross_distances(a, [], "jsd", k=3, ctx=ctx).shape == (3, 0)
    idx, d = distance.nearest([], a, 2, "jsd", k=3, ctx=ctx)
    assert idx.shape == d.shape == (0, 2) and idx.dtype == np.int64 and d.dtype == np.float64


def test_handle_level_argument_errors():
    class _Matrix:  # (checked before the handle is touched)
        nrows, ctx = 5, _NoContext()

    m = _Matrix()
    with pytest.raises(ValueError, match="Unexpected distance 'mash'"):
        distance.matrix_cross_distances(m, m, "mash")
    with pytest.raises(ValueError, match="Unexpected distance"):
        distance.matrix_nearest(m, m, 1, "manhattan")
    for rows in ([5], [-1], [[0, 1]], [0.5]):
        with pytest.raises(ValueError, match="row list"):
            distance.matrix_cross_distances(m, m, "jsd", q_rows=rows)
        with pytest.raises(ValueError, match="row list"):
            distance.matrix_nearest(m, m, 1, "jsd", r_rows=rows)
    with pytest.raises(ValueError, match="n_nearest"):
        distance.matrix_nearest(m, m, 3, "jsd", r_rows=[0, 1])  # (two references listed)
    with pytest.raises(NotImplementedError):
        distance.matrix_nearest(m, m, 65, "jsd", r_rows=[0] * 70)


def test_dvs_nearest_constructor_checks():
    refs = {"a": "ACGTACGTAC", "b": "AACCGGTTAA"}
    with pytest.raises(ValueError, match="Unexpected distance 'manhattan'"):
        apps.dvs_nearest(refs, distance_mode="manhattan")
    with pytest.raises(ValueError, match="Expected sketch size for mash distance measure"):
        apps.dvs_nearest(refs, distance_mode="mash", sketch_size=None)
    with pytest.raises(ValueError, match="Canonical kmers only supported for dna sequences"):
        apps.dvs_nearest(refs, moltype="protein", mash_canonical_kmers=True)
    for bad in (0, 3, 65):
        with pytest.raises((ValueError, NotImplementedError), match="n_nearest"):
            apps.dvs_nearest(refs, n_nearest=bad)


def test_expected_nearest_is_the_stable_order():
    d = np.array([[0.5, np.nan, 0.25, 0.25, 0.0], [np.nan] * 5, [1.0, 0.0, -0.0, np.nan, 1.0]])
    idx, val = expected_nearest(d, 4)
    assert idx.tolist() == [[4, 2, 3, 0], [-1] * 4, [1, 2, 0, 4]]
    assert np.array_equal(val[0], [0.0, 0.25, 0.25, 0.5]) and np.isnan(val[1]).all()
    idx, val = expected_nearest(d, 5)
    assert idx[0].tolist() == [4, 2, 3, 0, -1] and np.isnan(val[0, 4])


# ------------------------------------------------------------------ the family case of the GPU test
@pytest.mark.parametrize("case,pinned", zip(FAMILY_CASES, FAMILY_MIN_GAP), ids=["k4", "k6"])
def test_family_case_order_does_not_depend_on_rounding(case, pinned):
    nfam, per, length, seed, k = case
    ref_names, refs, query_names, queries = family_split(nfam, per, length, seed)
    assert len(refs) == len(queries) == 6 * nfam
    d = oracle_cross_jsd(queries, refs, k)
    assert not np.isnan(d).any()
    gap = smallest_gap(d)
    bound = tol_derived(4 ** k)
    print(f"k={k}: smallest gap among the {TOP} nearest = {gap:.3g} = {gap / bound:.3g} x tol_derived")
    assert gap > GAP_FACTOR * bound
    assert 0.9 * pinned <= gap <= 1.1 * pinned  # (the figure this case was chosen by)
    idx, val = expected_nearest(d, 3)
    for i, name in enumerate(query_names):
        fam = name.split("_m")[0]
        assert all(ref_names[j].split("_m")[0] == fam for j in idx[i]), (name, [ref_names[j] for j in idx[i]])
        zeros = [ref_names[j] for j in np.flatnonzero(d[i] == 0.0)]
        # member 10 is an exact copy of its family's root, as reference 3 is: distance 0 from that one reference only
        assert zeros == ([f"{fam}_m3"] if name.endswith("_m10") else []), (name, zeros)


# ------------------------------------------------------------------ the Selection.assign case
@pytest.mark.parametrize("with_order", [False, True])
def test_assign_case_order_does_not_depend_on_rounding(with_order):
    k, n = ASSIGN_CASE[3:]
    seqs, _, _, members = assign_case(with_order)
    assert len(set(members.tolist())) == n
    d = oracle_cross_jsd(seqs, [seqs[i] for i in members], k)
    assert not np.isnan(d).any()
    gap = smallest_gap(d)
    print(f"assign: smallest gap among the {TOP} nearest members = {gap:.3g} = {gap / tol_derived(4 ** k):.3g} x tol_derived")
    assert gap > GAP_FACTOR * tol_derived(4 ** k)
    idx, val = expected_nearest(d, 1)
    for pos, row in enumerate(members):  # a member is nearest to itself, at exactly 0, and to nothing else at 0
        assert idx[row, 0] == pos and val[row, 0] == 0.0 and (d[row] == 0.0).sum() == 1


# ------------------------------------------------------------------ the BRCA1 case of apps.dvs_nearest
def test_brca1_jsd_case_order_does_not_depend_on_rounding(brca1):
    assert len(BRCA1_REFS) == 4 and set(BRCA1_REFS) <= set(brca1)
    queries = [n for n in brca1 if n not in BRCA1_REFS]
    assert len(queries) == 51
    d = oracle_cross_jsd([brca1[n] for n in queries], [brca1[n] for n in BRCA1_REFS], BRCA1_JSD_K)
    assert not np.isnan(d).any() and (d > 0).all()
    gap = smallest_gap(d)
    bound = tol_derived(4 ** BRCA1_JSD_K)
    print(f"brca1 jsd k={BRCA1_JSD_K}: smallest gap = {gap:.3g} = {gap / bound:.3g} x tol_derived")
    assert gap > GAP_FACTOR * bound


def test_brca1_mash_ties_are_equal_quotients(brca1):
    """mash distances are a function of (intersection, union), two integers: equal counts give equal bits on both
    sides, so the stable order of the oracle's matrix is the order the device must return"""
    k, s = 12, 400
    sk = {n: oracle.mash_sketch(brca1[n], k, s, 4, False) for n in brca1}
    queries = [n for n in brca1 if n not in BRCA1_REFS]
    d = np.array([[oracle.mash_distance(sk[q], sk[r], k, s) for r in BRCA1_REFS] for q in queries])
    assert not np.isnan(d).any()
    # distinct values of this case differ by far more than the rtol of 1e-13 the distances are compared to
    v = np.unique(d)
    assert (np.diff(v) > 1e-9 * v[1:]).all()
