"""The distance matrices of csrc/rowdist.hip (jsd_pairs_kernel / jsd_finish_kernel, euclid_kernel) against the
long-double yardstick of tests/test_distance_truth_host.py, which pins that yardstick, the cases and the oracle's own
error on the CPU.

For every case, in both count widths where the build has a choice:
  * the exact properties of the matrix -- dtype, shape, symmetry bit for bit, a zero diagonal, NaN in exactly the rows
    and columns of rows without a valid k-mer, JSD cells in [0, 1], exactly 0.0 between rows whose f64 quotients are
    equal (copies in other tiles, counts in proportion), > 0 where the truth exceeds the bound, the same bits from a
    second call and from the fused tree entries;
  * JSD gate 1, derived: every cell within tol_derived(B) of the truth;
  * JSD gate 2, measured against the reference: the worst device error of a case at most
    max(4 E_oracle[case], 8 2^-52 max(1, log2 B)) -- 4 is the room two correct f64 evaluations of one sum (fma chain
    against mul + add, another log2) have against each other, the floor is a few ulps of an entropy for the cases where
    the oracle's roundings happen to cancel;
  * euclidean cells within 1e-12 relative of the truth (atol = 0);
  * on family320, the sorted single-linkage heights within tol_derived(B) of scipy's over the truth matrix: they are
    the weights of the minimum spanning tree, 1-Lipschitz in the sup norm of the matrix."""
import numpy as np
import pytest

from diverseseq_amd import cluster, distance, engine
from test_distance_truth_host import (EUCLID_RTOL, case_rows, case_truth, distance_cases, f64_quotients, gate2_floor,
                                      oracle_errors, tol_derived)
from test_linkage_methods_host import scipy_z

pytestmark = pytest.mark.gpu

_CASES = distance_cases()
_BY_NAME = {c.name: c for c in _CASES}


def _has_width_choice(case):
    """16-bit count rows: at most 4096 bins, a multiple of four, every sequence at most 32768 windows
    (csrc/kmer_hist.hip dvs_hist_rows_fit_u16); DVS_COUNTS_U32 then asks for 32-bit rows all the same"""
    return (case.seqs is not None and case.nbins <= 4096 and case.nbins % 4 == 0
            and max(s.size for s in case.seqs) - case.k + 1 <= 32768)


_RUNS = [(c, w) for c in _CASES for w in ((2, 4) if _has_width_choice(c) else (0 if c.seqs is None else 4,))]


def _run_id(run):
    case, width = run
    return case.name + {2: "-u16", 4: "-u32"}[width] if _has_width_choice(case) else case.name


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context()


_results = {}


def matrices(ctx, monkeypatch, case, width):
    """(JSD matrix, JSD matrix of a second call over a matrix handle, euclidean matrix) of a case, once per module"""
    key = (case.name, width)
    if key not in _results:
        if width == 4 and _has_width_choice(case):
            monkeypatch.setenv("DVS_COUNTS_U32", "1")
        if case.seqs is None:
            m = ctx.matrix_from_freqs(case.freqs)
            first = None
        else:
            first = distance.jsd_distances(case.seqs, case.k, case.num_states, ctx=ctx)
            m = ctx.build_matrix(case.seqs, case.k, case.num_states)
        try:
            assert m.count_bytes == width, (case.name, m.count_bytes, width)
            again = distance.matrix_jsd_distances(m)
            first = distance.matrix_jsd_distances(m) if first is None else first
            euclid = distance.matrix_euclidean_distances(m) if case.seqs is None else \
                distance.euclidean_distances(case.seqs, case.k, case.num_states, ctx=ctx)
        finally:
            m.close()
        _results[key] = (first, again, euclid)
    return _results[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _cells(d, pairs):
    return d[pairs[:, 0], pairs[:, 1]]


_equal = {}


def _equal_rows(case, pairs):
    """which pairs are rows of bit-equal f64 quotients RN(c / t): equal counts, or counts in proportion"""
    if case.name not in _equal:
        q = f64_quotients(case_rows(case))
        _equal[case.name] = np.array([bool((q[i] == q[j]).all()) for i, j in pairs])
    return _equal[case.name]


def assert_exact_properties(d, case, *, jsd):
    n = case.nrows
    assert d.shape == (n, n) and d.dtype == np.float64
    assert (_bits(d) == _bits(d.T)).all()
    assert (_bits(np.diag(d)) == 0).all()  # (+0.0)
    off = ~np.eye(n, dtype=bool)
    nan = np.zeros((n, n), dtype=bool)
    for e in case.empty:
        nan[e, :] = nan[:, e] = True
    np.testing.assert_array_equal(np.isnan(d), nan & off)
    ok = off & ~nan
    assert (d[ok] >= 0.0).all()
    if jsd:
        assert (d[ok] <= 1.0).all()


# --------------------------------------------------------------------------------------------- every case
@pytest.mark.parametrize("run", _RUNS, ids=_run_id)
def test_jsd_exact_properties(ctx, monkeypatch, run):
    case, width = run
    d, again, _ = matrices(ctx, monkeypatch, case, width)
    assert_exact_properties(d, case, jsd=True)
    assert (_bits(d) == _bits(again)).all()  # (a second call, over a matrix handle)
    pairs, truth, _ = case_truth(case)
    got = _cells(d, pairs)
    same = _equal_rows(case, pairs)
    assert (_bits(got[same]) == 0).all(), f"{case.name}: rows of equal quotients, cell not 0.0"
    assert (truth[same] == 0).all()
    assert (got[truth > tol_derived(case.nbins)] > 0).all()
    print(f"{case.name}: {len(pairs)} cells, {int(same.sum())} between rows of equal quotients")


@pytest.mark.parametrize("run", _RUNS, ids=_run_id)
def test_jsd_cells_against_the_truth(ctx, monkeypatch, run):
    """Gate 1 and gate 2 of the module docstring.

    Measured on an MI355X (this test prints the figures): see DESIGN.md 4.8 "Accuracy"."""
    case, width = run
    d = matrices(ctx, monkeypatch, case, width)[0]
    pairs, truth, _ = case_truth(case)
    err = np.abs(_cells(d, pairs).astype(np.longdouble) - truth)
    worst = float(err.max())
    at = pairs[int(np.argmax(err))]
    e_oracle = oracle_errors(case)[0]
    tol, gate2 = tol_derived(case.nbins), max(4 * e_oracle, gate2_floor(case.nbins))
    ratio = worst / e_oracle if e_oracle else (0.0 if worst == 0 else float("inf"))
    print(f"{_run_id(run)}: B = {case.nbins}, {len(pairs)} cells, worst |D - truth| = {worst:.3g} at {tuple(int(x) for x in at)} "
          f"(truth {float(truth[int(np.argmax(err))]):.3g}), device / tol_derived = {worst / tol:.3g}, "
          f"E_oracle = {e_oracle:.3g}, device / oracle = {ratio:.3g}, gate 2 = {gate2:.3g}")
    assert worst <= tol, "gate 1"
    assert worst <= gate2, "gate 2"


@pytest.mark.parametrize("run", _RUNS, ids=_run_id)
def test_euclidean_cells_against_the_truth(ctx, monkeypatch, run):
    case, width = run
    d = matrices(ctx, monkeypatch, case, width)[2]
    assert_exact_properties(d, case, jsd=False)
    pairs, _, truth = case_truth(case)
    got = _cells(d, pairs)
    same = _equal_rows(case, pairs)
    assert (_bits(got[same]) == 0).all() and (truth[same] == 0).all()
    assert (got[~same] > 0).all()
    rel = np.abs(got[~same].astype(np.longdouble) - truth[~same]) / truth[~same]
    worst = float(rel.max()) if rel.size else 0.0
    print(f"{_run_id(run)}: B = {case.nbins}, {len(pairs)} cells, worst relative |D - truth| = {worst:.3g}")
    assert worst <= EUCLID_RTOL


# --------------------------------------------------------------------------------------------- the fused entries
def _tree_case(name):
    """(sequences with a valid k-mer, their indices in the case) of a case"""
    case = _BY_NAME[name]
    keep = [i for i in range(case.nrows) if i not in case.empty]
    return case, [case.seqs[i] for i in keep], np.array(keep)


@pytest.mark.parametrize("method", ["single", "average"])
@pytest.mark.parametrize("name", ["family320", "tiles"])
def test_fused_tree_entries_see_the_same_matrix(ctx, monkeypatch, name, method):
    """jsd_linkage / euclidean_linkage, which leave the matrix in HBM, against cluster.linkage over the matrix that came
    to the host; for `tiles`, the rows without a valid k-mer removed (which moves every later row to another place of
    its tile: a pair's cell is summed by one thread in bin order and keeps its bits)"""
    case, seqs, keep = _tree_case(name)
    full = matrices(ctx, monkeypatch, case, 2)
    for which, fused in ((0, distance.jsd_linkage), (2, distance.euclidean_linkage)):
        d = full[which][np.ix_(keep, keep)]
        if len(keep) < case.nrows:
            dist = distance.jsd_distances if which == 0 else distance.euclidean_distances
            assert (_bits(dist(seqs, case.k, ctx=ctx)) == _bits(d)).all()
        z = fused(seqs, case.k, method=method, ctx=ctx)
        assert np.array_equal(z, cluster.linkage(d, method, ctx=ctx))
        assert np.array_equal(z, scipy_z(d, method))


def test_single_linkage_heights_follow_the_truth(ctx):
    case = _BY_NAME["family320"]
    pairs, truth, _ = case_truth(case)
    t = np.zeros((case.nrows, case.nrows))
    t[pairs[:, 0], pairs[:, 1]] = t[pairs[:, 1], pairs[:, 0]] = truth.astype(np.float64)
    exp = np.sort(scipy_z(t, "single")[:, 2])
    got = np.sort(distance.jsd_linkage(case.seqs, case.k, method="single", ctx=ctx)[:, 2])
    worst = float(np.abs(got - exp).max())
    print(f"family320: single-linkage heights, worst |device - scipy over the truth| = {worst:.3g} "
          f"(bound {tol_derived(case.nbins):.3g}); {int((exp == 0).sum())} merges at height 0")
    assert (got[exp == 0] == 0).all()
    assert worst <= tol_derived(case.nbins)
