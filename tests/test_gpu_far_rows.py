"""Every count-matrix operation on rows behind the 2^32nd (and the 2^31st) element of the matrix.

Every kernel that touches a count row computes `mat + row * B`; csrc/persist.hip, select.hip, rowdist.hip, crossdist.hip,
canon.hip, maxmin.hip, kmer_hist.hip, api.cpp and exact_set.cpp hold more than sixty such products.  A product that lost
its 64-bit cast would wrap: row r* + j would read row j, and no other test puts a row that far.  The layouts of
tests/test_far_rows_host.py do, in three shapes (16-bit rows of 4096 bins, the persistent engine; 32-bit rows of 16 384
bins, the persistent engine for nmost; 32-bit rows of 262 144 bins, the multi-launch engine and the global-memory
histogram build): about 120 real rows, nearly all of them behind r* = 2^32 / B, and rows without a valid k-mer
everywhere else.  A product that wraps at 2^32 reads a front row or an empty row in place of a far one; one that goes
negative at 2^31 reads outside the matrix.

One module-scoped matrix per layout (8.6, 17.2 and 17.5 GB), built one at a time and closed, the context's block cache
trimmed, before the next is built; the teardown checks that free device memory is back where it was.  A layout is
skipped when less than 1.6 x its bytes (the matrix and its folded copy) + 2 GB of device memory is free.

Every comparison is against something other than the code under test -- the oracle, the long-double truth of
tests/test_distance_truth_host.py, numpy -- at the tolerance the suite already holds the same quantity to.  And every
output that is a function of the rows' contents alone must have the bits the TWIN gives: the same real sequences, in
the same order, as a matrix of 123 rows.  Address arithmetic is all that differs.

What a selection without an order can reach.  The reference seeds a set with the first n records of the stream and
drops those without a valid k-mer (src/records.rs:299-306), so nmost(40) over a whole layout keeps a set of the 8 front
rows, and rows behind r* enter it by accepts only; it is the one form of nmost the persistent engine takes.  The seeds
of the layouts are chosen so that it does accept such rows and ends holding some (tests/test_far_rows_host.py,
MIN_WHOLE_FAR): 5 accepts of rows >= r* and 3 members there at 4^6 bins, 2 and 2 at 4^7, 4 and 3 at 4^9 -- the engine
replaces its lowest member by a far row, fetches far rows as members and scans the rest of the stream against them.
The set of 40 members, 27 of them seeded behind r*, is the selection with an explicit order of the real rows'
positions (multi-launch engine); max_divergent(4, 30) grows from rows 0 .. 3 by far rows on either engine.  Every far
row's score as such is held to the oracle in the read-back tests (score_kernel).

What was tried against it, on scratch copies.  The persistent scan's candidate read `mat + p * B` formed in 32 bits
fails test_nmost at 4^6 and 4^7 bins and test_max_divergent at 4^6.  The persistent engine's member-row reads
`mat + s_pos[..] * B` formed in 32 bits do not change its answer: its own checks hand the decision to the host arbiter,
which replays it right; at 4^7 bins that shows as n_arbitrated == 1, which _run_selection refuses, at 4^6 bins (16-bit
rows) it showed nowhere -- the member-row reads of that instantiation are not covered by this module's outputs.
crossdist.hip's query-row read formed in 32 bits fails all six jsd tests of the row lists.

Measured on an MI355X: the module takes about 32 s, 11 s of them in the first layout's set-up, which also creates the
process's first context (the other two layouts are set up in about 1 s each); the slowest test takes 3.1 s (the jsd
cells at 4^9 bins with their 45 x 107 long-double truth); least free device memory 26.6 GB below the start (the 17.5 GB
matrix of 4^9 bins and its folded copy).

Out of reach, and not covered here:
  * the square distance entry, the trees, NJ and max-min take rows 0 .. n - 1 only: pointing them at far rows needs an
    n x n matrix of 10^12 cells;
  * frequency (f64) matrices of 2^32 elements need a 34 GB host array;
  * sketch sets of 2^32 hashes;
  * a caller's n x n matrix with n >= 65 536: 34 GB, and a chain of 65 000 dependent steps."""
import types

import numpy as np
import pytest
from scipy.cluster.hierarchy import linkage as scipy_linkage

import oracle
from test_canonical_host import ENTROPY_TOL, canonical_count, folded_of_counts
from test_cophenet_host import condensed
from test_distance_truth_host import EUCLID_RTOL, tol_derived
from test_far_rows_host import (LAYOUTS, MAX_ARGS, MIN_WHOLE_FAR, N_FRONT, N_Q, N_SELECT, TIE_N, oracle_max, oracle_nmost, oracle_nmost_by_order,
                                oracle_nmost_whole,
                                real_counts, real_entropies, real_positions, real_seqs, row_lists, row_seq, square_of, stream,
                                tie_case, truth_cells, window_counts, windows)
from test_gpu_clusters import assert_same_scores as assert_same_cluster_scores
from test_gpu_clusters import assert_scores as assert_cluster_scores
from test_gpu_cophenet import assert_same_scores as assert_same_cophenet_scores
from test_gpu_cophenet import assert_scores as assert_cophenet_scores
from test_gpu_cross import assert_nearest, same_bits
from test_gpu_parity import RTOL, TIGHT, _assert_selection
from test_gpu_within import assert_labels, assert_within, same_neighbours
from test_readback_host import assert_scores

pytestmark = pytest.mark.gpu

MODES = ("jsd", "euclidean")
RESIDENT_MARGIN = 1 << 30  # bytes a neighbour on the card may take in between: an eighth of the smallest layout
_lowest_free = [None]      # the least free device memory seen while a layout was resident (printed)


@pytest.fixture(scope="module")
def ctx():
    from diverseseq_amd import engine

    return engine.default_context()


def _free(ctx) -> int:
    import torch

    ctx.sync()
    torch.cuda.synchronize()
    return int(torch.cuda.mem_get_info(0)[0])


def _note_free(ctx, what):
    free = _free(ctx)
    _lowest_free[0] = free if _lowest_free[0] is None else min(free, _lowest_free[0])
    print(f"{what}: {free} bytes of device memory free (the least so far in this module: {_lowest_free[0]})")


def _trimmed_free(ctx) -> int:
    ctx.sync()
    ctx.check(ctx._L.dvs_ctx_trim(ctx._h))
    return _free(ctx)


def _guard(ctx, layout) -> int:
    """free device memory with the block cache released; skips the layout unless 1.6 x its bytes + 2 GB are free"""
    free = _trimmed_free(ctx)
    need = int(1.6 * layout.nbytes) + 2 * 10 ** 9
    if free < need:
        pytest.skip(f"{layout.name}: {free} bytes of device memory free, {need} needed (1.6 x the {layout.nbytes} bytes of "
                    "the matrix, for it and its folded copy, + 2 GB)")
    return free


def _assert_released(ctx, layout, free_before):
    free_after = _trimmed_free(ctx)
    print(f"{layout.name}: {free_before} bytes free before the build, {free_after} with everything closed and the cache "
          "released")
    assert free_before - free_after <= RESIDENT_MARGIN, (layout.name, free_before, free_after)


def _build(ctx, route, data, offsets, k):
    """(matrix, what has to stay alive beside it) by one of the three build routes"""
    if route == "concat":
        return ctx.build_matrix_concat(data, offsets, k, 4), None
    if route == "device":
        import torch

        t = torch.from_numpy(np.array(data)).to("cuda:0")
        torch.cuda.synchronize()
        return ctx.build_matrix_device(t.data_ptr(), offsets, k, 4), t
    packed = ctx.pack_host(np.array(data[: int(offsets[-1])]))
    return ctx.build_matrix_packed(packed, offsets, k), packed


def _twin_stream(layout):
    data, offsets = oracle.concat(list(real_seqs(layout)))
    return np.concatenate([data, np.zeros(16, np.uint8)]), offsets


_resident = []  # the layout that is resident now: (release,), at most one


def _release_resident():
    """close the resident layout, release the block cache and check that free device memory is back where it was"""
    while _resident:
        _resident.pop()()


@pytest.fixture(scope="module", params=LAYOUTS, ids=[x.name for x in LAYOUTS])
def far(request, ctx):
    """one layout's matrix and its twin.  pytest runs the tests of one layout together and tears the fixture down before
    the next layout's first test; the last layout is released by the first test behind it (the build routes) or here"""
    layout = request.param
    _release_resident()
    free_before = _guard(ctx, layout)
    m, _ = _build(ctx, "concat", *stream(layout), layout.k)
    twin, _ = _build(ctx, "concat", *_twin_stream(layout), layout.k)
    cache = {}

    def release():
        twin.close()
        m.close()
        _assert_released(ctx, layout, free_before)

    _resident.append(release)
    try:
        _note_free(ctx, f"{layout.name} built")
        yield types.SimpleNamespace(layout=layout, m=m, twin=twin, pos=real_positions(layout), ctx=ctx, cache=cache)
    finally:
        _release_resident()


# ---------------------------------------------------------------- 1. build and read-back
def _assert_read_back(layout, m, twin, what):
    """count windows around h*, around r* and at the end against oracle.count_kmers (the empty neighbours all zero),
    the whole totals vector, the entropies against oracle.to_kfreqs within 1e-11 max(1, |h|) (tests/test_gpu_parity.py
    TIGHT), 0.0 for an empty row, and the twin's bits"""
    pos = real_positions(layout)
    assert m.nrows == layout.nrows and m.nbins == layout.nbins and m.count_bytes == layout.count_bytes == twin.count_bytes, what
    assert twin.nrows == pos.size
    real = np.zeros(layout.nrows, dtype=bool)
    real[pos] = True
    for row0, nrows in windows(layout):
        got = m.counts(row0, nrows)
        exp = window_counts(layout, row0, nrows)
        assert got.dtype == np.uint32 and np.array_equal(got, exp), (what, row0, "count window differs")
        inside = np.arange(row0, row0 + nrows)
        assert not got[~real[inside]].any() and got[real[inside]].any(axis=1).all(), (what, row0)
    assert np.array_equal(twin.counts(), real_counts(layout)), what
    totals = np.zeros(layout.nrows, dtype=np.uint32)
    totals[pos] = real_counts(layout).sum(axis=1, dtype=np.uint64)
    assert np.array_equal(m.totals(), totals), (what, "totals differ")
    h, eh = m.entropy(), real_entropies(layout)
    worst = float((np.abs(h[pos] - eh) / np.maximum(1.0, np.abs(eh))).max())
    print(f"{what}: worst |H - oracle| / max(1, |H|) over the real rows = {worst:.3g}")
    assert (np.abs(h[pos] - eh) <= TIGHT * np.maximum(1.0, np.abs(eh))).all(), what
    assert (h[~real] == 0.0).all(), (what, "an empty row's entropy is not 0.0")
    assert same_bits(h[pos], twin.entropy()), (what, "entropies differ from the twin's bits")


def test_build_and_read_back(far):
    _assert_read_back(far.layout, far.m, far.twin, far.layout.name)


@pytest.mark.parametrize("route", ["device", "packed"])
def test_other_build_routes_of_16_bit_rows(ctx, route):
    """u16-k6 from sequences resident in HBM (a torch tensor) and from the packed form (pack_host +
    build_matrix_packed), one at a time, the twin by the same route"""
    layout = LAYOUTS[0]
    assert layout.name == "u16-k6"
    _release_resident()
    free_before = _guard(ctx, layout)
    m, keep = _build(ctx, route, *stream(layout), layout.k)
    twin, keep_twin = _build(ctx, route, *_twin_stream(layout), layout.k)
    try:
        _assert_read_back(layout, m, twin, f"{layout.name} {route}")
    finally:
        twin.close()
        m.close()
        for x in (keep, keep_twin):
            if hasattr(x, "close"):
                x.close()
        del keep, keep_twin
    _assert_released(ctx, layout, free_before)


# ---------------------------------------------------------------- 2. the canonical fold
def _assert_folded_rows(f, src, ref, rows_of, what):
    """the assertions of test_gpu_canonical.assert_folded over the rows of the read-back windows (`rows_of(row0, nrows)`
    -> the rows of `ref` that window holds): shape and flags, folded counts, totals unchanged, entropies within
    ENTROPY_TOL of oracle.entropy over the folded rows, +0.0 for a row without a valid k-mer"""
    counts, totals, ent, where = ref
    k = src.k
    assert f.is_canonical and f.k == k and f.num_states == 4 and f.count_bytes == src.count_bytes, what
    assert f.nrows == src.nrows and f.nbins == canonical_count(k) == counts.shape[1], what
    for row0, nrows in rows_of:
        got = f.counts(row0, nrows)
        exp = np.zeros_like(got)
        inside = (where >= row0) & (where < row0 + nrows)
        exp[where[inside] - row0] = counts[inside]
        assert got.dtype == np.uint32 and np.array_equal(got, exp), (what, row0, "folded counts differ")
    assert np.array_equal(f.totals(), src.totals()), what
    h, t = f.entropy(), f.totals()
    assert np.array_equal(t[where], totals), what
    worst = float(np.abs(h[where] - ent).max())
    print(f"{what}: k = {k}, worst |H - oracle.entropy| over the real rows = {worst:.3g}")
    assert worst <= ENTROPY_TOL, what
    assert (np.ascontiguousarray(h[t == 0]).view(np.uint64) == 0).all(), what
    return h


def test_canonical_fold(far):
    """CountMatrix.canonical() of the whole matrix: the far rows against the numpy fold of the oracle's counts
    (test_canonical_host.folded_of_counts), totals unchanged, entropies as test_gpu_canonical holds them; the twin's
    bits"""
    layout, m, twin, pos = far.layout, far.m, far.twin, far.pos
    ref = folded_of_counts(real_counts(layout), layout.k)
    f = m.canonical()
    try:
        _note_free(far.ctx, f"{layout.name} and its folded copy")
        h = _assert_folded_rows(f, m, ref + (pos,), windows(layout), f"{layout.name} fold")
        ft = twin.canonical()
        try:
            ht = _assert_folded_rows(ft, twin, ref + (np.arange(pos.size),), [(0, pos.size)], f"{layout.name} twin fold")
            assert same_bits(h[pos], ht), "folded entropies differ from the twin's bits"
        finally:
            ft.close()
        assert not m.is_canonical
    finally:
        f.close()


# ---------------------------------------------------------------- 3. selections
def _run_selection(far, run, exp, engine, what):
    sel = run(far.m)
    try:
        s = _assert_selection(sel, exp)
        print(f"{far.layout.name} {what}: engine {s.engine}, size {s.size}, accepts {s.n_accepts}, arbitrated "
              f"{s.n_arbitrated}, rows scored {s.rows_scored}")
        assert s.engine == engine, (what, "engine", s.engine)
        # No decision of these runs lies within the arbiter's band of its threshold: only a copy of the set's lowest
        # member scores exactly the threshold, and that is test_tie_takes_the_arbiter's case.  (A member's row read
        # from a wrapped address makes the persistent engine's own sum checks fail and hands decisions to the arbiter,
        # which replays them right: the answer stays the oracle's, this count does not stay 0.)
        assert s.n_arbitrated == 0, (what, "arbitrated", s.n_arbitrated)
        return s
    finally:
        sel.close()


@pytest.mark.parametrize("n", [N_SELECT, N_FRONT], ids=lambda n: f"n{n}")
def test_nmost(far, n):
    """nmost(40) over the whole stream.  The seeds are the first 40 positions, of which 0 .. 7 hold a valid k-mer
    (src/records.rs:299-306): a set of 8, the oracle's over the real rows with n = 8 (test_far_rows_host.oracle_nmost_whole).
    nmost(8) is the same selection with room for 8: at 4096 bins of 16-bit counts the persistent engine then keeps the
    members' count rows in LDS (its SMALL instantiation, up to 13 members)"""
    exp, acc = oracle_nmost_whole(far.layout)
    s = _run_selection(far, lambda m: m.nmost(n), exp, far.layout.engine_nmost, f"nmost({n})")
    assert s.n_accepts == acc and s.rows_scored >= far.pos.size - N_SELECT
    assert int((exp.members()[0] >= far.layout.r_star).sum()) >= MIN_WHOLE_FAR  # (members fetched from behind r*)


def test_max_divergent(far):
    _run_selection(far, lambda m: m.max_divergent(*MAX_ARGS), oracle_max(far.layout), far.layout.engine_max, "max")


def test_nmost_multi_launch(far, monkeypatch):
    monkeypatch.setenv("DVS_NO_PERSIST", "1")
    exp, acc = oracle_nmost_whole(far.layout)
    s = _run_selection(far, lambda m: m.nmost(N_SELECT), exp, 0, "nmost, DVS_NO_PERSIST")
    assert s.n_accepts == acc


def test_max_divergent_multi_launch(far, monkeypatch):
    monkeypatch.setenv("DVS_NO_PERSIST", "1")
    _run_selection(far, lambda m: m.max_divergent(*MAX_ARGS), oracle_max(far.layout), 0, "max, DVS_NO_PERSIST")


def test_nmost_explicit_order(far):
    """an order that lists the real rows' positions only (scan_rows_general: the row of a position is order[position]):
    the oracle's nmost(40) over the real rows alone, 27 of its seeds and most of its members behind r*; the members are
    named by their place in the order"""
    order = far.pos.astype(np.uint32)
    s = _run_selection(far, lambda m: m.nmost(N_SELECT, order=order), oracle_nmost_by_order(far.layout), 0, "nmost, order")
    assert s.n_accepts == oracle_nmost(far.layout)[1]


def test_tie_takes_the_arbiter(far):
    """the planted pair made to tie (test_far_rows_host.tie_case): the host arbiter replays the decision over far rows
    it fetches by position (csrc/exact_set.cpp).  The assertions of _assert_selection but for the spread of the scores
    (std, cov): three rows of 4^9 bins share next to no k-mer, every member's delta_jsd is log2(3) - 1 up to 1e-13, and
    the standard deviation of such a set is rounding noise in the oracle as on the device."""
    order, exp = tie_case(far.layout)
    sel = far.m.nmost(TIE_N, order=order)
    try:
        s, got = sel.summary(), sel.members(with_freqs=True)
        elab, edelta, eent, efreq = exp.members(with_freqs=True)
        print(f"{far.layout.name} tie: engine {s.engine}, accepts {s.n_accepts}, arbitrated {s.n_arbitrated}, rechecked "
              f"{s.rows_rechecked}")
        assert s.n_arbitrated >= 1 and s.size == exp.size == TIE_N
        assert got.positions.tolist() == elab.tolist(), "selected ids / member order differ"
        assert (got.kfreqs == efreq).all()
        np.testing.assert_allclose(got.delta_jsd, edelta, rtol=RTOL, atol=1e-13)
        np.testing.assert_allclose(got.entropy, eent, rtol=RTOL)
        for name in ("total_jsd", "mean_delta_jsd"):
            g, e = getattr(s, name), getattr(exp, name)
            assert abs(g - e) <= RTOL * abs(e) + 1e-13, (name, g, e)
        assert s.lowest_index == exp.lowest_index
    finally:
        sel.close()


# ---------------------------------------------------------------- 4. scores of a finished selection
def _assert_read_back_scores(far, sel, oset, members, what):
    """delta_jsd of every row of the big matrix against the selection `sel` (score_kernel): the real rows against
    oracle.SummedRecords.delta_jsd within TIGHT (test_readback_host.assert_scores, as tests/test_gpu_readback.py: NaN for
    NaN -- the score has no clamp), NaN for a row without a valid k-mer; with the rows' positions as labels a member
    (`members`: matrix rows) scores exactly 0.0; the twin's rows as queries of the same selection give the same bits.
    -> the number of finite scores among the real rows"""
    layout, m, pos = far.layout, far.m, far.pos
    escores = np.array([oset.delta_jsd(*oracle.to_kfreqs(s, 4, layout.k)) for s in real_seqs(layout)])
    got = sel.delta_jsd(m)
    real = np.zeros(layout.nrows, dtype=bool)
    real[pos] = True
    assert got.shape == (layout.nrows,) and np.isnan(got[~real]).all(), what
    worst = assert_scores(got[pos], escores, what)
    finite = int(np.isfinite(escores).sum())
    print(f"{what}: {finite} finite scores among the real rows, largest difference {worst:.3g}")
    assert same_bits(sel.delta_jsd(far.twin), got[pos]), (what, "scores differ from the twin rows' bits")
    lab = sel.delta_jsd(m, np.arange(layout.nrows, dtype=np.uint32))
    assert (lab[members] == 0.0).all() and not np.signbit(lab[members]).any(), what
    rest = np.ones(layout.nrows, dtype=bool)
    rest[members] = False
    assert same_bits(lab[rest], got[rest]), what
    return finite


def test_scores_of_a_finished_selection(far):
    """against a finished nmost(40) over the real rows, most of whose members lie behind r*.  After its accepts the
    running sum has drifted below the lowest member's own frequency in some bins, and rows of 600 to 1500 bases miss
    most bins: at 4^7 and 4^9 bins nearly every score is NaN in the oracle too (tests/test_readback_host.py), and the
    NaN pattern is what this run compares there (at 4^6 bins all 123 are finite); the values are compared at every
    width in test_scores_of_a_set_of_far_rows"""
    layout = far.layout
    exp, _ = oracle_nmost(layout)
    order = far.pos.astype(np.uint32)
    sel = far.m.nmost(N_SELECT, order=order, labels=order)
    try:
        members = sel.members(with_freqs=False).labels.astype(np.int64)
        assert members.tolist() == exp.members()[0].tolist()
        _assert_read_back_scores(far, sel, exp, members, f"{layout.name} read-back, nmost")
    finally:
        sel.close()


def test_scores_of_a_set_of_far_rows(far):
    """against the set of 40 rows behind r* (MODE_SET, oracle.SummedRecords.from_seqs): no member was ever replaced,
    the sum has not drifted, every real row's score is finite and compared by value"""
    layout = far.layout
    rows = far.pos[far.pos >= layout.r_star][:N_SELECT].astype(np.uint32)
    oset = oracle.SummedRecords.from_seqs([row_seq(layout, int(p)) for p in rows], layout.k, 4, labels=rows)
    sel = far.m.as_set(order=rows, labels=rows)
    try:
        s = _assert_selection(sel, _ByPlace(oset))
        assert s.size == N_SELECT
        finite = _assert_read_back_scores(far, sel, oset, rows.astype(np.int64), f"{layout.name} read-back, set")
        assert finite == far.pos.size
    finally:
        sel.close()


class _ByPlace:
    """an oracle set whose members are named by their place in the order (the device's `positions`)"""

    def __init__(self, oset):
        self._oset = oset

    def members(self, with_freqs=False):
        out = self._oset.members(with_freqs)
        return (np.arange(len(out[0])),) + tuple(out[1:])

    def __getattr__(self, name):
        return getattr(self._oset, name)


# ---------------------------------------------------------------- 5. distances through row lists
def _assert_truth(layout, mode, got, truth):
    """cells against the long-double truth: jsd within tol_derived(B) absolute, euclidean within EUCLID_RTOL relative"""
    err = np.abs(got.astype(np.longdouble) - truth)
    if mode == "jsd":
        print(f"{layout.name} jsd: largest |cell - truth| = {float(err.max()):.3g} (bound {tol_derived(layout.nbins):.3g})")
        assert (err <= tol_derived(layout.nbins)).all()
    else:
        rel = err[truth > 0] / truth[truth > 0]
        print(f"{layout.name} euclidean: largest relative error = {float(rel.max()):.3g}")
        assert (err <= EUCLID_RTOL * np.abs(truth)).all()


def _cells(far, mode):
    """the q x r cells of matrix_cross_distances over the big matrix, held to the long-double truth (jsd: tol_derived(B)
    absolute; euclidean: EUCLID_RTOL relative) and to the twin's bits -- once per layout and mode; what the checks
    below feed their helpers"""
    from diverseseq_amd import distance

    key = ("cells", mode)
    if key not in far.cache:
        layout = far.layout
        q, r = row_lists(layout)
        got = distance.matrix_cross_distances(far.m, far.m, mode, q_rows=far.pos[q], r_rows=far.pos[r])
        _assert_truth(layout, mode, got, truth_cells(layout, mode))
        assert not np.isnan(got).any()
        assert same_bits(got, distance.matrix_cross_distances(far.twin, far.twin, mode, q_rows=q, r_rows=r)), \
            "cells differ from the twin's bits"
        far.cache[key] = got
    return far.cache[key]


def _square(far, mode):
    """the q x q cells: a call of its own over the far rows, which must give the bits of the checked q x r cells"""
    from diverseseq_amd import distance

    q, _ = row_lists(far.layout)
    d = distance.matrix_cross_distances(far.m, far.m, mode, q_rows=far.pos[q], r_rows=far.pos[q])
    assert same_bits(d, square_of(_cells(far, mode), far.layout))
    assert d.shape == (N_Q, N_Q)
    return d


@pytest.mark.parametrize("mode", MODES)
def test_cross_distances(far, mode):
    """45 x 107 rows of the big matrix against itself, a ragged last 32-row tile on each side; both orders of the sides"""
    from diverseseq_amd import distance

    _cells(far, mode)
    q, r = row_lists(far.layout)
    back = distance.matrix_cross_distances(far.m, far.m, mode, q_rows=far.pos[r], r_rows=far.pos[q])
    assert same_bits(back, distance.matrix_cross_distances(far.twin, far.twin, mode, q_rows=r, r_rows=q))
    _assert_truth(far.layout, mode, back, truth_cells(far.layout, mode).T)


@pytest.mark.parametrize("mode", MODES)
def test_nearest(far, mode):
    from diverseseq_amd import distance

    d = _cells(far, mode)
    q, r = row_lists(far.layout)
    for kk in (1, 5):
        got = distance.matrix_nearest(far.m, far.m, kk, mode, q_rows=far.pos[q], r_rows=far.pos[r])
        assert_nearest(got, d, kk)
        tw = distance.matrix_nearest(far.twin, far.twin, kk, mode, q_rows=q, r_rows=r)
        assert np.array_equal(got[0], tw[0]) and same_bits(got[1], tw[1])


@pytest.mark.parametrize("mode", MODES)
def test_within(far, mode):
    """two radii that are cells of the checked matrix: its median and its first decile"""
    from diverseseq_amd import distance

    d = _cells(far, mode)
    q, r = row_lists(far.layout)
    cells = np.sort(d.reshape(-1))
    for radius in (float(cells[cells.size // 2]), float(cells[cells.size // 10])):
        nb = distance.matrix_within(far.m, far.m, radius, mode, q_rows=far.pos[q], r_rows=far.pos[r])
        assert_within(nb, d, radius, what=(far.layout.name, mode))
        assert nb.index.size > N_Q  # more than every row's own cell
        assert same_neighbours(nb, distance.matrix_within(far.twin, far.twin, radius, mode, q_rows=q, r_rows=r))


@pytest.mark.parametrize("mode", MODES)
def test_threshold_clusters(far, mode):
    from diverseseq_amd import distance

    d = _square(far, mode)
    q, _ = row_lists(far.layout)
    v = np.sort(d[np.triu_indices(N_Q, 1)])
    counts = set()
    for t in (float(v[N_Q // 2]), float(v[2 * N_Q])):  # cells of the matrix: about half an edge a row, about two
        got = distance.matrix_threshold_clusters(far.m, t, mode, rows=far.pos[q])
        assert_labels(got, d, t, what=(far.layout.name, mode))
        tw = distance.matrix_threshold_clusters(far.twin, t, mode, rows=q)
        assert np.array_equal(got.labels, tw.labels) and got.n_clusters == tw.n_clusters
        counts.add(got.n_clusters)
    assert all(1 < c < N_Q for c in counts)


@pytest.mark.parametrize("mode", MODES)
def test_cluster_scores(far, mode):
    from diverseseq_amd import distance

    d = _square(far, mode)
    q, _ = row_lists(far.layout)
    labels = np.arange(N_Q) % 4
    got = distance.matrix_cluster_scores(far.m, labels, mode, rows=far.pos[q])
    assert_cluster_scores(got, d, labels, what=f"{far.layout.name} {mode}")
    assert_same_cluster_scores(got, distance.matrix_cluster_scores(far.twin, labels, mode, rows=q), "the twin's bits")


@pytest.mark.parametrize("mode", MODES)
def test_cophenet(far, mode):
    """the tree: scipy's average linkage of the checked cells"""
    from diverseseq_amd import distance

    d = _square(far, mode)
    q, _ = row_lists(far.layout)
    Z = scipy_linkage(condensed(d), "average")
    got = distance.matrix_cophenet(far.m, Z, mode, rows=far.pos[q], matrix=True)
    assert_cophenet_scores(got, d, Z, what=f"{far.layout.name} {mode}")
    assert_same_cophenet_scores(got, distance.matrix_cophenet(far.twin, Z, mode, rows=q, matrix=True), "the twin's bits")
