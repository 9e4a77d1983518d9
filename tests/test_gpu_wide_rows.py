"""Selections and distances over rows of more than 16 384 bins, against the oracle and the long-double yardstick.

Past 16 384 bins the state vector no longer fits the scan's LDS: scan_kernel<T, false> reads it from global memory
(csrc/select.hip, sel_geometry / scan_body), the persistent engine refuses (csrc/persist.hip, dvs_persist_setup) and the
multi-launch kernels -- seed / rebuild / resolve / loo / finalize, max_batch_jobs / max_batch_decide -- serve the whole
selection with loops over B 4 to 16 times longer than any other test drives them; the stepwise mode runs its plain step
path; the host arbiter and the row log replay rows of 65 536 doubles.  Every selection test here asserts
`summary().engine == 0` first: it ran the path it is about.

The cases (shapes, seeds, set sizes) and the conditions that keep them meaningful are those of
tests/test_wide_rows_host.py, which checks them on the CPU from the oracle alone.

Two float checks on every selection: the project's contract (`_assert_selection`: 1e-6 relative) and the engine's own
band -- every delta_jsd and the total_jsd within sel_band(B) = 4 B 2^-52 max(1, log2 B) absolute of the oracle's value.
Measured on an MI355X, largest |device - oracle| / sel_band(B) per shape over every test below (they print it):
    65 536 bins (4 states, k = 8)   0.0072x  (0.025x in the FAST_BAND case, whose rows are 20 000 bases long)
    78 125 bins (5 states, k = 7)   0.0084x
   160 000 bins (20 states, k = 4)  0.0041x
   262 144 bins (4 states, k = 9)   0.0027x
i.e. differences of 7e-12 to 2e-11 against bands of 9e-10 to 4e-9: the band is a worst-case bound over B roundings, and
the rows of these cases fill 2 to 25 % of their bins."""
import numpy as np
import pytest

import oracle
from test_distance_truth_host import distance_cases
from test_bands_host import FAST_BAND, _band_stream
from test_gpu_parity import _assert_selection
from test_maxmin_host import same_bits
from test_readback_host import assert_scores
from test_wide_rows_host import (BAND_CASE, FREQS_CASE, LARGE_CASE, MAX_CASES, MAXMIN_CASE, NMOST_CASES, ORDER_CASE,
                                 READBACK_CASE, STEPWISE_CASE, TIE_MAX, TIE_NMOST_N, TIE_STREAMS, WIDE_DISTANCE_CASES,
                                 freqs_case, oracle_max, oracle_nmost, order_case, readback_queries, readback_scores,
                                 sel_band, stream_seqs, tie_copies_of_the_lowest, tie_oracle, tie_seqs)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from diverseseq_amd import engine

    return engine.default_context()


def _ids(case):
    return f"s{case.stream.states}_k{case.stream.k}"


def _build(ctx, stream):
    m = ctx.build_matrix(stream_seqs(stream), stream.k, stream.states)
    assert m.nbins == stream.nbins and m.count_bytes == 4  # (whole-sequence builds keep 16-bit rows up to 4096 bins only)
    return m


def _assert_band(sel, exp, nbins, what):
    """every delta_jsd and the total_jsd within sel_band(nbins) absolute of the oracle's (the multiples are printed)"""
    band = sel_band(nbins)
    got, s = sel.members(with_freqs=False), sel.summary()
    diff = np.abs(np.asarray(got.delta_jsd, dtype=np.float64) - exp.members()[1])
    worst_delta, worst_total = float(diff.max()) / band, abs(s.total_jsd - exp.total_jsd) / band
    print(f"{what}: B = {nbins}, size {s.size}, accepts {s.n_accepts}, arbitrated {s.n_arbitrated}, rechecked "
          f"{s.rows_rechecked}; |device - oracle| / sel_band: delta_jsd {worst_delta:.3g}, total_jsd {worst_total:.3g} "
          f"(sel_band = {band:.3g})")
    assert worst_delta <= 1.0 and worst_total <= 1.0, (what, worst_delta, worst_total)


def _assert_wide(sel, exp, nbins, what, arbitrated=False):
    """engine first, then the oracle's set by the project's contract, then the engine's own band"""
    s = sel.summary()
    assert s.engine == 0, f"{what}: not the multi-launch engine"
    _assert_selection(sel, exp)
    _assert_band(sel, exp, nbins, what)
    assert (s.n_arbitrated > 0) == arbitrated, (what, s.n_arbitrated)
    return s


# ---------------------------------------------------------------- 1. nmost against the oracle, every shape
@pytest.mark.parametrize("case", NMOST_CASES, ids=_ids)
def test_nmost_vs_oracle(ctx, case):
    """reference src/records.rs:311-342 at 65 536, 78 125, 160 000 and 262 144 bins: member order and ids, frequency rows
    bit-exact, delta_jsd, entropies, the four summary statistics, lowest_index, and the oracle's accept count"""
    exp, acc = oracle_nmost(case)
    m = _build(ctx, case.stream)
    sel = m.nmost(case.n)
    s = _assert_wide(sel, exp, case.stream.nbins, f"nmost {_ids(case)}")
    assert s.n_accepts == acc, (s.n_accepts, acc)
    assert s.rows_scored >= case.stream.nseq - case.n
    sel.close()
    m.close()


# ---------------------------------------------------------------- 2. max_divergent: the max-batch kernels over wide rows
@pytest.mark.parametrize("case", MAX_CASES, ids=lambda c: f"{_ids(c)}_{c.stat}")
def test_max_divergent_vs_oracle(ctx, case):
    """reference src/records.rs:390-454: the set grows beyond min_size (the host file checks that on the oracle)"""
    exp = oracle_max(case)
    m = _build(ctx, case.stream)
    sel = m.max_divergent(case.min_size, case.max_size, case.stat)
    s = _assert_wide(sel, exp, case.stream.nbins, f"max {_ids(case)} {case.stat}")
    assert s.size > case.min_size
    sel.close()
    m.close()


# ---------------------------------------------------------------- 3. a large set at wide rows
def test_large_set(ctx):
    """nmost(70) at 65 536 bins: more members than one wave's argmin, a member matrix of 37 MB"""
    exp, acc = oracle_nmost(LARGE_CASE)
    m = _build(ctx, LARGE_CASE.stream)
    sel = m.nmost(LARGE_CASE.n)
    s = _assert_wide(sel, exp, LARGE_CASE.stream.nbins, "nmost(70) s4_k8")
    assert s.n_accepts == acc
    sel.close()
    m.close()


# ---------------------------------------------------------------- 4. explicit order and labels
class _ByPosition:
    """the oracle's set with its members named by stream position (the device's `positions`) instead of by label"""

    def __init__(self, exp, positions):
        self._exp, self._positions = exp, np.asarray(positions)

    def members(self, with_freqs=False):
        return (self._positions,) + tuple(self._exp.members(with_freqs)[1:])

    def __getattr__(self, name):
        return getattr(self._exp, name)


def test_explicit_order_and_labels(ctx):
    """a shuffled order and labels with ids repeated later in the stream: scan_rows_general's label and inset skips with
    the state vector in global memory (built as test_gpu_parity.test_explicit_order_and_labels)"""
    seqs, order, exp, acc = order_case()
    m = _build(ctx, ORDER_CASE.stream)
    sel = m.nmost(ORDER_CASE.n, order=order, labels=order)
    assert sel.summary().engine == 0
    pos = sel.members(False).positions
    assert [int(order[p]) for p in pos] == exp.members()[0].tolist(), "selected ids / member order differ"
    s = _assert_wide(sel, _ByPosition(exp, pos), ORDER_CASE.stream.nbins, "order + labels s4_k8")
    assert s.n_accepts == acc
    sel.close()
    m.close()


# ---------------------------------------------------------------- 5. frequency rows (T = double)
def test_frequency_rows(ctx):
    """ctx.matrix_from_freqs at 65 536 bins: the chunk-merge form of the rows; the expectation is the oracle over the
    sequences the rows were made from"""
    rows, exp = freqs_case()
    m = ctx.matrix_from_freqs(rows)
    assert m.count_bytes == 0 and m.nbins == FREQS_CASE.stream.nbins
    sel = m.nmost(FREQS_CASE.n)
    s = _assert_wide(sel, exp, m.nbins, "frequency rows s4_k8")
    assert s.n_accepts == oracle_nmost(FREQS_CASE)[1]
    sel.close()
    m.close()


# ---------------------------------------------------------------- 6. stepwise (row-sharded) mode
def test_stepwise_mode(ctx):
    """parallel.nmost_exact at world 1 (as test_gpu_parity.test_exact_mode_fast_step_shapes): the two-launch step's LDS
    no longer fits, the plain step path serves.  ids, accept count, delta_jsd and total_jsd."""
    import torch

    from diverseseq_amd import parallel

    case = STEPWISE_CASE
    exp, acc = oracle_nmost(case)
    dev = torch.device("cuda", 0)
    m = _build(ctx, case.stream)
    _, order = parallel.shard_order(case.stream.nseq, case.n, 0, 1, block=32)
    sel = parallel.nmost_exact(ctx, m, order, case.n, dev, 1)
    s = _assert_wide(sel, exp, case.stream.nbins, "stepwise s4_k8")
    assert s.n_accepts == acc and acc >= 1
    sel.close()
    m.close()


# ---------------------------------------------------------------- 7. ties at wide rows
@pytest.mark.parametrize("stream", TIE_STREAMS, ids=lambda s: f"s{s.states}_k{s.k}")
def test_ties_take_the_arbiter(ctx, stream):
    """every sequence twice: the device hands the exact ties to the host arbiter, which replays the event log over rows
    of 65 536 (78 125) doubles (csrc/exact_set.cpp) -- the oracle's ids, arbitrations > 0; without the arbiter the call
    is refused.  Every candidate that is a copy of the set's lowest member scores exactly the threshold: it has to pass
    the f64 tier (precise_row, at 78 125 bins its scalar loop) on its way to the arbiter."""
    from diverseseq_amd import _lib

    seqs = tie_seqs(stream)
    nm, mx = tie_oracle(stream)
    what = f"s{stream.states}_k{stream.k}"
    m = ctx.build_matrix(seqs, stream.k, stream.states)
    sel = m.nmost(TIE_NMOST_N)
    s = _assert_wide(sel, nm, stream.nbins, f"ties nmost {what}", arbitrated=True)
    assert s.rows_rechecked >= tie_copies_of_the_lowest(stream) >= 1, (s.rows_rechecked, tie_copies_of_the_lowest(stream))
    sel.close()
    lo, hi, stat = TIE_MAX
    sel = m.max_divergent(lo, hi, stat)
    _assert_wide(sel, mx, stream.nbins, f"ties max {what}", arbitrated=True)
    sel.close()
    with pytest.raises(NotImplementedError, match="ambiguous decision"):
        m.nmost(TIE_NMOST_N, flags=_lib.SELECT_NO_ARBITER)
    m.close()


# ---------------------------------------------------------------- 8. candidates inside FAST_BAND
@pytest.fixture(scope="module")
def band_k8():
    """two near-copies of the prefix's lowest member at the threshold -+ 0.5 x FAST_BAND, crafted once: 4.6 s of CPU
    measured (2 x ~2 000 scores of 65 536 bins).  The rows are 20 000 bases long: at 3 000 to 6 000 bases a substitution
    moves the score by 1e-5 or not at all (most k-mers of so sparse a row are singletons) and _craft cannot land within
    0.08 x FAST_BAND of a target; a finer grain needs longer rows, not a wider tolerance."""
    c = BAND_CASE
    return _band_stream(c["k"], c["n"], c["length"], c["nprefix"], [x * FAST_BAND for x in c["mults"]], c["seed"])


def test_candidates_inside_the_fast_band(ctx, band_k8):
    """reference src/records.rs:86-92 for near-copies of the lowest member whose exact score is the threshold +- 0.5 x
    FAST_BAND (test_gpu_configs.test_candidates_inside_the_fast_band_k7 at 65 536 bins): the f32 tier may not decide
    them, the f64 tier must, without the arbiter; sel_band is 9e-10 there, FAST_BAND 4e-7 -- the tiers compose"""
    seqs, oset, margins = band_k8
    c = BAND_CASE
    exp = oracle.nmost(seqs, c["n"], c["k"], 4)
    assert exp.members()[0].tolist() == oset.members()[0].tolist()  # (the tracked set is the stream's)
    m = ctx.build_matrix(seqs, c["k"], 4)
    sel = m.nmost(c["n"])
    s = _assert_wide(sel, exp, 4 ** c["k"], "band s4_k8")
    m0 = ctx.build_matrix(seqs[:c["nprefix"]], c["k"], 4)
    sel0 = m0.nmost(c["n"])
    s0 = sel0.summary()
    assert s0.engine == 0
    sure = sum(1 for g in margins if abs(g) <= 0.6 * FAST_BAND)
    assert sure == len(c["mults"]) == 2, margins
    assert s.rows_rechecked >= s0.rows_rechecked + sure, (s.rows_rechecked, s0.rows_rechecked)
    for x in (sel, sel0, m, m0):
        x.close()


# ---------------------------------------------------------------- 9. score read-back
def test_score_read_back(ctx):
    """delta_jsd of query rows against a finished wide selection (score_kernel) and members(with_freqs=True)
    (gather_members_kernel), in the manner of tests/test_gpu_readback.py: NaN for NaN (the score has no clamp; a row
    without a valid k-mer is NaN), finite values within TIGHT and within sel_band; a member's label scores 0.0"""
    case = READBACK_CASE
    exp, _ = oracle_nmost(case)
    m = _build(ctx, case.stream)
    sel = m.nmost(case.n)
    assert sel.summary().engine == 0
    mem = sel.members(with_freqs=True)
    elab, _, _, efreq = exp.members(with_freqs=True)
    assert mem.positions.tolist() == elab.tolist() and (mem.kfreqs == efreq).all()
    queries, escores = readback_queries(), readback_scores()
    q = ctx.build_matrix(queries, case.stream.k, case.stream.states)
    got = sel.delta_jsd(q)
    worst = assert_scores(got, escores, "wide read-back")
    assert np.isnan(got[-1]) and np.isfinite(got[2])
    print(f"read-back s4_k8: oracle scores {escores}, largest finite difference {worst:.3g} "
          f"= {worst / sel_band(case.stream.nbins):.3g} x sel_band")
    assert worst <= sel_band(case.stream.nbins)
    assert np.array_equal(np.isnan(sel.delta_jsd(q)), np.isnan(got))
    lab = sel.delta_jsd(q, [int(elab[0]), 0xFFFFFFF0, int(elab[-1]), 0xFFFFFFFF])  # members' labels score exactly 0.0
    assert lab[0] == 0.0 and lab[2] == 0.0 and np.isnan(lab[3])
    assert_scores(lab[1:2], escores[1:2], "a label that is no member's")
    for x in (q, sel, m):
        x.close()


# ---------------------------------------------------------------- 10. distances at wide rows
# (the cells against the long-double yardstick: tests/test_gpu_distance_truth.py over the same two cases)
@pytest.mark.parametrize("mode", ["jsd", "euclidean"])
@pytest.mark.parametrize("name", WIDE_DISTANCE_CASES)
def test_cross_distances_give_the_square_paths_bits(ctx, name, mode):
    from diverseseq_amd import distance

    square = {"jsd": distance.matrix_jsd_distances, "euclidean": distance.matrix_euclidean_distances}[mode]
    case = next(c for c in distance_cases() if c.name == name)
    cut = 5
    ms, mq, mr = (ctx.build_matrix(x, case.k, case.num_states) for x in (case.seqs, case.seqs[:cut], case.seqs[cut:]))
    try:
        assert ms.nbins == case.nbins > 16_384
        sq = square(ms)
        assert not np.isnan(sq).any() and (sq[~np.eye(case.nrows, dtype=bool)] > 0).all()
        assert same_bits(distance.matrix_cross_distances(mq, mr, mode), sq[:cut, cut:])
        assert same_bits(distance.matrix_cross_distances(mr, mq, mode), sq[cut:, :cut])
        qr, rr = [11, 0, 7, 11], [3, 10, 1]
        assert same_bits(distance.matrix_cross_distances(ms, ms, mode, q_rows=qr, r_rows=rr), sq[np.ix_(qr, rr)])
        assert same_bits(distance.cross_distances(case.seqs[:cut], case.seqs[cut:], mode, k=case.k, num_states=case.num_states,
                                                  ctx=ctx), sq[:cut, cut:])
    finally:
        for x in (ms, mq, mr):
            x.close()


def test_maxmin_over_wide_rows(ctx):
    """one farthest-first case through test_gpu_maxmin.run_matrix_cases at k = 8, 4 states: a row without a valid k-mer
    and an exact duplicate among 40 rows of 65 536 bins"""
    from diverseseq_amd import distance
    from test_gpu_maxmin import run_matrix_cases

    s = MAXMIN_CASE
    seqs = list(stream_seqs(s))
    seqs[3] = np.full(40, s.states, np.uint8)
    seqs[20] = seqs[2].copy()
    m = ctx.build_matrix(seqs, s.k, s.states)
    try:
        assert m.nbins == 65_536
        run_matrix_cases(m, "jsd", distance.matrix_jsd_distances(m))
    finally:
        m.close()
