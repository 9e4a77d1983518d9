"""The cases of tests/test_gpu_wide_rows.py, pinned on the CPU before they are used on the device.

Rows of more than 16 384 bins leave the code every other selection test runs: the state vector no longer fits the
scan's LDS and is read from global memory (csrc/select.hip, sel_geometry: `base_in_lds` false), the persistent engine
refuses (csrc/persist.hip, dvs_persist_setup) and the multi-launch kernels serve the whole selection, the stepwise mode
loses its two-launch step.  This module holds the shapes, seeds and set sizes of the GPU module as constants, the oracle's
answer for each of them (computed once per session), and the conditions under which those cases say something:

  * the oracle's `nmost` accepts at least MIN_ACCEPTS rows beyond the seeds, `max` ends larger than its min_size;
  * no two rows of a case without ties are equal (so that `n_arbitrated == 0` is a fair expectation of the device),
    and the tie case really holds every row twice;
  * every bin count takes the branch its case is about: B * 8 > 128 KiB, B % 256 zero or not as SHAPES says.

`sel_band(B)` is the engine's own decision band 4 B eps max(1, H) with H <= log2 B (csrc/select_dev.h): the width inside
which the engine says it cannot tell its score from the reference's.  The GPU module holds every delta_jsd and total_jsd
of a wide selection to it, absolutely, beside the project's 1e-6 relative contract."""
import functools
import math
from typing import NamedTuple

import numpy as np
import pytest

import oracle

LDS_STATE_LIMIT = 128 * 1024  # bytes of state vector the scan keeps in LDS (csrc/select.hip sel_geometry)
MIN_ACCEPTS = 3

# (states, k): (bins, bins a multiple of 256) -- the smallest shapes that reach each branch of the wide path
SHAPES = {
    (4, 8): (65_536, True),     # the vector load4 / fast4 branch, state vector in global memory
    (5, 7): (78_125, False),    # odd: the scalar lane loop with a partial last pass, the (B & 1) staging split
    (20, 4): (160_000, True),   # protein alphabet, rolled k-mer index in the histogram
    (4, 9): (262_144, True),    # 1 MiB count rows, a 2 MiB state vector
}


def sel_band(nbins: int) -> float:
    """the engine's decision band with the entropy at its largest: 4 B 2^-52 max(1, log2 B)"""
    return 4.0 * nbins * 2.0 ** -52 * max(1.0, math.log2(nbins))


class Stream(NamedTuple):
    states: int
    k: int
    nseq: int
    length: int
    seed: int

    @property
    def nbins(self):
        return self.states ** self.k


class Nmost(NamedTuple):
    stream: Stream
    n: int


class Max(NamedTuple):
    stream: Stream
    min_size: int
    max_size: int
    stat: str


# ---- 1. nmost against the oracle, every shape
NMOST_CASES = (Nmost(Stream(4, 8, 300, 4000, 8101), 8), Nmost(Stream(5, 7, 250, 4000, 8102), 7),
               Nmost(Stream(20, 4, 200, 5000, 8123), 6), Nmost(Stream(4, 9, 150, 5000, 8104), 10))
# ---- 2. max_divergent, the max-batch kernels over wide rows
MAX_CASES = tuple(Max(Stream(s, k, 120, 3000, seed), 4, 30, stat)
                  for (s, k, seed) in ((4, 8, 8201), (5, 7, 8202)) for stat in ("stdev", "cov"))
# ---- 3. a set larger than one wave's argmin; d.M is 70 x 65 536 x 8 B = 37 MB
LARGE_CASE = Nmost(Stream(4, 8, 300, 5000, 8301), 70)
# ---- 4. explicit order and labels with repeated ids (built as test_gpu_parity.test_explicit_order_and_labels does)
ORDER_CASE = Nmost(Stream(4, 8, 300, 5000, 8401), 9)
ORDER_SEED, ORDER_REPEATS = 8402, 40
# ---- 5. frequency rows (T = double)
FREQS_CASE = Nmost(Stream(4, 8, 60, 5000, 8501), 6)
# ---- 6. stepwise mode: the stream of the first nmost case
STEPWISE_CASE = NMOST_CASES[0]
# ---- 7. ties: every sequence twice
# (60 unique sequences, 120 rows; the second stream beyond the issue's: precise_row's scalar tail runs only where a row of
# an odd bin count lands inside FAST_BAND, and a copy of the lowest member does)
TIE_STREAMS = (Stream(4, 8, 60, 5000, 8701), Stream(5, 7, 60, 5000, 8702))
TIE_NMOST_N = 6
TIE_MAX = (4, 12, "stdev")
# ---- 8. candidates inside FAST_BAND: arguments of test_bands_host._band_stream (k, n, length, nprefix, targets / FAST_BAND, seed)
BAND_CASE = dict(k=8, n=8, length=20_000, nprefix=150, mults=(-0.5, 0.5), seed=8801)
# ---- 9. score read-back: queries against the finished set of the first nmost case
READBACK_CASE = NMOST_CASES[0]
READBACK_QUERIES = ((4000, 60_000, 1_200_000), 8901)  # (lengths, seed), and one row without a valid k-mer behind them
# ---- 10. max-min over wide rows
MAXMIN_CASE = Stream(4, 8, 40, 3000, 9001)
# (the distance truth cases at (4, 8) and (5, 7) are entries of test_distance_truth_host.BINS_STATES_K)
WIDE_DISTANCE_CASES = ("bins_s4_k8", "bins_s5_k7")


@functools.lru_cache(maxsize=None)
def stream_seqs(stream: Stream):
    """i.i.d. uniform sequences of one length: every row scores about alike, so the greedy selection keeps accepting"""
    rng = np.random.default_rng(stream.seed)
    return [rng.integers(0, stream.states, size=stream.length, dtype=np.uint8) for _ in range(stream.nseq)]


@functools.lru_cache(maxsize=None)
def oracle_nmost(case: Nmost):
    """(the oracle's finished set, its accept count)"""
    return oracle.nmost_concat(*oracle.concat(stream_seqs(case.stream)), case.n, case.stream.k, case.stream.states)


@functools.lru_cache(maxsize=None)
def oracle_max(case: Max):
    return oracle.max_divergent(stream_seqs(case.stream), case.min_size, case.max_size, case.stream.k, case.stream.states,
                                case.stat)


@functools.lru_cache(maxsize=None)
def order_case():
    """(sequences, order with ORDER_REPEATS ids repeated later in the stream, the oracle's set over that stream)"""
    seqs = stream_seqs(ORDER_CASE.stream)
    order = np.random.default_rng(ORDER_SEED).permutation(len(seqs)).astype(np.uint32)
    order = np.concatenate([order, order[:ORDER_REPEATS]])
    s = ORDER_CASE.stream
    exp, acc = oracle.nmost_concat(*oracle.concat([seqs[i] for i in order]), ORDER_CASE.n, s.k, s.states, labels=order)
    return seqs, order, exp, acc


@functools.lru_cache(maxsize=None)
def freqs_case():
    """(frequency rows by the oracle, the oracle's set over the same sequences)"""
    s = FREQS_CASE.stream
    rows = np.stack([oracle.to_kfreqs(q, s.states, s.k)[0] for q in stream_seqs(s)])
    return rows, oracle_nmost(FREQS_CASE)[0]


@functools.lru_cache(maxsize=None)
def tie_seqs(stream: Stream):
    return [u for u in stream_seqs(stream) for _ in range(2)]  # each sequence twice, different ids


@functools.lru_cache(maxsize=None)
def tie_oracle(stream: Stream):
    """(the oracle's nmost set, its max set) over the doubled stream"""
    seqs, (lo, hi, stat) = tie_seqs(stream), TIE_MAX
    return (oracle.nmost(seqs, TIE_NMOST_N, stream.k, stream.states),
            oracle.max_divergent(seqs, lo, hi, stream.k, stream.states, stat))


@functools.lru_cache(maxsize=None)
def tie_copies_of_the_lowest(stream: Stream):
    """how many candidates of the doubled stream are a copy of the member that is the set's lowest when they arrive
    (select_nmost_divergent replayed step by step, src/records.rs:311-342): such a row scores exactly the threshold, so
    no f32 tier may decide it -- the device must take it through its f64 tier (rows_rechecked) to the arbiter"""
    seqs, n = tie_seqs(stream), TIE_NMOST_N
    oset = oracle.SummedRecords.from_seqs(seqs[:n], stream.k, stream.states)
    copies = 0
    for p in range(n, len(seqs)):
        f, h = oracle.to_kfreqs(seqs[p], stream.states, stream.k)
        low = int(oset.members()[0][oset.lowest_index])
        copies += bool((seqs[low] == seqs[p]).all())
        if oset.increases_jsd(f, h, p):
            oset.replace_lowest(f, h, p)
    assert oset.members()[0].tolist() == tie_oracle(stream)[0].members()[0].tolist()  # (the replay is the oracle's run)
    return copies


@functools.lru_cache(maxsize=None)
def readback_queries():
    """the query sequences: random ones of three lengths, then a row of invalid symbols (no valid k-mer: its score is
    NaN).  The score has no clamp (src/records.rs:70-84): a query that misses a bin in which the running sum has drifted
    below the lowest member's own frequency scores NaN in the oracle too (tests/test_readback_host.py); the longest
    query covers every bin and is compared by value."""
    lengths, seed = READBACK_QUERIES
    s = READBACK_CASE.stream
    rng = np.random.default_rng(seed)
    return [rng.integers(0, s.states, size=n, dtype=np.uint8) for n in lengths] + [np.full(40, s.states, np.uint8)]


@functools.lru_cache(maxsize=None)
def readback_scores():
    """the oracle's delta_jsd of the queries against the finished set of READBACK_CASE (NaN for the last)"""
    s = READBACK_CASE.stream
    exp = oracle_nmost(READBACK_CASE)[0]
    return np.array([exp.delta_jsd(*oracle.to_kfreqs(q, s.states, s.k)) for q in readback_queries()[:-1]] + [np.nan])


def _all_streams():
    out = [c.stream for c in NMOST_CASES + MAX_CASES] + [LARGE_CASE.stream, ORDER_CASE.stream, FREQS_CASE.stream,
                                                        MAXMIN_CASE] + list(TIE_STREAMS)
    return list(dict.fromkeys(out))


def _distinct_rows(seqs) -> bool:
    return len({s.tobytes() for s in seqs}) == len(seqs)


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: f"s{s[0]}_k{s[1]}")
def test_bin_counts_take_the_intended_branch(shape):
    states, k = shape
    nbins, vector = SHAPES[shape]
    assert states ** k == nbins
    assert nbins * 8 > LDS_STATE_LIMIT and nbins > 16_384
    assert (nbins % 256 == 0) == vector
    if shape == (5, 7):
        assert nbins % 2 == 1 and nbins % 64 != 0  # (the lane loop ends on a partial pass)
    assert sel_band(nbins) < 0.05 * 4e-7           # (the band is far below FAST_BAND, select_dev.h)
    assert abs(sel_band(65_536) - 9.3e-10) < 1e-11


def test_every_shape_and_every_case_is_there():
    assert {(c.stream.states, c.stream.k) for c in NMOST_CASES} == set(SHAPES)
    assert {(c.stream.states, c.stream.k, c.stat) for c in MAX_CASES} == {(4, 8, "stdev"), (4, 8, "cov"), (5, 7, "stdev"),
                                                                          (5, 7, "cov")}
    for s in _all_streams():
        assert (s.states, s.k) in SHAPES and s.nbins == SHAPES[(s.states, s.k)][0]
        assert 3000 <= s.length <= 6000 and s.nseq <= 400
    assert all(6 <= c.n <= 10 for c in NMOST_CASES)
    assert LARGE_CASE.n > 64 and LARGE_CASE.n * LARGE_CASE.stream.nbins * 8 > 36e6
    from test_distance_truth_host import distance_cases

    by = {c.name: c for c in distance_cases()}
    assert [by[n].nbins for n in WIDE_DISTANCE_CASES] == [65_536, 78_125] and all(by[n].nrows <= 40 for n in WIDE_DISTANCE_CASES)


@pytest.mark.parametrize("stream", _all_streams(), ids=lambda s: f"s{s.states}_k{s.k}_seed{s.seed}")
def test_no_two_rows_are_equal(stream):
    """... so that a device run of these streams has nothing to hand to the tie arbiter"""
    seqs = stream_seqs(stream)
    assert len(seqs) == stream.nseq and all(q.size == stream.length and q.max() < stream.states for q in seqs)
    assert _distinct_rows(seqs)
    rows = {oracle.count_kmers(q, stream.states, stream.k).tobytes() for q in seqs[:40]}
    assert len(rows) == min(40, stream.nseq)  # (distinct as count rows too, not only as sequences)


@pytest.mark.parametrize("case", NMOST_CASES + (LARGE_CASE, FREQS_CASE), ids=lambda c: f"s{c.stream.states}_k{c.stream.k}_n{c.n}")
def test_oracle_nmost_keeps_accepting(case):
    exp, acc = oracle_nmost(case)
    print(f"{case}: {acc} accepts")
    assert exp.size == case.n and acc >= MIN_ACCEPTS
    assert len(set(exp.members()[0].tolist())) == case.n


def test_oracle_nmost_over_an_order_with_repeated_ids():
    seqs, order, exp, acc = order_case()
    assert order.size == len(seqs) + ORDER_REPEATS and np.unique(order).size == len(seqs)
    assert not (order[:len(seqs)] == np.arange(len(seqs))).all()
    assert acc >= MIN_ACCEPTS and len(set(exp.members()[0].tolist())) == ORDER_CASE.n
    # a member among the repeated ids: the label skip has something to skip
    assert set(exp.members()[0].tolist()) & set(order[:ORDER_REPEATS].tolist())


def test_frequency_rows_are_the_oracles_rows():
    rows, exp = freqs_case()
    assert rows.shape == (60, 65_536) and rows.dtype == np.float64
    by_rows = oracle.final_nmost(rows, FREQS_CASE.n)
    assert by_rows.members()[0].tolist() == exp.members()[0].tolist()
    assert by_rows.total_jsd == exp.total_jsd


@pytest.mark.parametrize("case", MAX_CASES, ids=lambda c: f"s{c.stream.states}_k{c.stream.k}_{c.stat}")
def test_oracle_max_grows_beyond_min_size(case):
    exp = oracle_max(case)
    print(f"{case}: size {exp.size}")
    assert case.min_size < exp.size <= case.max_size


@pytest.mark.parametrize("stream", TIE_STREAMS, ids=lambda s: f"s{s.states}_k{s.k}")
def test_tie_case_holds_every_row_twice(stream):
    seqs = tie_seqs(stream)
    assert len(seqs) == 2 * stream.nseq and len({q.tobytes() for q in seqs}) == stream.nseq
    assert all((seqs[2 * i] == seqs[2 * i + 1]).all() for i in range(stream.nseq))
    nm, mx = tie_oracle(stream)
    assert nm.size == TIE_NMOST_N and TIE_MAX[0] < mx.size <= TIE_MAX[1]
    assert tie_copies_of_the_lowest(stream) >= 1


def test_readback_queries():
    qs = readback_queries()
    s = READBACK_CASE.stream
    assert len(qs) == 4 and oracle.count_kmers(qs[-1], s.states, s.k).sum() == 0
    scores = readback_scores()
    print("oracle scores of the read-back queries:", scores)
    assert (oracle.count_kmers(qs[2], s.states, s.k) > 0).all()  # (the longest query misses no bin ...)
    assert np.isfinite(scores[2]) and scores[2] > 0              # (... and is compared by value)
    assert np.isnan(scores[3])
