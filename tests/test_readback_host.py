"""The yardstick of tests/test_gpu_readback.py, pinned on the CPU before it is used on the device.

A finished selection is read back through `delta_jsd` of query rows (src/records.rs:70-84).  That score has no clamp:
where `summed_kfreqs[i] - lowest.kfreqs[i] + query.kfreqs[i]` is negative in one bin -- the lowest member holds the bin
alone, the running sum has drifted an ulp below it and the query misses it -- `log2` gives NaN and so does the score.  The
NaN pattern of a batch of queries therefore shows the exact bits of the running sum, and this module holds

  * `numpy_delta_jsd`: a plain float64 restatement of records.rs:70-84 over the oracle's public state, against the
    oracle's own `delta_jsd` (NaN pattern exact, finite values within TIGHT);
  * `readback_cases()`: the cases the GPU module runs, with the conditions that keep them from hiding a failure -- the
    longest queries of every case are all finite in the oracle, some cases mix NaN and finite scores within one length,
    some sets hold bins with `S - low < 0` and some hold none.
"""
import functools
from typing import NamedTuple

import numpy as np
import pytest

import oracle
from conftest import synth_seqs
from test_gpu_parity import TIGHT, _degenerate_seqs

NQ = 48          # queries of every length
QSEED = 999
NO_LABEL = 0xFFFFFFFF


class Case(NamedTuple):
    name: str
    seqs: list       # the stream (for set_form == "freqs": the sequences the chunk winners are taken from)
    k: int
    num_states: int
    mode: str        # "nmost" | "max" | "set"
    args: tuple      # nmost: (n,); max: (min_size, max_size, stat); set: ()
    queries: tuple   # three lists of NQ sequences, shortest first
    opts: dict       # how the GPU module runs it: env, drive, engine, labels, order, set_form, query_form, arbitrated


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _seqs(nseq, length, seed):
    return synth_seqs(nseq, length, seed, ragged=True)


def _to_states20(seqs):
    """four-state sequences three bases at a time -> sequences over 20 states (every state occurs)"""
    out = []
    for s in seqs:
        t = s[: s.size // 3 * 3].reshape(-1, 3).astype(np.uint32)
        out.append(((t[:, 0] * 16 + t[:, 1] * 4 + t[:, 2]) % 20).astype(np.uint8))
    return out


@functools.lru_cache(maxsize=None)
def _queries(length, num_states=4):
    if num_states == 20:
        return _to_states20(synth_seqs(NQ, 3 * length, QSEED))
    return synth_seqs(NQ, length, QSEED)


@functools.lru_cache(maxsize=None)
def _seqs20(nseq, length, seed):
    return _to_states20(synth_seqs(nseq, 3 * length, seed, ragged=True))


def _case(name, seqs, k, mode, args, lengths, num_states=4, **opts):
    return Case(name, seqs, k, num_states, mode, tuple(args), tuple(_queries(n, num_states) for n in lengths), opts)


@functools.lru_cache(maxsize=None)
def readback_cases():
    """(name, seqs, k, num_states, mode, args, queries, opts) of every case of tests/test_gpu_readback.py.  Engine, mode,
    set size, bin count and count width vary one at a time around three streams:
      s61: 3000 ragged sequences of up to 3000 bp (k = 6; k = 7 uses s62, 1500 of them)
      s70: 3000 ragged sequences of up to 1000 bp (k = 6: the set sizes and the `max` runs)
      s71: 3000 ragged sequences of up to  400 bp (k = 5 and below)"""
    s61, s62, s70, s71 = _seqs(3000, 3000, 61), _seqs(1500, 3000, 62), _seqs(3000, 1000, 70), _seqs(3000, 400, 71)
    L6, L7, L5, L70 = (3000, 12000, 60000), (3000, 60000, 300000), (400, 3000, 20000), (1000, 6000, 60000)
    L3, L2, L20 = (300, 2000, 20000), (200, 1000, 20000), (400, 3000, 40000)
    degen, s71_600, s71_900 = _degenerate_seqs(), s71[:600], s71[:900]
    no_persist = {"DVS_NO_PERSIST": "1"}
    rng = np.random.default_rng(5)
    order = np.concatenate([rng.permutation(600), rng.permutation(600)[:80]]).astype(np.uint32)  # ids repeated later on
    distinct = (np.random.default_rng(1).permutation(3000) * 7 + 3).astype(np.uint32)
    s79 = synth_seqs(600, 800, 79)  # (the selection of test_caller_labels_come_back_from_the_label_free_engine)
    distinct79 = (np.random.default_rng(1).permutation(600) * 7 + 3).astype(np.uint32)
    cases = [
        # ---- engines, around one selection (4096 bins, 10 members)
        _case("k6_n10_persist", s61, 6, "nmost", (10,), L6, engine=1),
        _case("k6_n10_multi", s61, 6, "nmost", (10,), L6, engine=0, env=no_persist),
        _case("k6_n10_fallback", s61, 6, "nmost", (10,), L6, engine=0, env={"DVS_TEST_KNOBS": "fake_persist_error"}),
        _case("k6_n10_stepwise", s61, 6, "nmost", (10,), L6, engine=0, drive="stepwise"),
        _case("k6_n10_u32", s61, 6, "nmost", (10,), L6, engine=1, env={"DVS_COUNTS_U32": "1"}),
        _case("k6_n10_u32_multi", s61, 6, "nmost", (10,), L6, engine=0, env={"DVS_COUNTS_U32": "1", **no_persist}),
        _case("k6_n10_labels_distinct", s61, 6, "nmost", (10,), L6, engine=1, labels=distinct),
        _case("k6_n10_queries_as_freqs", s61, 6, "nmost", (10,), L6, engine=1, query_form="freqs"),
        _case("k6_n10_queries_packed", s61, 6, "nmost", (10,), L6, engine=1, query_form="packed"),
        _case("k5_n9_labels_distinct", s79, 5, "nmost", (9,), L5, engine=1, labels=distinct79),
        # ---- bin counts
        _case("k7_n12", s62, 7, "nmost", (12,), L7, engine=1),
        _case("k7_n12_multi", s62, 7, "nmost", (12,), L7, engine=0, env=no_persist),
        _case("k5_n10", s71, 5, "nmost", (10,), L5, engine=1),
        _case("k3_n10", s71, 3, "nmost", (10,), L3, engine=1),
        _case("k2_n6", s71, 2, "nmost", (6,), L2, engine=1),
        _case("ns20_k2_n8", _seqs20(1500, 600, 72), 2, "nmost", (8,), L20, num_states=20, engine=1),
        # ---- set sizes (s70, 4096 bins)
        _case("k6_n2", s70, 6, "nmost", (2,), L70, engine=1),
        _case("k6_n63", s70, 6, "nmost", (63,), L70, engine=1),
        _case("k6_n64", s70, 6, "nmost", (64,), L70, engine=1),
        _case("k6_n65", s70, 6, "nmost", (65,), L70, engine=1),
        _case("k6_n100", s70, 6, "nmost", (100,), L70, engine=1),
        _case("k6_n100_multi", s70, 6, "nmost", (100,), L70, engine=0, env=no_persist),
        # ---- `max`: the run ends on a tentative push taken back (stdev at 9, cov at 60), or at max_size
        _case("k6_max_stdev", s70, 6, "max", (5, 60, "stdev"), L70, engine=1),
        _case("k6_max_cov", s70, 6, "max", (5, 60, "cov"), L70, engine=1),
        _case("k6_max_full", s70, 6, "max", (5, 8, "stdev"), L70, engine=1),
        _case("k6_max_stdev_multi", s70, 6, "max", (5, 60, "stdev"), L70, engine=0, env=no_persist),
        _case("k6_max_full_multi", s70, 6, "max", (5, 8, "stdev"), L70, engine=0, env=no_persist),
        _case("k6_max_full_fallback", s70, 6, "max", (5, 8, "stdev"), L70, engine=0,
              env={"DVS_TEST_KNOBS": "fake_persist_error"}),
        _case("k6_max_cov_stepwise", s70, 6, "max", (5, 60, "cov"), L70, engine=0, drive="stepwise"),
        # ---- a set that never ran a selection
        _case("k6_set12", s61[:12], 6, "set", (), L6, engine=0),
        # ---- decisions at the edge
        _case("degenerate_k3_n7", degen, 3, "nmost", (7,), L3, engine=1, arbitrated=True),
        _case("degenerate_k3_n7_stepwise", degen, 3, "nmost", (7,), L3, engine=0, drive="stepwise",
              arbitrated=True),
        _case("k5_order_repeats_ids", s71_600, 5, "nmost", (9,), L5, engine=0, order=order, labels=order),
        # ---- the chunk merge: a frequency matrix as the set's matrix
        _case("k5_merge_freqs", s71_900, 5, "nmost", (8,), L5, engine=1, set_form="freqs"),
        _case("k5_merge_freqs_multi", s71_900, 5, "nmost", (8,), L5, engine=0, set_form="freqs", env=no_persist),
    ]
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def merge_rows(case):
    """set_form == "freqs": the winners' frequency rows of three chunks of the stream and their global ids (records.py:225-245)"""
    n, rows, ids = case.args[0], [], []
    third = len(case.seqs) // 3
    for c in range(3):
        lab, _, _, f = oracle.nmost(case.seqs[c * third:(c + 1) * third], n, case.k, case.num_states).members(with_freqs=True)
        rows.append(f)
        ids.append(lab.astype(np.uint32) + np.uint32(c * third))
    return np.vstack(rows), np.concatenate(ids)


def stream_of(case):
    """the sequences in stream order and the caller's labels (None: the stream position)"""
    order, labels = case.opts.get("order"), case.opts.get("labels")
    seqs = case.seqs if order is None else [case.seqs[int(i)] for i in order]
    return seqs, labels


_oracle_sets = {}


def _set_key(case):
    return (id(case.seqs), len(case.seqs), case.k, case.num_states, case.mode, case.args, case.opts.get("set_form"),
            id(case.opts.get("order")), id(case.opts.get("labels")))


def oracle_set(case):
    """the oracle's finished set of a case (one per distinct selection: engines and widths do not change it)"""
    key = _set_key(case)
    if key not in _oracle_sets:
        seqs, labels = stream_of(case)
        if case.opts.get("set_form") == "freqs":
            rows, ids = merge_rows(case)
            oset = oracle.final_nmost(rows, case.args[0], labels=ids)
        elif case.mode == "nmost":
            oset = oracle.nmost(seqs, case.args[0], case.k, case.num_states, labels=labels)
        elif case.mode == "max":
            lo, hi, stat = case.args
            oset = oracle.max_divergent(seqs, lo, hi, case.k, case.num_states, stat, labels=labels)
        else:
            oset = oracle.SummedRecords.from_seqs(seqs, case.k, case.num_states)
        _oracle_sets[key] = oset
    return _oracle_sets[key]


_query_rows = {}


def query_rows(case, which):
    """(frequency rows [NQ, bins], entropies [NQ]) of the case's queries of length index `which`, by the oracle"""
    key = (id(case.queries[which]), case.k, case.num_states)
    if key not in _query_rows:
        fh = [oracle.to_kfreqs(q, case.num_states, case.k) for q in case.queries[which]]
        _query_rows[key] = (np.stack([f for f, _ in fh]), np.array([h for _, h in fh]))
    return _query_rows[key]


def oracle_scores(oset, rows, ents):
    """the oracle's delta_jsd of unlabelled query rows"""
    return np.array([oset.delta_jsd(f, h) for f, h in zip(rows, ents)])


def lowest_member_row(oset):
    """the lowest member's own row and entropy: as a query (without its label) it restores `S` exactly in the bins that
    member holds alone, so whether it scores NaN is decided by the other drifted bins only"""
    _, _, ents, rows = oset.members(with_freqs=True)
    low = oset.lowest_index
    return rows[low].copy(), float(ents[low])


def negative_bins(oset):
    """bins of the finished set in which the running sum lies below the lowest member's own frequency"""
    rows = oset.members(with_freqs=True)[3]
    return int(((oset.summed_kfreqs - rows[oset.lowest_index]) < 0).sum())


# ------------------------------------------------------------------------------------- the numpy restatement
def numpy_delta_jsd(oset, f, h):
    """src/records.rs:70-84 for a query without a label, in numpy float64 over the public state of an
    oracle.SummedRecords: elementwise IEEE arithmetic, then entropy() (record.rs:86-106) as a sequential sum in bin order
    over the non-zero bins.  log2 of a negative mean is NaN, and the NaN stays."""
    S = oset.summed_kfreqs
    _, _, ents, rows = oset.members(with_freqs=True)
    low = oset.lowest_index
    size = float(oset.size)
    mean_entropy = (oset.summed_entropies - ents[low] + h) / size
    mean = (S - rows[low] + np.asarray(f, dtype=np.float64)) / size
    nz = mean[mean != 0.0]
    with np.errstate(invalid="ignore"):
        terms = -nz * np.log2(nz)
    total = np.add.accumulate(nz)[-1]
    assert np.isnan(total) or abs(total - 1.0) <= mean.size * np.finfo(np.float64).eps  # (record.rs:99-104 would panic)
    return float(np.add.accumulate(terms)[-1]) - mean_entropy


def assert_scores(got, exp, what=""):
    """NaN pattern equal element for element, finite values within TIGHT of max(1, |expected|); returns the largest
    finite difference"""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    gn, en = np.isnan(got), np.isnan(exp)
    assert (gn == en).all(), f"{what}: NaN pattern differs at {np.flatnonzero(gn != en).tolist()} " \
                             f"(got {int(gn.sum())} NaN, expected {int(en.sum())})"
    fin = ~en
    if not fin.any():
        return 0.0
    diff = np.abs(got[fin] - exp[fin])
    bound = TIGHT * np.maximum(1.0, np.abs(exp[fin]))
    worst = int(np.argmax(diff - bound))
    assert (diff <= bound).all(), (what, got[fin][worst], exp[fin][worst], diff[worst])
    return float(diff.max())


# ------------------------------------------------------------------------------------------------ the tests
_CASES = readback_cases()
# one case per distinct selection is enough on the CPU (the others differ in how the device runs them)
_DISTINCT = list({_set_key(c): c for c in reversed(_CASES)}.values())[::-1]


@pytest.mark.parametrize("case", _DISTINCT, ids=lambda c: c.name)
def test_numpy_restatement_is_the_oracle(case):
    """every query of every length, and the lowest member's own row: NaN pattern exact, values within TIGHT"""
    oset = oracle_set(case)
    worst = 0.0
    for which in range(3):
        rows, ents = query_rows(case, which)
        exp = oracle_scores(oset, rows, ents)
        got = [numpy_delta_jsd(oset, f, h) for f, h in zip(rows, ents)]
        worst = max(worst, assert_scores(got, exp, f"{case.name}, length {which}"))
    f, h = lowest_member_row(oset)
    worst = max(worst, assert_scores([numpy_delta_jsd(oset, f, h)], [oset.delta_jsd(f, h)], f"{case.name}, lowest member"))
    print(f"{case.name}: numpy - oracle, largest finite difference {worst:.3g}")


def test_lowest_member_as_query_restores_its_own_bins():
    """With the lowest member's own row as the query (no label) every bin's mean is `(S - low + low) / size`: S itself
    wherever the subtraction was exact, the member's bins held alone among them.  The score is NaN iff some other bin
    still ends below zero, in the oracle and in the numpy restatement; with the member's label it is 0.0."""
    seen = set()
    for case in _DISTINCT:
        oset = oracle_set(case)
        f, h = lowest_member_row(oset)
        S = oset.summed_kfreqs
        still_negative = bool((((S - f) + f) < 0).any())
        got = oset.delta_jsd(f, h)
        assert np.isnan(got) == still_negative, case.name
        assert np.isnan(numpy_delta_jsd(oset, f, h)) == still_negative, case.name
        # its own label makes it a member: 0.0, whatever the row
        labs = oset.members()[0]
        assert oset.delta_jsd(f, h, int(labs[oset.lowest_index])) == 0.0
        seen.add(still_negative)
    assert False in seen  # (the kind that is compared by value occurs)


@pytest.mark.parametrize("case", _CASES, ids=lambda c: c.name)
def test_longest_queries_are_all_finite(case):
    """condition 1: the longest of a case's three query lengths gives no NaN in the oracle, so at least a third of the
    unlabelled queries of every case are compared by value"""
    assert len(case.queries) == 3 and all(len(q) == NQ for q in case.queries)
    rows, ents = query_rows(case, 2)
    assert not np.isnan(oracle_scores(oracle_set(case), rows, ents)).any()


def test_cases_mix_nan_and_finite_scores():
    """condition 2: at least three cases hold NaN and finite oracle scores among queries of ONE length; at least four
    sets hold a bin with S - low < 0 and at least four hold none"""
    mixed, negative, clean = set(), set(), set()
    for case in _DISTINCT:
        oset = oracle_set(case)
        for which in range(3):
            rows, ents = query_rows(case, which)
            nn = int(np.isnan(oracle_scores(oset, rows, ents)).sum())
            if 0 < nn < NQ:
                mixed.add(case.name)
        (negative if negative_bins(oset) else clean).add(case.name)
    print("mixed:", sorted(mixed), "\nS - low < 0 in some bin:", sorted(negative), "\nin none:", sorted(clean))
    assert len(mixed) >= 3 and len(negative) >= 4 and len(clean) >= 4


def test_measured_sets_of_the_case_table():
    """the sets the module was designed around: their counts of bins with S - low < 0 and of NaN scores per length"""
    by_name = {c.name: c for c in _CASES}
    table = {"k6_n10_persist": (11, (48, 16, 0)), "k7_n12": (13, (48, 14, 0)), "k5_n10": (11, (48, 25, 0)),
             "k6_n2": (74, (48, 48, 0)), "k6_n63": (0, (0, 0, 0)), "k6_n64": (0, (0, 0, 0)), "k6_n65": (0, (0, 0, 0)),
             "k6_n100": (0, (0, 0, 0)), "k6_max_stdev": (0, (0, 0, 0)), "k6_max_cov": (0, (0, 0, 0)),
             "k6_max_full": (12, (48, 47, 0))}
    sizes = {"k6_max_stdev": 9, "k6_max_cov": 60, "k6_max_full": 8}
    for name, (nneg, nans) in table.items():
        case = by_name[name]
        oset = oracle_set(case)
        assert negative_bins(oset) == nneg, name
        got = tuple(int(np.isnan(oracle_scores(oset, *query_rows(case, w))).sum()) for w in range(3))
        assert got == nans, (name, got)
        if name in sizes:
            assert oset.size == sizes[name], (name, oset.size)


def test_case_matrix_is_complete():
    """every item the read-back is asked over appears at least once"""
    cs = _CASES
    envs = [c.opts.get("env", {}) for c in cs]
    assert any(e.get("DVS_NO_PERSIST") for e in envs) and any(e.get("DVS_COUNTS_U32") for e in envs)
    assert any(e.get("DVS_TEST_KNOBS") == "fake_persist_error" for e in envs)
    assert {c.mode for c in cs if c.opts.get("drive") == "stepwise"} == {"nmost", "max"}
    assert {c.args[2] for c in cs if c.mode == "max"} == {"stdev", "cov"} and any(c.mode == "set" for c in cs)
    assert {2, 10, 63, 64, 65, 100} <= {c.args[0] for c in cs if c.mode == "nmost"}
    assert {16, 64, 1024, 4096, 16384, 400} <= {c.num_states ** c.k for c in cs}
    assert {c.opts.get("query_form") for c in cs} >= {"freqs", "packed"}
    assert any(c.opts.get("set_form") == "freqs" for c in cs) and any(c.opts.get("arbitrated") for c in cs)
    order = next(c.opts["order"] for c in cs if c.opts.get("order") is not None)
    assert np.unique(order).size < order.size
    lab = next(c.opts["labels"] for c in cs if c.opts.get("labels") is not None and c.opts.get("order") is None)
    assert np.unique(lab).size == lab.size and not (lab == np.arange(lab.size)).all()
    # a 60 000 bp query has more windows than a 16-bit count holds: its matrix is 32 bits wide whatever the set's
    assert any(min(q.size for q in c.queries[2]) - c.k + 1 > 32768 for c in cs)
