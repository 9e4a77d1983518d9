"""What a finished selection leaves on the device, read back and compared with the oracle.

The selection tests compare which ids are picked, and the members and the summary, which come from the host copy of the
control block and from M / ord / mH / mPos / mLabel / mDelta.  The running sum S, the device copy of the control block
(sum_entropy, lowest, size), the membership table `inset`, and how ord / mH / M fit those are only read by the NEXT
decision -- so after the last one by nothing, except dvs_select_delta_jsd and dvs_select_gather_members.  Every test here
ends in `assert_readback`: query scores of the finished set against the oracle's (src/records.rs:70-84), NaN for NaN
-- the score has no clamp, so its NaN pattern shows the sign of `S - lowest` in every bin a query misses, i.e. the exact
bits of S -- and finite values within TIGHT; labels; the gathered members; the entropy sum; idempotence.

The cases and the conditions that keep them sharp (how many scores are NaN, at which query lengths) are those of
tests/test_readback_host.py, which checks them on the CPU from the oracle alone."""
import numpy as np
import pytest

import oracle
from test_gpu_parity import TIGHT
from test_readback_host import (NO_LABEL, NQ, assert_scores, lowest_member_row, merge_rows, oracle_scores, oracle_set,
                                query_rows, readback_cases)

pytestmark = pytest.mark.gpu

_CASES = readback_cases()
_BY_NAME = {c.name: c for c in _CASES}


@pytest.fixture(scope="module")
def ctx():
    from diverseseq_amd import engine

    return engine.default_context()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _invalid_symbol(case):
    return 4 if case.num_states == 4 else 255


def _count_bytes(case, seqs, u32=False):
    """the width of a count matrix of these sequences: 16 bits where the bins are at most 4096 (and a multiple of four)
    and every sequence is a single tile of at most 32768 windows, 32 bits otherwise or when DVS_COUNTS_U32 asks for it"""
    nbins = case.num_states ** case.k
    fits = nbins <= 4096 and nbins % 4 == 0 and max(s.size for s in seqs) - case.k + 1 <= 32768
    return 2 if fits and not u32 else 4


# ------------------------------------------------------------------------------------------ running a case
def build_set_matrix(ctx, case):
    """-> (matrix, caller labels or None, order or None)"""
    if case.opts.get("set_form") == "freqs":
        rows, ids = merge_rows(case)
        return ctx.matrix_from_freqs(rows), ids, None
    return ctx.build_matrix(case.seqs, case.k, case.num_states), case.opts.get("labels"), case.opts.get("order")


def select(ctx, m, case, labels, order):
    kw = {}
    if labels is not None:
        kw["labels"] = labels
    if order is not None:
        kw["order"] = order
    if case.opts.get("drive") == "stepwise":
        torch = pytest.importorskip("torch")
        from diverseseq_amd import parallel

        assert not kw
        dev = torch.device("cuda", 0)
        _, order1 = parallel.shard_order(m.nrows, case.args[0], 0, 1, block=32)
        if case.mode == "nmost":
            return parallel.nmost_exact(ctx, m, order1, case.args[0], dev, 1, window=256, poll_every=4)
        lo, hi, stat = case.args
        return parallel.max_exact(ctx, m, order1, lo, hi, stat, dev, 1, window=256, poll_every=4)
    if case.mode == "nmost":
        return m.nmost(case.args[0], **kw)
    if case.mode == "max":
        lo, hi, stat = case.args
        return m.max_divergent(lo, hi, stat, **kw)
    return m.as_set(**kw)


def run_case(ctx, case, monkeypatch):
    """the case's matrix and its finished selection, built and run under the case's switches; the switches are taken
    back before anything is read, so that the queries are built the default way (16-bit count rows where they fit)"""
    env = case.opts.get("env", {})
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    try:
        m, labels, order = build_set_matrix(ctx, case)
        if case.opts.get("set_form") != "freqs":
            assert m.count_bytes == _count_bytes(case, case.seqs, bool(env.get("DVS_COUNTS_U32")))
        sel = select(ctx, m, case, labels, order)
    finally:
        for name in env:
            monkeypatch.delenv(name)
    return m, sel


def query_matrix(ctx, case, which):
    """the case's queries of one length as a matrix: from sequences, from a packed batch, or from frequency rows"""
    from diverseseq_amd import engine

    form = case.opts.get("query_form")
    seqs = case.queries[which]
    if form == "freqs":
        q = ctx.matrix_from_freqs(query_rows(case, which)[0])
        assert q.count_bytes == 0
    elif form == "packed":
        data, offsets = engine.concat(seqs)
        q = ctx.build_matrix_packed(ctx.pack_host(data), offsets, case.k)
    else:
        q = ctx.build_matrix(seqs, case.k, case.num_states)
    if form != "freqs":  # (a 60 000 bp query keeps its matrix at 32 bits, whatever the width of the set's)
        assert q.count_bytes == _count_bytes(case, seqs)
    assert q.nrows == NQ
    return q


# ------------------------------------------------------------------------------------------ the read-back
def _gather(ctx, sel, nbins, cap):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    rows = torch.full((max(cap, 1), nbins), -7.0, dtype=torch.float64, device=dev)
    meta = torch.full((max(cap, 1), 2), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    sel.gather_members(rows.data_ptr(), meta.data_ptr(), cap)
    ctx.sync()
    return rows.cpu().numpy()[:cap], meta.cpu().numpy()[:cap]


def snapshot(ctx, sel, qmats):
    """every number the read-back entries return for a selection, as bits (for the same-call-same-bits checks)"""
    s = sel.summary()
    mem = sel.members(with_freqs=True)
    rows, meta = _gather(ctx, sel, sel.matrix.nbins, s.size)
    return {"scores": [_bits(sel.delta_jsd(q)).copy() for q in qmats],
            "summary": (s.size, s.lowest_index, _bits([s.total_jsd, s.mean_delta_jsd, s.std_delta_jsd, s.cov_delta_jsd,
                                                       s.summed_entropies]).tolist()),
            "members": (mem.positions.tolist(), mem.labels.tolist(), _bits(mem.delta_jsd).tolist(),
                        _bits(mem.entropy).tolist(), _bits(mem.kfreqs).copy()),
            "gathered": (_bits(rows).copy(), _bits(meta).copy())}


def assert_same_bits(a, b, what):
    assert a["summary"] == b["summary"], what
    assert a["members"][:4] == b["members"][:4], what
    assert np.array_equal(a["members"][4], b["members"][4]), what
    for x, y in zip(a["scores"], b["scores"]):
        assert np.array_equal(x, y), what
    for x, y in zip(a["gathered"], b["gathered"]):
        assert np.array_equal(x, y), what


def caller_labels(case):
    """the caller's labels of the stream positions (None: the positions themselves)"""
    return merge_rows(case)[1] if case.opts.get("set_form") == "freqs" else case.opts.get("labels")


def assert_readback(ctx, sel, oset, case):
    """The one check every test of this module ends in: device against oracle.  Returns (snapshot, query matrices) for
    the interleaving tests."""
    nbins = sel.matrix.nbins
    labels = caller_labels(case)
    elab, _, _, efreq = oset.members(with_freqs=True)
    size = oset.size
    # ---- the summary: the entropy sum (which _assert_selection does not look at) and the lowest member
    s = sel.summary()
    assert s.size == size and s.lowest_index == oset.lowest_index
    assert abs(s.summed_entropies - oset.summed_entropies) <= TIGHT * max(1.0, abs(oset.summed_entropies))
    if case.opts.get("engine") is not None:
        assert s.engine == case.opts["engine"], (case.name, s.engine)
    if case.opts.get("arbitrated"):
        assert s.n_arbitrated > 0, "no decision went to the arbiter"
    mem = sel.members(with_freqs=True)
    pos = mem.positions.astype(np.int64)
    caller = pos if labels is None else np.asarray(labels)[pos].astype(np.int64)
    assert caller.tolist() == elab.tolist(), "selected ids / member order differ"
    assert (mem.kfreqs == efreq).all()
    # ---- query scores of three lengths, and the lowest member's own row as a query
    worst, nan_counts, qmats = 0.0, [], []
    for which in range(3):
        q = query_matrix(ctx, case, which)
        qmats.append(q)
        exp = oracle_scores(oset, *query_rows(case, which))
        got = sel.delta_jsd(q)
        worst = max(worst, assert_scores(got, exp, f"{case.name}, queries of length index {which}"))
        nan_counts.append(int(np.isnan(exp).sum()))
        assert np.array_equal(_bits(sel.delta_jsd(q)), _bits(got)), "a second delta_jsd returns other bits"
    assert nan_counts[2] == 0
    f, h = lowest_member_row(oset)
    qlow = ctx.matrix_from_freqs(f[None, :])
    worst = max(worst, assert_scores(sel.delta_jsd(qlow), [oset.delta_jsd(f, h)], f"{case.name}, lowest member as query"))
    # ---- labels: a member's label scores exactly 0.0 whatever the row; any other label counts for nothing
    member_labels = set(int(x) for x in elab)
    pool = np.arange(sel.matrix.nrows) if labels is None else np.asarray(labels)
    # (a set of every row of its matrix has no outsider among the rows: the first label behind them is one)
    outsider = next((int(x) for x in pool if int(x) not in member_labels), int(pool.max()) + 1)
    qseqs = list(case.queries[2][:6]) + [np.full(40, _invalid_symbol(case), dtype=np.uint8)]
    qlab = [int(elab[0]), int(elab[oset.lowest_index]), int(elab[-1]), outsider, NO_LABEL, 0xFFFFFFF0, NO_LABEL]
    ql = ctx.build_matrix(qseqs, case.k, case.num_states)
    got = sel.delta_jsd(ql, qlab)
    rows, ents = query_rows(case, 2)
    exp = [oset.delta_jsd(rows[i], ents[i], qlab[i]) for i in range(6)] + [np.nan]
    assert exp[:3] == [0.0, 0.0, 0.0] and not np.isnan(exp[3:6]).any()
    assert (got[:3] == 0.0).all() and not np.signbit(got[:3]).any(), got[:3]
    worst = max(worst, assert_scores(got, exp, f"{case.name}, labelled queries"))
    unl = sel.delta_jsd(ql)  # the same rows without labels: rows 3..5 score what they scored with a label that counts for nothing
    assert np.array_equal(_bits(unl[3:]), _bits(got[3:]))
    assert_scores(unl[:3], [oset.delta_jsd(rows[i], ents[i]) for i in range(3)], f"{case.name}, members' labels dropped")
    # ---- gather_members: set order, bit-equal rows, positions, zero padding; a delta_jsd in between changes nothing
    for cap in (size, size + 3):
        grows, gmeta = _gather(ctx, sel, nbins, cap)
        sel.delta_jsd(qmats[0])
        grows2, gmeta2 = _gather(ctx, sel, nbins, cap)
        assert np.array_equal(_bits(grows), _bits(grows2)) and np.array_equal(_bits(gmeta), _bits(gmeta2))
        assert np.array_equal(_bits(grows[:size]), _bits(efreq)), "gathered rows are not the members' rows"
        gpos = gmeta[:size, 0].astype(np.int64)
        assert (gmeta[:size, 0] == gpos).all() and (gmeta[:size, 1] == 1.0).all()
        gcaller = gpos if labels is None else np.asarray(labels)[gpos].astype(np.int64)
        assert gcaller.tolist() == elab.tolist() and gpos.tolist() == pos.tolist()
        assert not _bits(grows[size:]).any() and not _bits(gmeta[size:]).any(), "padding is not exactly zero"
    with pytest.raises(ValueError, match="buffer of"):
        _gather(ctx, sel, nbins, size - 1)
    # ---- idempotence: the same calls once more give the same bits
    first = snapshot(ctx, sel, qmats)
    assert_same_bits(first, snapshot(ctx, sel, qmats), f"{case.name}: a second read-back differs")
    print(f"{case.name}: engine {s.engine}, size {size}, NaN scores {nan_counts} of {NQ}, "
          f"largest finite difference {worst:.3g}")
    ql.close()
    qlow.close()
    return first, qmats


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("case", _CASES, ids=lambda c: c.name)
def test_readback_of_a_finished_selection(ctx, case, monkeypatch):
    m, sel = run_case(ctx, case, monkeypatch)
    _, qmats = assert_readback(ctx, sel, oracle_set(case), case)
    for q in qmats:
        q.close()
    sel.close()
    m.close()


@pytest.mark.parametrize("first", ["persist", "multi"])
def test_readback_survives_other_selections(ctx, first, monkeypatch):
    """Selection A is read back, selection B runs on the same matrix with another n on the other engine, A is read back
    again: the same bits.  Then B is destroyed and a third selection created -- the context pools device allocations, so
    it re-uses B's -- and A is read back once more.  (The matrix and the context stay alive under their selections.)"""
    case_a = _BY_NAME["k6_n10_persist"]

    def no_persist(on):
        if on:
            monkeypatch.setenv("DVS_NO_PERSIST", "1")
        else:
            monkeypatch.delenv("DVS_NO_PERSIST", raising=False)

    m = ctx.build_matrix(case_a.seqs, case_a.k, case_a.num_states)
    no_persist(first == "multi")
    a = m.nmost(10)
    no_persist(False)
    case_a = case_a._replace(opts={"engine": 1 if first == "persist" else 0})
    snap_a, qmats = assert_readback(ctx, a, oracle_set(case_a), case_a)
    # B: another n, the other engine
    case_b = case_a._replace(name="interleaved_n25", args=(25,), opts={"engine": 0 if first == "persist" else 1})
    no_persist(first == "persist")
    b = m.nmost(25)
    no_persist(False)
    assert_same_bits(snap_a, snapshot(ctx, a, qmats), "A changed when B ran")
    _, qb = assert_readback(ctx, b, oracle_set(case_b), case_b)
    assert_same_bits(snap_a, snapshot(ctx, a, qmats), "A changed when B was read back")
    # B destroyed, C created from the pooled allocations, on either engine
    b.close()
    case_c = case_a._replace(name="interleaved_n7", args=(7,), opts={"engine": 1})
    c = m.nmost(7)
    assert_same_bits(snap_a, snapshot(ctx, a, qmats), "A changed when C took over B's allocations")
    _, qc = assert_readback(ctx, c, oracle_set(case_c), case_c)
    no_persist(True)
    d = m.max_divergent(5, 12, "stdev")
    no_persist(False)
    assert_same_bits(snap_a, snapshot(ctx, a, qmats), "A changed when a `max` selection ran beside it")
    case_d = case_a._replace(name="interleaved_max", mode="max", args=(5, 12, "stdev"), opts={"engine": 0})
    _, qd = assert_readback(ctx, d, oracle_set(case_d), case_d)
    # and A against the oracle again, from scratch
    _, qa = assert_readback(ctx, a, oracle_set(case_a), case_a)
    for q in qmats + qb + qc + qd + qa:
        q.close()
    for sel in (a, c, d):
        sel.close()
    m.close()


def test_delta_jsd_errors_come_before_any_launch(ctx):
    case = _BY_NAME["k5_n10"]
    m = ctx.build_matrix(case.seqs[:200], case.k, 4)
    sel = m.nmost(5)
    other = ctx.build_matrix(case.queries[0][:3], case.k + 1, 4)
    with pytest.raises(ValueError, match="bins"):
        sel.delta_jsd(other)
    empty = ctx.build_matrix([], case.k, 4)
    assert empty.nrows == 0
    got = sel.delta_jsd(empty)
    assert got.shape == (0,) and got.dtype == np.float64
    # the selection is still readable afterwards
    q = ctx.build_matrix(case.queries[2][:4], case.k, 4)
    oset = oracle.nmost(case.seqs[:200], 5, case.k, 4)
    rows, ents = query_rows(case, 2)
    assert_scores(sel.delta_jsd(q), oracle_scores(oset, rows[:4], ents[:4]), "after the refused calls")
    for x in (q, empty, other, sel, m):
        x.close()
