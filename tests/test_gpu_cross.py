"""Distances between two collections and the nearest references on the GPU (csrc/crossdist.hip, csrc/nearest.hip, the cross
instantiation of csrc/mash.hip's pair kernel).  Every comparison is against something other than the code under test:
the square entries (same bits for the same two rows), the long-double yardsticks of tests/test_distance_truth_host.py,
the oracle's sketches and mash distances, the reference's own mash_distance vectors, numpy's stable argsort, the oracle's
selection.  tests/test_cross_host.py pins the cases' preconditions on the CPU."""
import numpy as np
import pytest

import oracle
from conftest import GOLDEN, read_fasta, synth_seqs
from diverseseq_amd import apps, distance, engine
from test_cross_host import (ASSIGN_CASE, BRCA1_JSD_K, BRCA1_REFS, FAMILY_CASES, assign_case, expected_nearest,
                             family_split, oracle_cross_jsd)
from test_distance_truth_host import EUCLID_RTOL, tol_derived, truth_euclid_rows, truth_jsd_rows

pytestmark = pytest.mark.gpu

SIZES = (1, 31, 32, 33, 65, 200)  # on both sides of one 32-row tile and of two, and several tiles
ALL = 4_000_000_000               # the reference's ctree tests' "every k-mer"
MASH_RTOL = 1e-13                 # the project's bound for a mash cell against the oracle (test_mash_distances_matrix)


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context()


def _seqs(rng, n, states=4, lo=100, hi=1500, empty=()):
    out = [rng.integers(0, states, size=int(rng.integers(lo, hi)), dtype=np.uint8) for _ in range(n)]
    for e in empty:
        if e < n:
            out[e] = np.full(40, states, np.uint8)  # no valid k-mer
    return out


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """equal shapes, NaN in the same cells, the same bits everywhere else"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return bool((a[ok].view(np.uint64) == b[ok].view(np.uint64)).all())


def assert_nearest(got, d, kk):
    """(idx, dist) of a nearest call against the stable argsort of the matrix d"""
    idx, val = got
    eidx, eval_ = expected_nearest(d, kk)
    assert idx.dtype == np.int64 and val.dtype == np.float64 and idx.shape == val.shape == (d.shape[0], kk)
    np.testing.assert_array_equal(idx, eidx)
    assert same_bits(val, eval_)
    assert np.array_equal(np.isnan(val), idx < 0)


_SQUARE = {"jsd": distance.matrix_jsd_distances, "euclidean": distance.matrix_euclidean_distances}


# ------------------------------------------------------------------ 1. the same bits as the square path
def _count_case(ctx, mode, m, n, k, states, seed, count_bytes=None):
    """Q (m rows) and R (n rows) as matrices of their own, against the square matrix over the stacked rows; -> the
    cross matrix"""
    rng = np.random.default_rng(seed)
    q = _seqs(rng, m, states, empty=(3,))
    r = _seqs(rng, n, states, empty=(5,))
    if n > 2 and m > 1:
        r[1] = q[0].copy()  # equal counts on the two sides: exactly 0
    mq, mr, ms = (ctx.build_matrix(x, k, states) for x in (q, r, q + r))
    try:
        assert mq.count_bytes == mr.count_bytes == ms.count_bytes
        assert count_bytes is None or mq.count_bytes == count_bytes
        sq = _SQUARE[mode](ms)
        cross = distance.matrix_cross_distances(mq, mr, mode)
        assert cross.shape == (m, n)
        assert same_bits(cross, sq[:m, m:])
        assert same_bits(distance.matrix_cross_distances(mr, mq, mode), sq[m:, :m])
        if n > 2 and m > 1:
            assert cross[0, 1] == 0.0
        # the same through row lists into the stacked matrix: shuffled, repeated
        qr = rng.permutation(m + n)[: max(1, m)]
        rr = np.concatenate([rng.integers(0, m + n, size=n), qr[:1]])
        via = distance.matrix_cross_distances(ms, ms, mode, q_rows=qr, r_rows=rr)
        exp = sq[np.ix_(qr, rr)].copy()
        tot = ms.totals()
        for a, row in enumerate(qr):  # a row against itself: the square matrix has a 0 diagonal, a rectangular one none
            for b, col in enumerate(rr):
                if row == col:
                    assert (via[a, b] == 0.0) if tot[row] else np.isnan(via[a, b])
                    exp[a, b] = via[a, b]
        assert same_bits(via, exp)
        assert via[0, -1] == 0.0 or tot[qr[0]] == 0
        return cross
    finally:
        for x in (mq, mr, ms):
            x.close()


@pytest.mark.parametrize("mode", ["jsd", "euclidean"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("m", SIZES)
def test_count_modes_same_bits_as_square_sizes(ctx, mode, m, n):
    cross = _count_case(ctx, mode, m, n, 3, 4, 1000 * m + n)
    assert np.isnan(cross).sum() == (n if m > 3 else 0) + (m if n > 5 else 0) - (1 if m > 3 and n > 5 else 0)


@pytest.mark.parametrize("mode", ["jsd", "euclidean"])
@pytest.mark.parametrize("u32", [False, True])
@pytest.mark.parametrize("k,states", [(1, 4), (2, 4), (3, 4), (4, 4), (5, 4), (6, 4), (7, 4), (2, 20)])
def test_count_modes_same_bits_as_square_k_and_width(ctx, monkeypatch, mode, u32, k, states):
    if u32:
        monkeypatch.setenv("DVS_COUNTS_U32", "1")
    # (whole-sequence builds leave 16-bit rows up to 4 096 bins only: csrc/kmer_hist.hip dvs_hist_rows_fit_u16)
    _count_case(ctx, mode, 33, 65, k, states, 7 * k + states, count_bytes=4 if u32 or states ** k > 4096 else 2)


@pytest.mark.parametrize("mode", ["jsd", "euclidean"])
def test_frequency_rows_same_bits_as_square(ctx, mode):
    rng = np.random.default_rng(17)
    seqs = _seqs(rng, 70)
    for k in (2, 6):
        f = np.stack([oracle.to_kfreqs(s, 4, k)[0] for s in seqs])
        ms, mq, mr = ctx.matrix_from_freqs(f), ctx.matrix_from_freqs(f[:33]), ctx.matrix_from_freqs(f[33:])
        try:
            sq = _SQUARE[mode](ms)
            assert same_bits(distance.matrix_cross_distances(mq, mr, mode), sq[:33, 33:])
            assert same_bits(distance.matrix_cross_distances(ms, ms, mode, q_rows=[5, 69, 5], r_rows=[0, 40]), sq[np.ix_([5, 69, 5], [0, 40])])
        finally:
            for x in (ms, mq, mr):
                x.close()


@pytest.mark.parametrize("strip", [1, 7, 64])
def test_strip_height_does_not_change_a_bit(ctx, monkeypatch, strip):
    rng = np.random.default_rng(5)
    q, r = _seqs(rng, 200, empty=(3, 150)), _seqs(rng, 65, empty=(5,))
    r[64] = r[2].copy()  # a tie for the nearest lists
    mq, mr = ctx.build_matrix(q, 4, 4), ctx.build_matrix(r, 4, 4)
    sq_, sr_ = _seqs(rng, 200), _seqs(rng, 65)  # (no empty sketches: two of them would divide by zero)
    sr_[64] = sr_[2].copy()
    skq, skr = distance.Sketches(sq_, 8, 50, ctx=ctx), distance.Sketches(sr_, 8, 50, ctx=ctx)
    try:
        whole = {m: distance.matrix_cross_distances(mq, mr, m) for m in ("jsd", "euclidean")}
        near = {m: distance.matrix_nearest(mq, mr, 5, m) for m in ("jsd", "euclidean")}
        whole["mash"], near["mash"] = skq.cross_distances(skr), skq.nearest(skr, 5)
        monkeypatch.setenv("DVS_CROSS_STRIP_ROWS", str(strip))
        for m in ("jsd", "euclidean"):
            assert same_bits(distance.matrix_cross_distances(mq, mr, m), whole[m])
            idx, val = distance.matrix_nearest(mq, mr, 5, m)
            assert np.array_equal(idx, near[m][0]) and same_bits(val, near[m][1])
            assert_nearest((idx, val), whole[m], 5)
        assert same_bits(skq.cross_distances(skr), whole["mash"])
        idx, val = skq.nearest(skr, 5)
        assert np.array_equal(idx, near["mash"][0]) and same_bits(val, near["mash"][1])
        assert_nearest((idx, val), whole["mash"], 5)
    finally:
        for x in (mq, mr, skq, skr):
            x.close()


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("m,n", [(1, 1), (1, 200), (31, 33), (32, 32), (65, 31), (200, 65), (33, 300)])
def test_mash_same_bits_as_square_and_oracle(ctx, m, n, canonical):
    rng = np.random.default_rng(100 * m + n)
    k, s = 9, 120
    q, r = _seqs(rng, m, lo=60, hi=900), _seqs(rng, n, lo=60, hi=900)
    if m > 2:
        q[2] = q[2][: k - 1]  # an empty sketch on the query side only
    if n > 4:
        r[4] = r[4][: k + 20]  # a short sketch
        r[3] = q[0].copy()
    sks = distance.Sketches(q + r, k, s, 4, canonical, ctx=ctx)
    skq, skr = distance.Sketches(q, k, s, 4, canonical, ctx=ctx), distance.Sketches(r, k, s, 4, canonical, ctx=ctx)
    try:
        sq = sks.distances()
        cross = skq.cross_distances(skr)
        assert same_bits(cross, sq[:m, m:])
        assert same_bits(skr.cross_distances(skq), sq[m:, :m])
        rows, cols = rng.permutation(m)[: max(1, m // 2)], rng.integers(0, n, size=n + 3)
        assert same_bits(sks.cross_distances(sks, rows=rows, other_rows=m + cols), sq[np.ix_(rows, m + cols)])
        osk_q = [oracle.mash_sketch(x, k, s, 4, canonical) for x in q]
        osk_r = [oracle.mash_sketch(x, k, s, 4, canonical) for x in r]
        exp = np.array([[oracle.mash_distance(a, b, k, s) for b in osk_r] for a in osk_q])
        np.testing.assert_allclose(cross, exp, rtol=MASH_RTOL, atol=0)
        if n > 4:
            assert cross[0, 3] == 0.0
        if m > 2:
            assert (cross[2] == 1.0).all()  # nothing in common with an empty sketch
        for kk in sorted({1, 3, min(n, 64)} & set(range(1, n + 1))):
            got = skq.nearest(skr, kk)
            assert_nearest(got, cross, kk)
            again = skq.nearest(skr, kk)
            assert np.array_equal(got[0], again[0]) and same_bits(got[1], again[1])
    finally:
        for x in (sks, skq, skr):
            x.close()


def test_mash_every_kmer_sketches(ctx, brca1):
    """sketch_size = 4 000 000 000: every k-mer of either sequence, sketches of different lengths on the two sides"""
    names = list(brca1)
    q, r = [brca1[n] for n in names[:7]], [brca1[n] for n in names[7:20]]
    skq, skr, sks = (distance.Sketches(x, 16, ALL, ctx=ctx) for x in (q, r, q + r))
    try:
        cross = skq.cross_distances(skr)
        assert same_bits(cross, sks.distances()[:7, 7:])
        oq, orr = [oracle.mash_sketch(x, 16, ALL, 4, False) for x in q], [oracle.mash_sketch(x, 16, ALL, 4, False) for x in r]
        exp = np.array([[oracle.mash_distance(a, b, 16, ALL) for b in orr] for a in oq])
        np.testing.assert_allclose(cross, exp, rtol=MASH_RTOL, atol=0)
        assert_nearest(skq.nearest(skr, 13), cross, 13)
    finally:
        for x in (skq, skr, sks):
            x.close()


def test_mash_golden_vectors_one_query_one_reference(ctx, mash_vectors):
    """the reference's own mash_distance (tests/golden/mash_distance_vectors.json), each pair as one query against one
    reference, the sketches uploaded with torch and wrapped where they lie; the bounds of test_mash_distance_golden"""
    import torch

    def wrap(values, k, s):
        a = np.zeros(max(1, len(values)), dtype=np.uint32)
        a[: len(values)] = values
        t = torch.from_numpy(a.view(np.int32).copy()).cuda()
        n = torch.tensor([len(values)], dtype=torch.int32).cuda()
        torch.cuda.synchronize()
        return distance.Sketches.from_device(ctx, t.data_ptr(), n.data_ptr(), 1, a.size, k, s, keep=(t, n))

    for c in mash_vectors["mash_distance"]:
        left, right = wrap(c["left"], c["k"], c["sketch_size"]), wrap(c["right"], c["k"], c["sketch_size"])
        try:
            if c["distance"] == "ZeroDivisionError":
                with pytest.raises(ZeroDivisionError):
                    left.cross_distances(right)
                with pytest.raises(ZeroDivisionError):
                    left.nearest(right, 1)
                continue
            got = left.cross_distances(right)
            assert got.shape == (1, 1)
            assert abs(got[0, 0] - c["distance"]) <= 1e-6 * abs(c["distance"]), c
            assert abs(got[0, 0] - c["distance"]) <= 1e-14 * max(1.0, abs(c["distance"]))
            assert same_bits(right.cross_distances(left), got)
            idx, val = left.nearest(right, 1)
            assert idx.tolist() == [[0]] and same_bits(val, got)
        finally:
            left.close()
            right.close()


# ------------------------------------------------------------------ 2. against the yardsticks
def _truth(mode, rows_q, rows_r):
    """the long-double truth of every cell: rows of one kind on both sides are stacked, a mix is compared through the
    frequencies (f64 quotients for the euclidean mode, as its yardstick defines it)"""
    m, n = len(rows_q), len(rows_r)
    pairs = [(i, m + j) for i in range(m) for j in range(n)]
    fn = truth_jsd_rows if mode == "jsd" else truth_euclid_rows
    return np.asarray(fn(np.concatenate([rows_q, rows_r]), pairs), dtype=np.longdouble).reshape(m, n)


def _assert_close(mode, got, truth, nbins):
    got_ld = got.astype(np.longdouble)
    err = np.abs(got_ld - truth)
    if mode == "jsd":
        print(f"jsd: largest |cell - truth| = {float(err.max()):.3g} (bound {tol_derived(nbins):.3g})")
        assert (err <= tol_derived(nbins)).all()
    else:
        rel = err / np.maximum(np.abs(truth), np.finfo(np.float64).tiny)
        print(f"euclidean: largest relative error = {float(rel[truth > 0].max() if (truth > 0).any() else 0):.3g}")
        assert (err <= EUCLID_RTOL * np.abs(truth)).all()


@pytest.mark.parametrize("mode", ["jsd", "euclidean"])
@pytest.mark.parametrize("k", [2, 6])
def test_count_modes_against_the_truth_all_width_mixes(ctx, monkeypatch, mode, k):
    """uint16 x uint32 x f64 rows in every combination: the mixes have no square twin"""
    rng = np.random.default_rng(31 + k)
    q, r = _seqs(rng, 40, lo=300, hi=2500), _seqs(rng, 70, lo=300, hi=2500)
    r[9] = q[4].copy()
    cq = np.stack([oracle.count_kmers(s, 4, k) for s in q]).astype(np.uint32)
    cr = np.stack([oracle.count_kmers(s, 4, k) for s in r]).astype(np.uint32)
    truth = _truth(mode, cq, cr)
    sides = {}
    sides[2] = (ctx.build_matrix(q, k, 4), ctx.build_matrix(r, k, 4))
    monkeypatch.setenv("DVS_COUNTS_U32", "1")
    sides[4] = (ctx.build_matrix(q, k, 4), ctx.build_matrix(r, k, 4))
    monkeypatch.delenv("DVS_COUNTS_U32")
    fq, fr = (x / x.sum(axis=1, keepdims=True) for x in (cq.astype(np.float64), cr.astype(np.float64)))
    sides[0] = (ctx.matrix_from_freqs(fq), ctx.matrix_from_freqs(fr))
    try:
        for w, (a, b) in sides.items():
            assert a.count_bytes == b.count_bytes == w
        got = {}
        for wq in sides:
            for wr in sides:
                d = distance.matrix_cross_distances(sides[wq][0], sides[wr][1], mode)
                _assert_close(mode, d, truth, 4 ** k)
                if wq and wr:  # equal counts, whatever the two widths: exactly 0
                    assert d[4, 9] == 0.0
                got[wq, wr] = d
        # the count of a row is the same number in 16 and in 32 bits: the same cells whatever the widths
        for key in ((2, 4), (4, 2), (4, 4)):
            assert same_bits(got[key], got[2, 2])
    finally:
        for a, b in sides.values():
            a.close()
            b.close()


# ------------------------------------------------------------------ 3. nearest
@pytest.mark.parametrize("mode", ["jsd", "euclidean"])
@pytest.mark.parametrize("m,n", [(1, 1), (33, 31), (65, 65), (31, 200), (200, 33)])
def test_nearest_is_the_stable_argsort_of_the_cross_matrix(ctx, mode, m, n):
    rng = np.random.default_rng(9 * m + n)
    q, r = _seqs(rng, m, empty=(3,)), _seqs(rng, n, empty=(5,))
    if n > 8:
        r[8] = r[2].copy()  # duplicate references: the lower position first
        r[n - 1] = r[2].copy()
    mq, mr = ctx.build_matrix(q, 3, 4), ctx.build_matrix(r, 3, 4)
    try:
        d = distance.matrix_cross_distances(mq, mr, mode)
        for kk in sorted({1, 3, min(n, 64)} & set(range(1, n + 1))):
            got = distance.matrix_nearest(mq, mr, kk, mode)
            assert_nearest(got, d, kk)
            again = distance.matrix_nearest(mq, mr, kk, mode)
            assert np.array_equal(got[0], again[0]) and same_bits(got[1], again[1])
            if m > 3:  # a query without a valid k-mer: nothing listed
                assert (got[0][3] == -1).all() and np.isnan(got[1][3]).all()
            if n > 5:  # a reference without: never listed
                assert not (got[0] == 5).any()
            if n > 8 and kk >= 3:
                for row_i, row_v in zip(*got):
                    at = {int(j): p for p, j in enumerate(row_i)}
                    if 2 in at and 8 in at:
                        assert at[2] < at[8] and row_v[at[2]] == row_v[at[8]]
        if n < 64:  # fewer finite cells than slots: the tail is -1 / NaN
            idx, val = distance.matrix_nearest(mq, mr, n, mode)
            if n > 5:
                assert (idx[:, -1] == -1).all() and np.isnan(val[:, -1]).all()
    finally:
        mq.close()
        mr.close()


@pytest.mark.parametrize("case", FAMILY_CASES, ids=["k4", "k6"])
def test_nearest_family_case_is_the_oracle_order(ctx, case):
    nfam, per, length, seed, k = case
    ref_names, refs, query_names, queries = family_split(nfam, per, length, seed)
    exp = oracle_cross_jsd(queries, refs, k)
    eidx, eval_ = expected_nearest(exp, 5)
    idx, val = distance.nearest(queries, refs, 5, "jsd", k=k, ctx=ctx)
    np.testing.assert_array_equal(idx, eidx)
    assert (np.abs(val - eval_) <= tol_derived(4 ** k)).all()
    d = distance.cross_distances(queries, refs, "jsd", k=k, ctx=ctx)
    assert (np.abs(d - exp) <= tol_derived(4 ** k)).all()
    assert np.array_equal(d == 0.0, exp == 0.0)
    assert_nearest((idx, val), d, 5)


def test_nearest_errors(ctx):
    rng = np.random.default_rng(2)
    mq, mr, other = ctx.build_matrix(_seqs(rng, 5), 3, 4), ctx.build_matrix(_seqs(rng, 70), 3, 4), ctx.build_matrix(_seqs(rng, 5), 4, 4)
    L, C = ctx._L, __import__("ctypes")
    idx, val = np.zeros((5, 70), np.uint32), np.zeros((5, 70), np.float64)

    def raw(kind, q, r, nq, nr, kk, q_rows=None, r_rows=None):
        from diverseseq_amd import _lib

        return L.dvs_nearest(ctx._h, distance.make_source(kind, q._h, nq, q_rows), distance.make_source(kind, r._h, nr, r_rows),
                             kk, _lib.ptr(idx, C.c_uint32), _lib.ptr(val, C.c_double))

    from diverseseq_amd._lib import ERR_UNSUPPORTED, ERR_VALUE, OK, SRC_EUCLIDEAN, SRC_JSD
    try:
        for entry in (SRC_JSD, SRC_EUCLIDEAN):
            assert raw(entry, mq, mr, 5, 70, 0) == ERR_VALUE       # kk == 0
            assert raw(entry, mq, mr, 5, 10, 11) == ERR_VALUE      # kk > N
            assert raw(entry, mq, mr, 5, 0, 1) == ERR_VALUE        # no references
            assert raw(entry, mq, mr, 5, 70, 65) == ERR_UNSUPPORTED
            assert raw(entry, mq, other, 5, 5, 1) == ERR_VALUE     # unequal nbins
            assert raw(entry, mq, mr, 6, 70, 1) == ERR_VALUE       # more rows than the handle holds
            assert raw(entry, mq, mr, 2, 70, 1, q_rows=np.array([0, 5], np.uint32)) == ERR_VALUE
            assert raw(entry, mq, mr, 5, 2, 1, r_rows=np.array([0, 70], np.uint32)) == ERR_VALUE
            assert raw(entry, mq, mr, 0, 70, 1) == OK
            assert raw(entry, mq, mr, 5, 70, 64) == OK             # the context is usable afterwards
        with pytest.raises(ValueError, match="bins"):
            distance.matrix_cross_distances(mq, other, "jsd")
        with pytest.raises(ValueError):
            distance.matrix_nearest(mq, mr, 71, "jsd")
        with pytest.raises(NotImplementedError):
            distance.matrix_nearest(mq, mr, 65, "jsd")
    finally:
        for x in (mq, mr, other):
            x.close()
    # two empty sketches meet: ZeroDivisionError, from either entry
    short = [np.zeros(3, np.uint8), rng.integers(0, 4, 80, dtype=np.uint8)]
    a, b = distance.Sketches(short, 8, 10, ctx=ctx), distance.Sketches(short[::-1], 8, 10, ctx=ctx)
    try:
        with pytest.raises(ZeroDivisionError):
            a.cross_distances(b)
        with pytest.raises(ZeroDivisionError):
            a.nearest(b, 1)
        assert a.cross_distances(b, rows=[1], other_rows=[0, 0])[0].tolist() == [0.0, 0.0]  # (only visited pairs count)
        assert a.cross_distances(b, rows=[0], other_rows=[0])[0, 0] == 1.0
        a.k = b.k = 0  # (the k of the distance formula: a division by zero before any device work)
        with pytest.raises(ZeroDivisionError):
            a.cross_distances(b, rows=[1], other_rows=[0])
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 4. the top layers
@pytest.mark.parametrize("with_order", [False, True])
def test_selection_assign_is_the_oracle_nearest_member(ctx, with_order):
    k, n = ASSIGN_CASE[3:]
    seqs, order, emembers, erows = assign_case(with_order)  # (members: stream positions; their matrix rows)
    exp = oracle_cross_jsd(seqs, [seqs[i] for i in erows], k)
    m = ctx.build_matrix(seqs, k, 4)
    sel = m.nmost(n) if order is None else m.nmost(n, order=order)
    try:
        assert sel.members(with_freqs=False).positions.tolist() == emembers.tolist()
        assert sel.member_rows().tolist() == [int(x) for x in erows]
        for kk in (1, 3):
            idx, val = sel.assign(kk)
            eidx, eval_ = expected_nearest(exp, kk)
            np.testing.assert_array_equal(idx, eidx)
            assert (np.abs(val - eval_) <= tol_derived(4 ** k)).all()
        idx, val = sel.assign()
        for pos, row in enumerate(erows):
            assert idx[row, 0] == pos and val[row, 0] == 0.0
        eidx, _ = expected_nearest(distance.matrix_cross_distances(m, m, "euclidean", r_rows=sel.member_rows()), 2)
        np.testing.assert_array_equal(sel.assign(2, "euclidean")[0], eidx)
    finally:
        sel.close()
        m.close()


def _brca1_text():
    raw = read_fasta(GOLDEN / "brca1.fasta")
    return {n: s.replace("-", "").replace("?", "") for n, s in raw.items()}


@pytest.mark.parametrize("mode", ["mash", "jsd"])
def test_dvs_nearest_app_on_brca1(brca1, mode):
    text = _brca1_text()
    refs = {n: text[n] for n in BRCA1_REFS}
    queries = {n: text[n] for n in text if n not in BRCA1_REFS}
    queries["Human again"] = text["Human"]  # a query that is itself a reference
    if mode == "mash":
        k, s = 12, 400
        app = apps.dvs_nearest(refs, n_nearest=3, distance_mode="mash", k=k, sketch_size=s)
        sk = {n: oracle.mash_sketch(brca1[n], k, s, 4, False) for n in brca1}
        exp = np.array([[oracle.mash_distance(sk["Human" if q == "Human again" else q], sk[r], k, s) for r in BRCA1_REFS]
                        for q in queries])
        tol = lambda e: MASH_RTOL * abs(e)  # noqa: E731
    else:
        k = BRCA1_JSD_K
        app = apps.dvs_nearest(refs, n_nearest=3, distance_mode="jsd", k=k, sketch_size=None)
        exp = oracle_cross_jsd([brca1["Human" if q == "Human again" else q] for q in queries], [brca1[r] for r in BRCA1_REFS], k)
        tol = lambda e: tol_derived(4 ** k)  # noqa: E731
    got = app(queries)
    assert list(got) == list(queries)
    eidx, eval_ = expected_nearest(exp, 3)
    for i, q in enumerate(queries):
        assert [n for n, _ in got[q]] == [BRCA1_REFS[j] for j in eidx[i]], q
        for (_, d), e in zip(got[q], eval_[i]):
            assert isinstance(d, float) and abs(d - e) <= tol(e)
    assert got["Human again"][0] == ("Human", 0.0)
    assert apps.dvs_nearest(refs, distance_mode=mode, k=k, sketch_size=400 if mode == "mash" else None)({}) == {}


def test_public_functions_over_sequences(ctx):
    """distance.cross_distances / nearest: every mode, the cells of MODES' square function over the stacked sequences"""
    rng = np.random.default_rng(77)
    q, r = _seqs(rng, 9, lo=200, hi=900), _seqs(rng, 40, lo=200, hi=900)
    for mode, kw in (("mash", dict(k=10, sketch_size=200)), ("euclidean", dict(k=4)), ("jsd", dict(k=4))):
        args = distance.mode_args(mode, kw["k"], kw.get("sketch_size"), 4, False)
        sq = distance.MODES[mode][0](q + r, *args)
        d = distance.cross_distances(q, r, mode, ctx=ctx, **kw)
        assert same_bits(d, sq[:9, 9:])
        assert_nearest(distance.nearest(q, r, 4, mode, ctx=ctx, **kw), d, 4)


# ------------------------------------------------------------------ 5. one large case per mode
def _sample_cells(m, n, seed=1, count=2000):
    """seeded cells, with every cell of the first and last tile row and column"""
    rng = np.random.default_rng(seed)
    cells = {(int(i), int(j)) for i, j in zip(rng.integers(0, m, count), rng.integers(0, n, count))}
    last_r, last_c = (m - 1) // 32 * 32, (n - 1) // 32 * 32
    for i in range(m):
        for j in range(n):
            if i < 32 or i >= last_r or j < 32 or j >= last_c:
                cells.add((i, j))
    return sorted(cells)


@pytest.mark.parametrize("mode", ["jsd", "euclidean", "mash"])
def test_cross_baseline_shape(ctx, mode):
    m, n, k = 2000, 300, 6
    q = synth_seqs(m, 2000, 91, invalid_frac=0.001, ragged=True)
    r = synth_seqs(n, 2000, 92, invalid_frac=0.001, ragged=True)
    cells = _sample_cells(m, n)
    assert len(cells) >= 2000
    ii, jj = np.array([c[0] for c in cells]), np.array([c[1] for c in cells])
    if mode == "mash":
        kk, s = 12, 300
        d = distance.cross_distances(q, r, "mash", k=kk, sketch_size=s, ctx=ctx)
        oq = {i: oracle.mash_sketch(q[i], kk, s, 4, False) for i in set(ii.tolist())}
        orr = {j: oracle.mash_sketch(r[j], kk, s, 4, False) for j in set(jj.tolist())}
        exp = np.array([oracle.mash_distance(oq[i], orr[j], kk, s) for i, j in cells])
        np.testing.assert_allclose(d[ii, jj], exp, rtol=MASH_RTOL, atol=0)
        near = distance.nearest(q, r, 16, "mash", k=kk, sketch_size=s, ctx=ctx)
    else:
        d = distance.cross_distances(q, r, mode, k=k, ctx=ctx)
        cq = np.stack([oracle.count_kmers(x, 4, k) for x in q]).astype(np.uint32)
        cr = np.stack([oracle.count_kmers(x, 4, k) for x in r]).astype(np.uint32)
        fn = truth_jsd_rows if mode == "jsd" else truth_euclid_rows
        truth = np.asarray(fn(np.concatenate([cq, cr]), np.stack([ii, m + jj], axis=1)), dtype=np.longdouble)
        _assert_close(mode, d[ii, jj], truth, 4 ** k)
        near = distance.nearest(q, r, 16, mode, k=k, ctx=ctx)
    assert d.shape == (m, n) and not np.isnan(d).any()
    assert_nearest(near, d, 16)
