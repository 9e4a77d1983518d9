"""Farthest-first (max-min) selection on the GPU (csrc/maxmin.hip).  Every result is compared with
tests/test_maxmin_host.py's `maxmin_ref` applied to the matrix of the SQUARE entry for the same input
(matrix_jsd_distances, matrix_euclidean_distances, Sketches.distances) or to the caller's own matrix: picks and owner
equal, radius, dist and cover the same bits, NaN in the same places.  No tolerance appears anywhere."""
import ctypes as C

import numpy as np
import pytest

from diverseseq_amd import _lib, apps, cluster, distance, engine
from test_gpu_linkage import family_seqs
from test_maxmin_host import (BATCHES, BINS, FAMILY_CASE, LARGE, MASH_CASES, MATRIX_SIZES, SIZES, maxmin_ref, same_bits,
                              threshold_plan)

pytestmark = pytest.mark.gpu

_SQUARE = {"jsd": distance.matrix_jsd_distances, "euclidean": distance.matrix_euclidean_distances}


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context()


def _seqs(rng, n, states=4, lo=100, hi=1500, empty=()):
    out = [rng.integers(0, states, size=int(rng.integers(lo, hi)), dtype=np.uint8) for _ in range(n)]
    for e in empty:
        if 0 <= e < n:
            out[e] = np.full(40, states, np.uint8)  # no valid k-mer
    return out


def assert_same(got, d, n_select=None, seeds=(0,), min_distance=None):
    exp = maxmin_ref(d, n_select, seeds, min_distance)
    assert got.picks.dtype == got.owner.dtype == np.int64 and got.radius.dtype == got.dist.dtype == np.float64
    np.testing.assert_array_equal(got.picks, exp.picks)
    np.testing.assert_array_equal(got.owner, exp.owner)
    assert same_bits(got.radius, exp.radius) and same_bits(got.dist, exp.dist) and same_bits(got.cover, exp.cover)
    assert isinstance(got.cover, float)
    return exp


def run_matrix_cases(m, mode, sq):
    """the rules over one count / frequency matrix whose square matrix is sq"""
    n = m.nrows
    assert_same(distance.matrix_maxmin(m, mode=mode, n_select=n), sq, n)  # seed 0
    if n < 3:
        return
    live = [j for j in range(n) if not np.isnan(sq[j, (j + 1) % n]) or not np.isnan(sq[j, (j + 2) % n])]
    s0 = live[0]
    for ns in sorted({1, 2, min(n, 40), n}):  # n_seeds, n_seeds + 1, ..., N: candidates run out before N where rows are out
        assert_same(distance.matrix_maxmin(m, ns, mode=mode, seeds=(s0,)), sq, ns, (s0,))
    seeds = (live[-1], s0, live[len(live) // 2])
    for ns in (3, 4, n):
        assert_same(distance.matrix_maxmin(m, ns, mode=mode, seeds=seeds), sq, ns, seeds)
    full = maxmin_ref(sq, n, (s0,))
    rad = full.radius[1:]
    for t in {0.0, float(rad[len(rad) // 2]), float(rad[0]), float(np.nextafter(rad[0], 0.0)), 2.0 * float(rad[0])}:
        assert_same(distance.matrix_maxmin(m, mode=mode, seeds=(s0,), min_distance=t), sq, None, (s0,), t)
        assert_same(distance.matrix_maxmin(m, min(n, 7), mode=mode, seeds=(s0,), min_distance=t), sq, min(n, 7), (s0,), t)


# ------------------------------------------------------------------ 1. count rows: sizes, bins, element types
@pytest.mark.parametrize("mode", ["jsd", "euclidean"])
@pytest.mark.parametrize("n", SIZES)
def test_count_modes_sizes(ctx, mode, n):
    rng = np.random.default_rng(n)
    seqs = _seqs(rng, n, empty=(0, 3, n - 1) if n > 4 else ())  # a row with no valid k-mer as the seed, inside, last
    if n > 20:
        seqs[11] = seqs[7].copy()  # exact duplicates: ties at 0
        seqs[n - 2] = seqs[7].copy()
    m = ctx.build_matrix(seqs, 3, 4)
    try:
        sq = _SQUARE[mode](m)
        run_matrix_cases(m, mode, sq)
        if n > 20:
            got = distance.matrix_maxmin(m, mode=mode, seeds=(1,), min_distance=0.0)  # keeps one of each duplicate
            assert_same(got, sq, None, (1,), 0.0)
            assert sum(j in got.picks.tolist() for j in (7, 11, n - 2)) == 1 and got.cover == 0.0
    finally:
        m.close()


@pytest.mark.parametrize("mode", ["jsd", "euclidean"])
@pytest.mark.parametrize("u32", [False, True])
@pytest.mark.parametrize("k,states", BINS)
def test_count_modes_bins_and_width(ctx, monkeypatch, mode, u32, k, states):
    if u32:
        monkeypatch.setenv("DVS_COUNTS_U32", "1")
    rng = np.random.default_rng(31 * k + states)
    seqs = _seqs(rng, 130, states, empty=(3,))
    seqs[50] = seqs[2].copy()
    m = ctx.build_matrix(seqs, k, states)
    try:
        assert m.count_bytes == (4 if u32 else 2)
        run_matrix_cases(m, mode, _SQUARE[mode](m))
    finally:
        m.close()


@pytest.mark.parametrize("mode", ["jsd", "euclidean"])
@pytest.mark.parametrize("k", [2, 6])
def test_frequency_rows(ctx, mode, k):
    import oracle

    seqs = _seqs(np.random.default_rng(17 + k), 70)
    f = np.stack([oracle.to_kfreqs(s, 4, k)[0] for s in seqs])
    m = ctx.matrix_from_freqs(f)
    try:
        run_matrix_cases(m, mode, _SQUARE[mode](m))
    finally:
        m.close()


# ------------------------------------------------------------------ 2. a caller's matrix
def _caller_matrices(n, seed):
    rng = np.random.default_rng(seed)
    yield "all_equal", np.full((n, n), 0.5)
    yield "small_integers", rng.integers(0, 4, (n, n)).astype(np.float64)
    yield "asymmetric", rng.random((n, n))
    sym = rng.random((n, n))
    sym = np.triu(sym, 1) + np.triu(sym, 1).T
    yield "symmetric", sym
    inf = sym.copy()
    if n > 2:
        inf[1, :] = inf[:, 1] = np.inf  # an item at +inf from everything
        inf[0, 2] = inf[2, 0] = np.inf
    yield "with_inf", inf
    nan = sym.copy()
    if n > 3:
        nan[2, :] = nan[:, 2] = np.nan
        nan[0, 3] = np.nan  # d(0, 3) only: a row is read as it stands
    yield "with_nan", nan
    yield "negative", sym - 0.5


@pytest.mark.parametrize("n", MATRIX_SIZES)
def test_callers_matrix(ctx, n):
    for label, d in _caller_matrices(n, n):
        keep = d.copy()
        assert_same(cluster.maxmin(d, n, ctx=ctx), d, n)
        assert np.array_equal(d, keep, equal_nan=True), label
        if n < 3:
            continue
        seeds = (n - 1, 0, n // 2)
        for ns in (3, 4, n):
            assert_same(cluster.maxmin(d, ns, seeds=seeds, ctx=ctx), d, ns, seeds)
        for t in (0.0, 0.5, 1.0, -1.0, np.inf):
            assert_same(cluster.maxmin(d, min_distance=t, ctx=ctx), d, None, (0,), t)
            assert_same(cluster.maxmin(d, 5, seeds=(1,), min_distance=t, ctx=ctx), d, 5, (1,), t)
    assert_same(cluster.maxmin([[0, 1, 4], [1, 0, 2], [4, 2, 0]], 2, ctx=ctx), np.array([[0, 1, 4], [1, 0, 2], [4, 2, 0.0]]), 2)


def test_device_tensor_is_only_read(ctx):
    import torch

    d = np.random.default_rng(7).random((513, 513))
    d[5, :] = np.nan
    t = torch.from_numpy(d).to("cuda:0")
    got = cluster.maxmin(t, 100, seeds=(3, 1), ctx=ctx)
    assert_same(got, d, 100, (3, 1))
    host = cluster.maxmin(d, 100, seeds=(3, 1), ctx=ctx)
    assert np.array_equal(got.picks, host.picks) and same_bits(got.dist, host.dist)
    assert np.array_equal(t.cpu().numpy(), d, equal_nan=True)
    with pytest.raises(ValueError, match="square, contiguous float64"):
        cluster.maxmin(t.float(), 3, ctx=ctx)


def test_c_entry_checks_its_arguments(ctx):
    """DVS_ERR_VALUE from the C entry itself, whatever the binding checked"""
    d = np.random.default_rng(1).random((5, 5))
    out = (np.zeros(5, np.uint32), np.zeros(5), C.c_uint32(), np.zeros(5, np.uint32), np.zeros(5), C.c_double())

    def call(seeds, n_select, use_min=0, min_d=0.0):
        s = np.asarray(seeds, dtype=np.uint32)
        given = distance.make_source(_lib.SRC_GIVEN, d.ctypes.data, 5)
        return ctx._L.dvs_maxmin(ctx._h, given, _lib.ptr(s, C.c_uint32), s.size, n_select, use_min,
                                 min_d, _lib.ptr(out[0], C.c_uint32), _lib.ptr(out[1], C.c_double), C.byref(out[2]),
                                 _lib.ptr(out[3], C.c_uint32), _lib.ptr(out[4], C.c_double), C.byref(out[5]))

    assert call([0], 3) == _lib.OK and out[2].value == 3
    for bad in (([], 3), ([5], 3), ([1, 1], 3), ([0, 1], 1), ([0], 6)):
        assert call(*bad) == _lib.ERR_VALUE, bad
    assert call([0], 3, 1, float("nan")) == _lib.ERR_VALUE


# ------------------------------------------------------------------ 3. the stop rules and the batch length
@pytest.fixture(scope="module")
def family(ctx):
    nfam, per, length, seed, k = FAMILY_CASE
    seqs = family_seqs(nfam, per, length, seed)
    m = ctx.build_matrix(list(seqs.values()), k, 4)
    yield m, {mode: _SQUARE[mode](m) for mode in _SQUARE}
    m.close()


@pytest.mark.parametrize("mode", ["jsd", "euclidean"])
@pytest.mark.parametrize("batch", BATCHES)
def test_batch_length_does_not_change_a_bit(ctx, monkeypatch, family, mode, batch):
    m, squares = family
    sq = squares[mode]
    n = m.nrows
    full = maxmin_ref(sq, n)
    plan = threshold_plan(full.radius)
    monkeypatch.setenv("DVS_MAXMIN_BATCH", str(batch))
    assert_same(distance.matrix_maxmin(m, n, mode=mode), sq, n)
    for label, (t, picks) in plan.items():
        got = distance.matrix_maxmin(m, mode=mode, min_distance=t)
        assert_same(got, sq, None, (0,), t)
        assert len(got.picks) == picks, label
    dedup = distance.matrix_maxmin(m, mode=mode, min_distance=0.0)  # one of every group of duplicates
    assert_same(dedup, sq, None, (0,), 0.0)
    assert len(dedup.picks) == n - FAMILY_CASE[0] and dedup.cover == 0.0
    for ns in (6, 7):  # n_select reached at a batch boundary and behind one
        assert_same(distance.matrix_maxmin(m, ns, mode=mode, seeds=(2, 1)), sq, ns, (2, 1))
    d = np.random.default_rng(batch).integers(0, 3, (97, 97)).astype(np.float64)
    assert_same(cluster.maxmin(d, 97, ctx=ctx), d, 97)
    assert_same(cluster.maxmin(d, min_distance=1.0, ctx=ctx), d, None, (0,), 1.0)


def test_the_tile_kernel_on_one_row_gives_the_same_bits(ctx, monkeypatch, family):
    """DVS_MAXMIN_JSD_CROSS: the traversal with jsd_cross_kernel in place of jsd_row_kernel (the A/B of DESIGN.md 4.13)"""
    m, squares = family
    monkeypatch.setenv("DVS_MAXMIN_JSD_CROSS", "1")
    assert_same(distance.matrix_maxmin(m, m.nrows, mode="jsd"), squares["jsd"], m.nrows)
    assert_same(distance.matrix_maxmin(m, mode="jsd", seeds=(5, 2), min_distance=0.0), squares["jsd"], None, (5, 2), 0.0)


def test_diversify_grows_an_nmost_selection(ctx):
    rng = np.random.default_rng(3)
    seqs = _seqs(rng, 300, lo=300, hi=900)
    m = ctx.build_matrix(seqs, 3, 4)
    try:
        sel = m.nmost(8)
        rows = sel.member_rows()
        assert len(set(rows.tolist())) == 8
        for mode in ("jsd", "euclidean"):
            sq = _SQUARE[mode](m)
            got = sel.diversify(20, mode)
            assert got.picks[:8].tolist() == rows.tolist() and np.isnan(got.radius[:8]).all()
            assert_same(got, sq, 20, tuple(rows.tolist()))
            assert_same(sel.diversify(8, mode), sq, 8, tuple(rows.tolist()))
            t = float(got.radius[12])
            assert_same(sel.diversify(None, mode, min_distance=t), sq, None, tuple(rows.tolist()), t)
        sel.close()
    finally:
        m.close()


# ------------------------------------------------------------------ 4. mash
@pytest.mark.parametrize("n,s,canonical", MASH_CASES)
def test_mash(ctx, n, s, canonical):
    k = 9
    # families of mutated copies (members 3 and 10 exact copies of the root): distances all over [0, 1], ties at 0
    seqs = list(family_seqs((n + 11) // 12, 12, 800, 1000 * n + s).values())[:n]
    if n > 4:
        seqs[2] = seqs[2][: k - 1]      # shorter than k: an empty sketch, at 1.0 from everything
        seqs[4] = seqs[4][: k + 20]     # a short sketch
        seqs[n - 1] = seqs[1].copy()    # a duplicate
    sk = distance.Sketches(seqs, k, s, 4, canonical, ctx=ctx)
    try:
        sq = sk.distances()
        got = sk.maxmin(n)
        assert_same(got, sq, n)
        if n > 4:
            assert 2 in got.picks.tolist() and (np.delete(sq[2], 2) == 1.0).all()
            seeds = (2, n - 1, 0)  # the empty sketch as a seed
            for ns in (3, 4, n):
                assert_same(sk.maxmin(ns, seeds=seeds), sq, ns, seeds)
            rad = got.radius[1:]
            for t in (0.0, float(rad[len(rad) // 2]), 1.0):
                assert_same(sk.maxmin(min_distance=t), sq, None, (0,), t)
    finally:
        sk.close()


def test_mash_two_empty_sketches_divide_by_zero(ctx):
    seqs = list(family_seqs(6, 11, 800, 5).values())[:65]
    seqs[2], seqs[40] = seqs[2][:5], seqs[40][:3]
    sk = distance.Sketches(seqs, 9, 50, ctx=ctx)
    try:
        with pytest.raises(ZeroDivisionError):
            sk.distances()
        with pytest.raises(ZeroDivisionError):
            sk.maxmin(65)
        with pytest.raises(ZeroDivisionError):
            sk.maxmin(3, seeds=(2, 40))
        with pytest.raises(ZeroDivisionError):
            distance.maxmin(seqs, 65, "mash", k=9, sketch_size=50, ctx=ctx)
        # a traversal that never visits the pair does not raise: the seed's row alone
        got = sk.maxmin(1)
        assert got.picks.tolist() == [0] and got.dist[2] == got.dist[40] == got.cover == 1.0
    finally:
        sk.close()


# ------------------------------------------------------------------ 5. the sequence-level entries and the app on BRCA1
@pytest.mark.parametrize("mode,kw", [("mash", dict(k=12, sketch_size=400)), ("jsd", dict(k=5)), ("euclidean", dict(k=4))])
def test_brca1(ctx, brca1, mode, kw):
    names = list(brca1)
    seqs = [brca1[n] for n in names]
    sq = distance.MODES[mode][0](seqs, *distance.mode_args(mode, kw["k"], kw.get("sketch_size"), 4, False), ctx=ctx)
    assert_same(distance.maxmin(seqs, 8, mode, ctx=ctx, **kw), sq, 8)
    t = float(maxmin_ref(sq, 12).radius[11])
    exp = assert_same(distance.maxmin(seqs, None, mode, seeds=(3, 1), min_distance=t, ctx=ctx, **kw), sq, None, (3, 1), t)
    app = apps.dvs_maxmin(None, t, mode, seeds=[names[3], names[1]], sketch_size=kw.get("sketch_size", 3000), k=kw["k"])
    out = app(dict(brca1))
    assert out["picks"] == [names[i] for i in exp.picks] and out["picks"][:2] == [names[3], names[1]]
    assert same_bits(out["radius"], exp.radius) and same_bits(out["cover"], exp.cover)
    assert out["representative"] == {n: names[exp.picks[o]] for n, o in zip(names, exp.owner)}
    assert same_bits([out["distance"][n] for n in names], exp.dist)
    out = apps.dvs_maxmin(5, distance_mode=mode, sketch_size=kw.get("sketch_size", 3000), k=kw["k"])(dict(brca1))
    exp = maxmin_ref(sq, 5)
    assert out["picks"] == [names[i] for i in exp.picks] and len(out["radius"]) == 5


# ------------------------------------------------------------------ 6. rows only, never the matrix
@pytest.mark.parametrize("mode", ["jsd", "euclidean"])
def test_large_case_keeps_no_matrix_on_the_device(ctx, monkeypatch, mode):
    import torch

    n, k, ns = LARGE["n"], LARGE["k"], LARGE["n_select"]
    seqs = _seqs(np.random.default_rng(9), n, lo=700, hi=1300, empty=(17,))
    seqs[n - 1] = seqs[5].copy()
    m = ctx.build_matrix(seqs, k, 4)
    try:
        sq = _SQUARE[mode](m)  # (the expectation's matrix: a call of its own)
        monkeypatch.setenv("DVS_CROSS_STRIP_ROWS", "1")
        ctx.sync()
        ctx._L.dvs_ctx_trim(ctx._h)  # (the context's block cache is empty: what the call allocates stays visible)
        free0 = torch.cuda.mem_get_info(0)[0]
        got = distance.matrix_maxmin(m, ns, mode=mode)
        free1 = torch.cuda.mem_get_info(0)[0]
        assert_same(got, sq, ns)
        assert free0 - free1 < n * n * 8 // 8, (free0, free1)  # far below the 200 MB of an n x n matrix
    finally:
        m.close()
