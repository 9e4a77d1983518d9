"""The Mantel test on the GPU (csrc/mantel.hip) against the yardstick of tests/mantel_cases.py, whose own pinning and the
conditions of every case here are in test_mantel_host.py.  Exact families as arrays through the raw C call; real-valued
input within (n + 8) 2^-52 of the long-double truth, r within four times that of Pearson's r, with the yardstick's
counts and p; only the cells above the diagonal read, of X and of Y, and a device tensor left as it was; every pair of
the three modes fused against the route through two host matrices; every batch length, poisoned blocks and a second
run; every block request refused in turn; every error of the C boundary;
the Python layer and the app.

Measured on an MI355X: the worst |device - truth| / band over every sum of the nine real-valued cases is 0.038
(uniform-n40-P99; 0.0013 to 0.021 in the others), the worst |r - Pearson's r| / (4 band) 0.0028;
test_real_valued_input_within_the_band prints each case's."""
import ctypes as C
import gc

import numpy as np
import pytest

from diverseseq_amd import _lib, distance, engine, mantel
import mantel_cases as mc
from test_blocks_host import POISON, REFUSE
from test_gpu_linkage import family_seqs

pytestmark = pytest.mark.gpu

u32p, f64p = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
MODE_ARGS = {"mash": {"distance_mode": "mash", "k": 10, "sketch_size": 500}, "euclidean": {"distance_mode": "euclidean", "k": 5},
             "jsd": {"distance_mode": "jsd", "k": 5}}


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context()


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_result(a, b) -> bool:
    """two Mantel (or lists of values), every field bit for bit"""
    return len(a) == len(b) and all(same_bits(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def given(D, n=None, on_device=0, rows=None):
    D = np.ascontiguousarray(D, dtype=np.float64)
    return distance.make_source(_lib.SRC_GIVEN, D.ctypes.data, D.shape[0] if n is None else n, rows, on_device=on_device, keep=D)


def on_device(t):
    return distance.make_source(_lib.SRC_GIVEN, t.data_ptr(), int(t.shape[0]), on_device=1, keep=t)


def raw_call(ctx, sx, sy, perms, *, info=True, moments=True, z=True):
    """dvs_mantel itself -> (rc, moments, z, info); the outputs NULL on demand"""
    perms = None if perms is None else np.ascontiguousarray(perms, dtype=np.uint32)
    P = 0 if perms is None else perms.shape[0]
    mom, zz, inf = np.full(6, -7.0), np.full(P + 1, -7.0), _lib.MantelInfo(99, 99, 99, 99, 99)
    rc = ctx._L.dvs_mantel(ctx._h, sx, sy, perms.ctypes.data_as(u32p) if P else None, P,
                           mom.ctypes.data_as(f64p) if moments else None, zz.ctypes.data_as(f64p) if z else None,
                           C.byref(inf) if info else None)
    return rc, mom, zz, inf


def run_case(ctx, case):
    X, Y = mc.case_matrices(case)
    return raw_call(ctx, given(X), given(Y), mc.case_perms(case))


def assert_is_yardstick(out, case, label=""):
    rc, mom, z, inf = out
    s, st = mc.case_sums(case), mc.case_stats(case)
    assert rc == _lib.OK, (label, case.id)
    assert np.array_equal(mom, s.moments) and np.array_equal(z, s.z), (label, case.id, mom, s.moments)
    assert (inf.n_ge, inf.n_le, inf.n_abs_ge) == (st.n_ge, st.n_le, st.n_abs_ge), (label, case.id)


def exact(case_id):
    return next(c for c in mc.EXACT_CASES if c.id == case_id)


# ---- exact families, as arrays

@pytest.mark.parametrize("case", mc.EXACT_CASES, ids=lambda c: c.id)
def test_exact_families_as_arrays(ctx, case):
    out = run_case(ctx, case)
    assert_is_yardstick(out, case)
    B = mc.DEFAULT_BATCH
    assert (out[3].passes, out[3].batch) == (2 + -(-(case.P + 1) // B), B)
    if case.n <= 300:  # the Python layer derives the rest as the yardstick does
        X, Y = mc.case_matrices(case)
        st = mc.case_stats(case)
        got = mantel.mantel(X, Y, permutations=0, ctx=ctx)
        assert same_bits(np.float64(got.r), st.r[0]) and np.isnan(got.p_value) and got.r_permuted.size == 0
        assert (got.n, got.permutations, got.alternative) == (case.n, 0, "two-sided")


def test_optional_info(ctx):
    case = exact("plain-n257-P33")
    X, Y = mc.case_matrices(case)
    rc, mom, z, inf = raw_call(ctx, given(X), given(Y), mc.case_perms(case), info=False)
    assert rc == _lib.OK and np.array_equal(mom, mc.case_sums(case).moments) and np.array_equal(z, mc.case_sums(case).z)
    assert (inf.n_ge, inf.passes, inf.batch) == (99, 99, 99)


# ---- real-valued input

WORST = {}


@pytest.mark.parametrize("case", mc.REAL_CASES, ids=lambda c: c.id)
def test_real_valued_input_within_the_band(ctx, case):
    """every sum within (n + 8) 2^-52 of the long-double truth over the device's own u and v, relative to the sum of its
    terms' magnitudes, r within four times that of Pearson's r of the cells; measured on an MI355X, the worst ratio of
    all nine cases is 0.038 for the sums and 0.0028 for r"""
    X, Y = mc.case_matrices(case)
    perms = mc.case_perms(case)
    n, m = case.n, mc.pairs_of(case.n)
    rc, mom, z, inf = raw_call(ctx, given(X), given(Y), perms)
    assert rc == _lib.OK
    ld, band = np.longdouble, mc.band(n)
    shifts = (mom[0], mom[1])
    for s, M in zip(shifts, (X, Y)):  # the shifts: the mean of the cells, within the band
        mean = mc.upper_cells(M).astype(ld).sum() / ld(m)
        assert abs(ld(s) - mean) <= band * mean
    truth, mag = mc.sums(X, Y, perms, ld, shifts=shifts), mc.magnitudes(X, Y, perms, shifts)
    ratios = [abs(ld(mom[2 + k]) - getattr(truth, name)) / (band * getattr(mag, name))
              for k, name in enumerate(("A", "B", "S_uu", "S_vv"))]
    ratios += list(np.abs(z.astype(ld) - truth.z) / (band * mag.z))
    r = mantel.mantel_statistics(n, mom, z)
    r_ratio = float(abs(ld(r[0]) - mc.pearson_truth(X, Y)) / (4 * band))
    WORST[case.id] = float(max(ratios))
    print(case.id, "worst |device - truth| / band:", WORST[case.id], "of all so far:", max(WORST.values()),
          "|r - Pearson's r| / (4 band):", r_ratio)
    assert max(ratios) <= 1.0, (case.id, float(max(ratios)))
    assert r_ratio <= 1.0, (case.id, r_ratio)
    st = mc.case_stats(case)
    assert (inf.n_ge, inf.n_le, inf.n_abs_ge) == (st.n_ge, st.n_le, st.n_abs_ge)
    for alt in mc.ALTERNATIVES:
        got = mantel.mantel(X, Y, permutations=case.P, seed=case.seed + 2, alternative=alt, ctx=ctx)
        assert got.p_value == st.p_value[alt] and got.alternative == alt and same_bits(got.z, z)
        assert abs(got.r - st.r[0]) <= 4 * band and same_bits(got.r_permuted, r[1:])


# ---- only the cells above the diagonal are read; a device tensor stays as it was

def test_only_the_upper_triangle_is_read_and_device_tensors_stay(ctx):
    import torch

    case = next(c for c in mc.REAL_CASES if c.n == 300 and c.family == "points")
    X, Y = (np.array(M) for M in mc.case_matrices(case))
    perms = mc.case_perms(case)
    want = raw_call(ctx, given(X), given(Y), perms)
    assert want[0] == _lib.OK
    n = case.n
    low = np.tril_indices(n)

    def variant(M, fill):
        out = M.copy()
        out[low] = fill if np.isscalar(fill) else fill[low]
        return out

    fills = (0.0, -1.0, np.inf, np.random.default_rng(3).random((n, n)))
    for fx in fills:
        for fy in fills[:3] if fx is not fills[3] else fills:
            got = raw_call(ctx, given(variant(X, fx)), given(variant(Y, fy)), perms)
            assert got[0] == _lib.OK and same_bits(got[1], want[1]) and same_bits(got[2], want[2])
    tx, ty = torch.from_numpy(X).to("cuda:0"), torch.from_numpy(Y).to("cuda:0")
    torch.cuda.synchronize()
    for sx, sy in ((on_device(tx), on_device(ty)), (given(X), on_device(ty)), (on_device(tx), given(Y)), (on_device(ty), on_device(ty))):
        got = raw_call(ctx, sx, sy, perms)
        assert got[0] == _lib.OK
        if sx.handle != sy.handle:
            assert same_bits(got[1], want[1]) and same_bits(got[2], want[2])
        assert same_bits(tx.cpu().numpy(), X) and same_bits(ty.cpu().numpy(), Y)  # NaN diagonal and lower triangle and all
    host = mantel.mantel(X, Y, permutations=20, seed=1, ctx=ctx)
    assert same_result(mantel.mantel(tx, ty, permutations=20, seed=1, ctx=ctx), host)
    assert same_bits(ty.cpu().numpy(), Y)
    with pytest.raises(ValueError):
        mantel.mantel(torch.zeros((4, 5), dtype=torch.float64, device="cuda:0"), ty, ctx=ctx)
    with pytest.raises(ValueError):
        mantel.mantel(tx, torch.zeros((n, n), dtype=torch.float32, device="cuda:0"), ctx=ctx)


# ---- sources

@pytest.fixture(scope="module")
def brca1_arrays(brca1):
    return [brca1[name] for name in brca1]


@pytest.fixture(scope="module")
def brca1_matrices(ctx, brca1_arrays):
    out = {}
    for mode, args in MODE_ARGS.items():
        pos = (args["k"], args["sketch_size"]) if mode == "mash" else (args["k"],)
        out[mode] = distance.MODES[mode][0](brca1_arrays, *pos, ctx=ctx)
    return out


@pytest.mark.parametrize("pair", [("mash", "jsd"), ("jsd", "mash"), ("mash", "euclidean"), ("euclidean", "jsd"),
                                  ("jsd", "euclidean"), ("euclidean", "mash")], ids="-".join)
def test_brca1_fused_equals_the_route_through_two_host_matrices(ctx, brca1_arrays, brca1_matrices, pair):
    import torch

    kw = dict(permutations=37, seed=4)
    mx, my = pair
    fused = mantel.of_sequences(brca1_arrays, MODE_ARGS[mx], MODE_ARGS[my], ctx=ctx, **kw)
    route = mantel.mantel(brca1_matrices[mx], brca1_matrices[my], ctx=ctx, **kw)
    assert same_result(fused, route), pair
    assert fused.n == len(brca1_arrays) and fused.r_permuted.shape == (37,) and 0 < fused.p_value <= 1 and 0 < fused.r < 1
    args = distance.mode_args(mx, MODE_ARGS[mx]["k"], MODE_ARGS[mx].get("sketch_size"), 4, False)
    with distance.device_side(brca1_arrays, mx, *args, ctx=ctx) as side:
        assert same_result(mantel.mantel(side, brca1_matrices[my], **kw), fused)            # a side against a host matrix
        t = torch.from_numpy(np.ascontiguousarray(brca1_matrices[my])).to("cuda:0")
        assert same_result(mantel.mantel(side, t, **kw), fused)                             # ... against a device tensor
        assert same_bits(t.cpu().numpy(), brca1_matrices[my])
        swapped = mantel.mantel(brca1_matrices[my], side, **kw)                             # ... and as the second side
        assert abs(swapped.r - fused.r) <= 8 * mc.band(fused.n)  # (each within 2 band (1 + |r|) of Pearson's r)


# ---- the schedule changes no bit

def _schedule_case(c):
    out = []
    for case in (next(x for x in mc.REAL_CASES if x.n == 300 and x.family == "crowded"),
                 next(x for x in mc.REAL_CASES if x.n == 1025 and x.family == "uniform"),
                 exact("plain-n257-P101"), exact("identity-n65-P33"), exact("plain-n256-P0")):
        got = run_case(c, case)
        st = mc.case_stats(case)
        assert got[0] == _lib.OK and (got[3].n_ge, got[3].n_le, got[3].n_abs_ge) == (st.n_ge, st.n_le, st.n_abs_ge)
        out += [got[1], got[2]]
    seqs = family_seqs(5, 8, 1500, seed=21)
    arrays = [seqs[s] for s in seqs]
    out += list(mantel.of_sequences(arrays, {"distance_mode": "jsd", "k": 4}, {"distance_mode": "mash", "k": 8, "sketch_size": 200},
                                    permutations=20, seed=3, ctx=c))[:-1]
    out.append(distance.jsd_kmedoids(arrays, 4, n_medoids=5, ctx=c).td)  # another operation in between
    with pytest.raises(ValueError, match="negative"):  # a failing call, then the same context again
        mantel.mantel(np.ones((9, 9)), -np.ones((9, 9)), ctx=c)
    out += list(mantel.of_sequences(arrays, {"distance_mode": "euclidean", "k": 4}, {"distance_mode": "jsd", "k": 4},
                                    permutations=20, seed=3, ctx=c))[:-1]
    return out


def _fresh(runs: int) -> list:
    c = engine.Context(0)
    try:
        c.refresh_knobs()
        return [_schedule_case(c) for _ in range(runs)]
    finally:
        c.close()


@pytest.fixture(scope="module")
def schedule_clean():
    return _fresh(1)[0]


@pytest.mark.parametrize("batch", mc.BATCHES)
def test_batch_length_changes_no_bit(monkeypatch, schedule_clean, batch):
    if batch is not None:
        monkeypatch.setenv("DVS_MANTEL_BATCH", str(batch))
    assert same_result(_fresh(1)[0], schedule_clean)
    c = engine.Context(0)
    try:
        c.refresh_knobs()
        info = run_case(c, exact("plain-n65-P32"))[3]
        B = batch or mc.DEFAULT_BATCH
        assert (info.batch, info.passes) == (B, 2 + -(-33 // B))
    finally:
        c.close()


def test_the_widest_batch(monkeypatch, schedule_clean):
    monkeypatch.setenv("DVS_MANTEL_BATCH", "1000")  # (32 at most)
    assert same_result(_fresh(1)[0], schedule_clean)


def test_poisoned_blocks_and_a_second_run_change_no_bit(monkeypatch, schedule_clean):
    monkeypatch.setenv("DVS_TEST_KNOBS", POISON)
    first, again = _fresh(2)
    assert same_result(first, schedule_clean) and same_result(again, schedule_clean)


# ---- every block request refused in turn

def _fused_case(c):
    seqs = family_seqs(3, 8, 600, seed=5)
    arrays = [seqs[s] for s in seqs]
    fit = mantel.of_sequences(arrays, {"distance_mode": "mash", "k": 8, "sketch_size": 100}, {"distance_mode": "jsd", "k": 4},
                              permutations=21, seed=2, ctx=c)
    return {"z": fit.z, "moments": fit.moments, "counts": np.array([fit.n_ge, fit.n_le, fit.n_abs_ge])}


def _host_against_device_case(c):
    import torch

    case = exact("plain-n257-P33")
    X, Y = mc.case_matrices(case)
    t = torch.from_numpy(np.array(Y)).to("cuda:0")
    torch.cuda.synchronize()
    rc, mom, z, inf = raw_call(c, given(X), on_device(t), mc.case_perms(case))
    c.check(rc)
    assert same_bits(t.cpu().numpy(), np.array(Y))
    assert_is_yardstick((rc, mom, z, inf), case)
    return {"z": z, "moments": mom, "counts": np.array([inf.n_ge, inf.n_le, inf.n_abs_ge])}


def _counts(c) -> dict:
    gc.collect()
    return c.block_stats()


@pytest.mark.parametrize("run", [_fused_case, _host_against_device_case], ids=["fused-mash-jsd", "host-x-device-y"])
def test_every_request_refused_in_turn(monkeypatch, run):
    c = engine.Context(0)
    try:
        clean = run(c)
        base = _counts(c)
    finally:
        c.close()
    R, L0, P0 = base["requests"], base["live_blocks"], base["pinned_out"]
    print(f"\nrefused blocks: {run.__name__}: R = {R}, L0 = {L0}, P0 = {P0}")
    assert R >= 3

    def same(got, what):
        assert list(got) == list(clean) and all(same_bits(got[k], clean[k]) for k in clean), what

    for i in range(1, R + 2):
        monkeypatch.setenv("DVS_TEST_KNOBS", f"{POISON},{REFUSE}{i}")
        c = engine.Context(0)
        try:
            what = f"{run.__name__}, request {i} of {R}"
            try:
                got = run(c)
            except MemoryError as err:
                assert f"{REFUSE}{i}" in str(err) and "refused by the test knob" in str(err), (what, str(err))
                assert i <= R, what
                got = None
            if got is not None:
                same(got, what)
            after = _counts(c)
            assert after["live_blocks"] <= L0 and after["pinned_out"] <= P0, (what, "left outstanding", after, base)
            if i == R + 1:
                assert after["requests"] == R, (what, after)
                continue
            same(run(c), f"{what}: the same context again")
            after = _counts(c)
            assert (after["live_blocks"], after["pinned_out"]) == (L0, P0), (what, after, base)
        finally:
            c.close()


# ---- errors; the context stays usable after each

def _still_usable(ctx):
    case = exact("plain-n65-P33")
    assert_is_yardstick(run_case(ctx, case), case, "after an error")


def test_bad_entries(ctx):
    case = exact("plain-n65-P1")
    X, Y = (np.array(M) for M in mc.case_matrices(case))
    n = case.n
    for where in ((0, 1), (2, 7), (n - 2, n - 1)):
        for value, match in ((np.nan, "NaN or infinity"), (np.inf, "NaN or infinity"), (-np.inf, "NaN or infinity"),
                             (-0.5, "negative")):
            for side in (0, 1):
                bad = [X.copy(), Y.copy()]
                bad[side][where] = value
                with pytest.raises(ValueError, match=match) as err:
                    mantel.mantel(bad[0], bad[1], permutations=3, ctx=ctx)
                assert "dvs_mantel" in str(err.value) and ("second" if side else "first") in str(err.value)
        _still_usable(ctx)
    no_kmers = [np.full(50, 4, np.uint8), np.arange(50, dtype=np.uint8) % 4, np.ones(50, np.uint8), np.arange(50, dtype=np.uint8) % 3]
    with pytest.raises(ValueError, match="NaN or infinity"):
        mantel.of_sequences(no_kmers, {"distance_mode": "euclidean", "k": 3}, {"distance_mode": "jsd", "k": 3}, permutations=2, ctx=ctx)
    empty = [np.zeros(3, np.uint8), np.ones(2, np.uint8), np.arange(40, dtype=np.uint8) % 4, np.arange(40, dtype=np.uint8) % 3]
    mash, jsd = {"distance_mode": "mash", "k": 8, "sketch_size": 10}, {"distance_mode": "jsd", "k": 2}
    for modes in ((mash, jsd), (jsd, mash)):  # either MASH source
        with pytest.raises(ZeroDivisionError):
            mantel.of_sequences(empty, *modes, permutations=2, ctx=ctx)
    _still_usable(ctx)


def test_errors_c_boundary(ctx):
    L = ctx._L
    n = 9
    rng = np.random.default_rng(13)
    dx, dy = (np.ascontiguousarray(rng.integers(0, 8, (n, n)).astype(np.float64)) for _ in range(2))
    perms = np.array([np.arange(n)[::-1], np.arange(n)], dtype=np.uint32)

    def fails(out, code, text=b"dvs_mantel"):
        assert (out if isinstance(out, int) else out[0]) == code, L.dvs_last_error(ctx._h)
        assert text in L.dvs_last_error(ctx._h), L.dvs_last_error(ctx._h)

    assert raw_call(ctx, given(dx), given(dy), perms)[0] == _lib.OK
    assert raw_call(ctx, given(dx), given(dy), None)[0] == _lib.OK
    fails(raw_call(ctx, given(dx[:2, :2]), given(dy[:2, :2]), None), _lib.ERR_VALUE, b"three at least")   # n < 3
    fails(raw_call(ctx, given(dx), given(dy[:8, :8]), None), _lib.ERR_VALUE, b"9 rows against 8 rows")     # x->n != y->n
    fails(raw_call(ctx, given(dx), given(dy), perms, moments=False), _lib.ERR_VALUE)
    fails(raw_call(ctx, given(dx), given(dy), perms, z=False), _lib.ERR_VALUE)
    mom, z = np.zeros(6), np.zeros(3)
    mp, zp = mom.ctypes.data_as(f64p), z.ctypes.data_as(f64p)
    fails(L.dvs_mantel(ctx._h, given(dx), given(dy), None, 2, mp, zp, None), _lib.ERR_VALUE)
    fails(L.dvs_mantel(ctx._h, given(dx), given(dy), perms.ctypes.data_as(u32p), 0, mp, zp, None), _lib.ERR_VALUE)
    fails(L.dvs_mantel(ctx._h, None, given(dy), None, 0, mp, zp, None), _lib.ERR_VALUE)
    fails(L.dvs_mantel(ctx._h, given(dx), None, None, 0, mp, zp, None), _lib.ERR_VALUE)
    for row, bad in ((0, [0, 1, 2, 3, 4, 5, 6, 7, 9]), (1, [0, 1, 2, 3, 4, 5, 6, 7, 7]), (1, [8] * 9)):  # not a permutation
        broken = np.array([np.arange(n)] * 2, dtype=np.uint32)
        broken[row] = bad
        fails(raw_call(ctx, given(dx), given(dy), broken), _lib.ERR_VALUE, f"permutation {row} ".encode())
    late = np.array([np.arange(n)] * 40, dtype=np.uint32)
    late[37, 0] = 1                                                                        # in the third batch
    fails(raw_call(ctx, given(dx), given(dy), late), _lib.ERR_VALUE, b"permutation 37 ")
    assert raw_call(ctx, given(dx, on_device=1), given(dy), perms)[0] == _lib.ERR_VALUE    # a host pointer said to be device memory
    assert raw_call(ctx, given(dx), given(dy, on_device=1), perms)[0] == _lib.ERR_VALUE
    huge = 200_000
    fails(raw_call(ctx, given(dx, huge), given(dy, huge), None), _lib.ERR_NOMEM)            # 320 GB a matrix
    seqs = [np.arange(60, dtype=np.uint8) % 4, np.arange(70, dtype=np.uint8) % 3, np.ones(50, np.uint8), np.arange(64, dtype=np.uint8) % 2]
    m = ctx.build_matrix(seqs, 2, 4)
    try:
        four = given(dx[:4, :4])
        listed = distance.make_source(_lib.SRC_JSD, m._h, 4, np.arange(4, dtype=np.uint32))
        fails(raw_call(ctx, listed, four, None), _lib.ERR_UNSUPPORTED)                     # a row list, on either side
        fails(raw_call(ctx, four, listed, None), _lib.ERR_UNSUPPORTED)
        three = given(dx[:3, :3])
        fails(raw_call(ctx, distance.make_source(_lib.SRC_JSD, m._h, 3), three, None), _lib.ERR_UNSUPPORTED)  # some of the rows
        whole = distance.make_source(_lib.SRC_JSD, m._h, 4)
        euclid = distance.make_source(_lib.SRC_EUCLIDEAN, m._h, 4)
        assert raw_call(ctx, whole, four, None)[0] == _lib.OK
        assert raw_call(ctx, whole, euclid, np.array([[3, 2, 1, 0]], dtype=np.uint32))[0] == _lib.OK  # two kinds: the point of the entry
    finally:
        m.close()
    _still_usable(ctx)


# ---- the Python layer and the app

def test_python_layer(ctx):
    case = next(c for c in mc.REAL_CASES if c.n == 300 and c.family == "uniform")
    X, Y = mc.case_matrices(case)
    one = mantel.mantel(X, Y, permutations=50, seed=12, ctx=ctx)
    assert same_result(mantel.mantel(X, Y, permutations=50, seed=12, ctx=ctx), one)
    s = mc.sums(X, Y, mc.documented_permutations(case.n, 50, 12))
    st = mc.statistics(case.n, s)
    assert one.p_value == st.p_value["two-sided"] and (one.n_ge, one.n_le, one.n_abs_ge) == (st.n_ge, st.n_le, st.n_abs_ge)
    assert abs(one.r - st.r[0]) <= 4 * mc.band(case.n) and np.abs(one.r_permuted - st.r[1:]).max() <= 4 * mc.band(case.n)
    assert one.permutations == 50 and one.n == case.n and one.moments.shape == (6,) and one.passes == 2 + 2
    assert mantel.mantel(X, Y, permutations=50, seed=12, alternative="greater", ctx=ctx).p_value == st.p_value["greater"]
    assert mantel.mantel(X, Y, permutations=50, seed=12, alternative="less", ctx=ctx).p_value == st.p_value["less"]
    assert not same_bits(mantel.mantel(X, Y, permutations=50, seed=13, ctx=ctx).z, one.z)
    assert mantel.mantel(X, Y, ctx=ctx).permutations == 999
    none = mantel.mantel(X, Y, permutations=0, ctx=ctx)
    assert np.isnan(none.p_value) and none.r_permuted.size == 0 and none.r == one.r
    strata = [i % 5 for i in range(case.n)]
    strat = mantel.mantel(X, Y, permutations=20, seed=3, strata=strata, ctx=ctx)
    want = mc.statistics(case.n, mc.sums(X, Y, mc.documented_permutations(case.n, 20, 3, np.array(strata))))
    assert strat.p_value == want.p_value["two-sided"] and (strat.n_ge, strat.n_le) == (want.n_ge, want.n_le)
    frozen = mantel.mantel(X, Y, permutations=7, seed=3, strata=list(range(case.n)), ctx=ctx)  # every item its own block
    assert frozen.p_value == 1.0 and (frozen.z == frozen.z[0]).all()
    const = mantel.mantel(X, np.ones((case.n, case.n)), permutations=5, ctx=ctx)
    assert np.isnan(const.r) and np.isnan(const.p_value) and np.isnan(const.r_permuted).all()


def test_app(brca1):
    x_mode, y_mode = {"distance_mode": "jsd", "k": 5}, {"distance_mode": "mash", "k": 10, "sketch_size": 500}
    got = mantel.dvs_mantel(x_mode, y_mode, permutations=25, seed=8, alternative="greater")(brca1)
    arrays = [brca1[n] for n in brca1]
    fit = mantel.of_sequences(arrays, MODE_ARGS["jsd"], MODE_ARGS["mash"], permutations=25, seed=8, alternative="greater")
    assert got == {"r": fit.r, "p_value": fit.p_value, "alternative": "greater", "permutations": 25, "n": len(arrays)}
    assert 0 < got["r"] < 1 and 0 < got["p_value"] <= 1
