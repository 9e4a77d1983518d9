"""PERMANOVA on the GPU (csrc/permanova.hip) against the yardstick of tests/permanova_cases.py, whose own pinning and
the conditions of every case here are in test_permanova_host.py.  Exact families as arrays; the bits of a partition
whatever its labels are called and wherever its vector sits in a batch; real-valued input within (n + 8) 2^-52 of the
long-double truth, with the yardstick's count and p; only the cells above the diagonal read; the three modes and a
caller's matrix in host and device memory; every batch length and poisoned blocks; every error of the C boundary; the
Python layer and the app.

Measured on an MI355X: the worst |device - truth| / (band * truth) over every sum of the nine real-valued cases is 0.030
(grouped-n40-a3-P99; 0.0013 to 0.024 in the others); test_real_valued_input_within_the_band prints each case's."""
import ctypes as C

import numpy as np
import pytest

from diverseseq_amd import _lib, apps, cluster, distance, engine
import permanova_cases as pc
from test_blocks_host import POISON
from test_gpu_linkage import family_seqs

pytestmark = pytest.mark.gpu

u32p, f64p = C.POINTER(C.c_uint32), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context()


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_result(a, b) -> bool:
    """two PERMANOVA (or lists of values), every field bit for bit"""
    return len(a) == len(b) and all(same_bits(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def given(D, n=None, on_device=0, rows=None):
    D = np.ascontiguousarray(D, dtype=np.float64)
    return distance.make_source(_lib.SRC_GIVEN, D.ctypes.data, D.shape[0] if n is None else n, rows, on_device=on_device, keep=D)


def raw_call(ctx, src, labels, a, perms, *, group=True, info=True, total=True, within=True):
    """dvs_permanova itself -> (rc, ss_total, ss_within, group_ss, info); the outputs NULL on demand"""
    labels = None if labels is None else np.ascontiguousarray(labels, dtype=np.uint32)
    perms = None if perms is None else np.ascontiguousarray(perms, dtype=np.uint32)
    P = 0 if perms is None else perms.shape[0]
    sst, ssw, gss, inf = C.c_double(-7.0), np.full(P + 1, -7.0), np.full(max(a, 1), -7.0), _lib.PermanovaInfo(99, 99, 99)
    rc = ctx._L.dvs_permanova(ctx._h, src, None if labels is None else labels.ctypes.data_as(u32p), a,
                              perms.ctypes.data_as(u32p) if P else None, P, C.byref(sst) if total else None,
                              ssw.ctypes.data_as(f64p) if within else None, gss.ctypes.data_as(f64p) if group else None,
                              C.byref(inf) if info else None)
    return rc, sst.value, ssw, gss, inf


def assert_is_ref(out, ref: pc.Ref, label: str):
    rc, sst, ssw, gss, inf = out
    assert rc == _lib.OK, label
    assert sst == ref.ss_total and np.array_equal(ssw, ref.ss_within) and np.array_equal(gss, ref.group_ss), label
    assert inf.n_le == ref.n_le, label


# ---- exact families, as arrays

@pytest.mark.parametrize("case", pc.EXACT_CASES, ids=lambda c: c.id)
def test_exact_families_as_arrays(ctx, case):
    D, lab, perms, ref = pc.case_matrix(case), pc.case_labels(case), pc.case_perms(case), pc.case_ref(case)
    out = raw_call(ctx, given(D), lab, case.a, perms)
    assert_is_ref(out, ref, case.id)
    B = pc.DEFAULT_BATCH
    assert (out[4].passes, out[4].batch) == (1 + -(-(case.P + 1) // B), B)
    if case.n <= 300:  # the Python layer derives the rest as the yardstick does
        got = cluster.permanova(D, lab.tolist(), permutations=0, ctx=ctx)
        assert got.ss_within == ref.ss_within[0] and np.array_equal(got.group_ss, ref.group_ss)
        assert same_bits(np.float64(got.f), ref.f[0]) and same_bits(np.float64(got.r2), np.float64(ref.r2))
        assert np.isnan(got.p_value) and got.perm_f.size == 0 and np.array_equal(got.group_sizes, np.bincount(lab))


def test_optional_outputs(ctx):
    case = next(c for c in pc.EXACT_CASES if c.n == 257 and c.P == 17)
    D, lab, perms, ref = pc.case_matrix(case), pc.case_labels(case), pc.case_perms(case), pc.case_ref(case)
    rc, sst, ssw, gss, inf = raw_call(ctx, given(D), lab, case.a, perms, group=False, info=False)
    assert rc == _lib.OK and sst == ref.ss_total and np.array_equal(ssw, ref.ss_within)
    assert (gss == -7.0).all() and (inf.n_le, inf.passes, inf.batch) == (99, 99, 99)


# ---- a function of the partition and its sizes only

def test_the_bits_of_a_partition(ctx, monkeypatch):
    case = next(c for c in pc.REAL_CASES if c.n == 300 and c.family == "grouped")
    D, lab, a, n = pc.case_matrix(case), pc.case_labels(case), case.a, case.n
    rng = np.random.default_rng(17)
    inside = np.arange(n)
    for g in range(a):  # a permutation that maps every group onto itself
        idx = np.flatnonzero(lab == g)
        inside[idx] = rng.permutation(idx)
    assert not np.array_equal(inside, np.arange(n)) and np.array_equal(lab[inside], lab)
    others = pc.documented_permutations(lab, 30, 5)
    rows = np.concatenate([others[:14], [lab], [lab[inside]], others[14:], [lab[np.arange(n)]]])  # vectors 15, 16 and 33
    same_at = [14, 15, 32]
    src = given(D)
    rc, sst, ssw, gss, inf = raw_call(ctx, src, lab, a, rows)
    assert rc == _lib.OK
    for p in same_at:
        assert same_bits(ssw[p + 1], ssw[0]), p
    ref = pc.permanova_ref(D, lab, a, rows)
    truth = pc.sums(D, lab, a, rows, np.longdouble)[1]
    assert inf.n_le == int((truth[1:] <= truth[0]).sum()) >= 3 and inf.n_le == ref.n_le
    # renamed groups: the same bits, each group's term under its new name
    rename = rng.permutation(a).astype(np.uint32)
    rc2, sst2, ssw2, gss2, inf2 = raw_call(ctx, src, rename[lab], a, rename[rows])
    assert rc2 == _lib.OK and same_bits(ssw2, ssw) and same_bits(np.float64(sst2), np.float64(sst)) and inf2.n_le == inf.n_le
    assert same_bits(gss2[rename], gss)
    # ... and wherever the vector sits in a batch, whatever stands beside it
    monkeypatch.setenv("DVS_PERMANOVA_BATCH", "3")
    rc3, _, ssw3, _, inf3 = raw_call(ctx, src, lab, a, rows[::-1].copy())
    assert rc3 == _lib.OK and same_bits(ssw3[1:], ssw[1:][::-1]) and same_bits(ssw3[0], ssw[0]) and inf3.batch == 3


# ---- real-valued input

WORST = {}


@pytest.mark.parametrize("case", pc.REAL_CASES, ids=lambda c: c.id)
def test_real_valued_input_within_the_band(ctx, case):
    """every sum within (n + 8) 2^-52 of the long-double truth, relative to the sum of its terms; measured on an MI355X,
    the worst ratio |device - truth| / (band * truth) of all nine cases is 0.030"""
    D, lab, perms, ref = pc.case_matrix(case), pc.case_labels(case), pc.case_perms(case), pc.case_ref(case)
    t_total, t_within, t_group = pc.case_truth(case)
    rc, sst, ssw, gss, inf = raw_call(ctx, given(D), lab, case.a, perms)
    assert rc == _lib.OK
    band = pc.band(case.n)
    ratios = [abs(np.longdouble(sst) - t_total) / (band * t_total)]
    ratios += list(np.abs(ssw.astype(np.longdouble) - t_within) / (band * t_within))
    ratios += [abs(np.longdouble(g) - t) / (band * t) if t > 0 else np.longdouble(g != 0) * 2 for g, t in zip(gss, t_group)]
    WORST[case.id] = float(max(ratios))
    print(case.id, "worst |device - truth| / band:", WORST[case.id], "of all so far:", max(WORST.values()))
    assert max(ratios) <= 1.0, (case.id, float(max(ratios)))
    assert inf.n_le == ref.n_le
    got = cluster.permanova(D, lab.tolist(), permutations=case.P, seed=case.seed + 2, ctx=ctx)
    assert same_bits(np.float64(got.ss_within), ssw[0]) and got.p_value == ref.p_value and got.permutations == case.P
    assert same_bits(got.perm_f, pc.statistics(case.n, case.a, sst, ssw)[1][1:])


# ---- only the cells above the diagonal are read

def test_only_the_upper_triangle_is_read(ctx):
    case = next(c for c in pc.REAL_CASES if c.n == 300 and c.family == "uniform")
    D, lab, perms = pc.case_matrix(case), pc.case_labels(case), pc.case_perms(case)
    upper = np.triu(D, 1)
    holed = upper + np.tril(np.full(D.shape, np.nan))  # NaN on and below the diagonal
    assert np.isnan(holed[5, 5]) and np.isnan(holed[7, 2]) and holed[2, 7] == D[2, 7]
    want = raw_call(ctx, given(D), lab, case.a, perms)
    for variant in (holed, upper - np.tril(np.ones(D.shape)), upper + np.tril(np.full(D.shape, np.inf))):
        got = raw_call(ctx, given(variant), lab, case.a, perms)
        assert got[0] == _lib.OK and got[1] == want[1] and same_bits(got[2], want[2]) and same_bits(got[3], want[3])


# ---- sources

@pytest.fixture(scope="module")
def brca1_arrays(brca1):
    return [brca1[name] for name in brca1]


def brca1_grouping(n):
    return [("even", "odd", "third")[i % 3] if i > 4 else "first" for i in range(n)]


@pytest.mark.parametrize("mode", ["mash", "euclidean", "jsd"])
def test_brca1_fused_equals_the_matrix_route(ctx, brca1_arrays, mode):
    args = (10, 500) if mode == "mash" else (5,)
    grouping = brca1_grouping(len(brca1_arrays))
    dist = distance.MODES[mode][0](brca1_arrays, *args, ctx=ctx)
    kw = dict(permutations=37, seed=4)
    fused = distance.PERMANOVA_MODES[mode](brca1_arrays, *args, grouping=grouping, ctx=ctx, **kw)
    assert same_result(cluster.permanova(dist, grouping, ctx=ctx, **kw), fused), mode
    assert 0 < fused.p_value <= 1 and fused.perm_f.shape == (37,) and fused.group_sizes.sum() == len(brca1_arrays)
    mode_kw = dict(k=args[0], sketch_size=args[1] if mode == "mash" else None)
    assert same_result(distance.permanova(brca1_arrays, grouping, mode, ctx=ctx, **mode_kw, **kw), fused)
    if mode == "mash":
        sk = distance.Sketches(brca1_arrays, 10, 500, 4, False, ctx=ctx)
        try:
            assert same_result(sk.permanova(grouping, **kw), fused)
        finally:
            sk.close()
    else:
        m = ctx.build_matrix(brca1_arrays, 5, 4)
        try:
            assert same_result(distance.matrix_permanova(m, grouping, mode=mode, **kw), fused)
        finally:
            m.close()


def test_device_tensor_is_only_read_and_gives_the_same_bits(ctx):
    import torch

    case = next(c for c in pc.REAL_CASES if c.n == 300 and c.family == "crowded")
    D, lab = np.array(pc.case_matrix(case)), pc.case_labels(case).tolist()
    np.fill_diagonal(D, np.nan)
    host = cluster.permanova(D, lab, permutations=40, seed=1, ctx=ctx)
    t = torch.from_numpy(D).to("cuda:0")
    assert same_result(cluster.permanova(t, lab, permutations=40, seed=1, ctx=ctx), host)
    assert same_bits(t.cpu().numpy(), D)  # only read (NaN diagonal and all)
    with pytest.raises(ValueError):
        cluster.permanova(torch.zeros((4, 5), dtype=torch.float64, device="cuda:0"), list("aabb"), ctx=ctx)
    with pytest.raises(ValueError):
        cluster.permanova(torch.zeros((5, 5), dtype=torch.float32, device="cuda:0"), list("aabbc"), ctx=ctx)


# ---- the schedule changes no bit

def _schedule_case(c):
    out = []
    for case in (next(x for x in pc.REAL_CASES if x.n == 300 and x.family == "grouped"),
                 next(x for x in pc.REAL_CASES if x.n == 1025 and x.family == "uniform"),
                 next(x for x in pc.EXACT_CASES if x.n == 257 and x.P == 53),
                 next(x for x in pc.EXACT_CASES if x.n == 65 and x.P == 16)):
        got = raw_call(c, given(pc.case_matrix(case)), pc.case_labels(case), case.a, pc.case_perms(case))
        assert got[0] == _lib.OK and got[4].n_le == pc.case_ref(case).n_le
        out += [np.float64(got[1]), got[2], got[3]]
    seqs = family_seqs(5, 8, 1500, seed=21)
    arrays = [seqs[s] for s in seqs]
    grouping = [i // 8 for i in range(len(arrays))]
    out += list(distance.jsd_permanova(arrays, 4, grouping=grouping, permutations=20, seed=3, ctx=c))
    out.append(distance.jsd_kmedoids(arrays, 4, n_medoids=5, ctx=c).td)  # another operation in between
    out += list(distance.mash_permanova(arrays, 8, 200, grouping=grouping, permutations=20, seed=3, ctx=c))
    with pytest.raises(ValueError, match="negative"):  # a failing call, then the same context again
        cluster.permanova(-np.ones((9, 9)), list("aaabbbccc"), ctx=c)
    out += list(distance.euclidean_permanova(arrays, 4, grouping=grouping, permutations=20, seed=3, ctx=c))
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


@pytest.mark.parametrize("batch", pc.BATCHES)
def test_batch_length_changes_no_bit(monkeypatch, schedule_clean, batch):
    if batch is not None:
        monkeypatch.setenv("DVS_PERMANOVA_BATCH", str(batch))
    assert same_result(_fresh(1)[0], schedule_clean)


def test_the_widest_batch_changes_no_bit(monkeypatch, schedule_clean):
    monkeypatch.setenv("DVS_PERMANOVA_BATCH", "1000")  # (32 at most)
    assert same_result(_fresh(1)[0], schedule_clean)
    case = next(x for x in pc.EXACT_CASES if x.n == 65 and x.P == 16)
    c = engine.Context(0)
    try:
        c.refresh_knobs()
        info = raw_call(c, given(pc.case_matrix(case)), pc.case_labels(case), case.a, pc.case_perms(case))[4]
        assert (info.batch, info.passes) == (pc.MAX_BATCH, 2)
    finally:
        c.close()


def test_poisoned_blocks_and_a_second_run_change_no_bit(monkeypatch, schedule_clean):
    monkeypatch.setenv("DVS_TEST_KNOBS", POISON)
    first, again = _fresh(2)
    assert same_result(first, schedule_clean) and same_result(again, schedule_clean)


# ---- errors; the context stays usable after each

def _still_usable(ctx):
    case = next(c for c in pc.EXACT_CASES if c.n == 65 and c.P == 17)
    assert_is_ref(raw_call(ctx, given(pc.case_matrix(case)), pc.case_labels(case), case.a, pc.case_perms(case)), pc.case_ref(case),
                  "after an error")


def test_bad_entries(ctx):
    case = next(c for c in pc.EXACT_CASES if c.n == 65 and c.P == 1)
    d, lab = np.array(pc.case_matrix(case)), pc.case_labels(case).tolist()
    n = case.n
    for where in ((0, 1), (2, 7), (n - 2, n - 1)):
        for value, match in ((np.nan, "NaN or infinity"), (np.inf, "NaN or infinity"), (-np.inf, "NaN or infinity"),
                             (-0.5, "negative")):
            bad = d.copy()
            bad[where] = value
            with pytest.raises(ValueError, match=match) as err:
                cluster.permanova(bad, lab, permutations=3, ctx=ctx)
            assert "dvs_permanova" in str(err.value)
        _still_usable(ctx)
    no_kmers = [np.full(50, 4, np.uint8), np.arange(50, dtype=np.uint8) % 4, np.ones(50, np.uint8), np.arange(50, dtype=np.uint8) % 3]
    for mode in ("euclidean", "jsd"):
        with pytest.raises(ValueError, match="NaN or infinity"):
            distance.PERMANOVA_MODES[mode](no_kmers, 3, grouping=list("aabb"), permutations=2, ctx=ctx)
    empty = [np.zeros(3, np.uint8), np.ones(2, np.uint8), np.arange(40, dtype=np.uint8) % 4, np.arange(40, dtype=np.uint8) % 3]
    with pytest.raises(ZeroDivisionError):
        distance.mash_permanova(empty, 8, 10, grouping=list("abab"), permutations=2, ctx=ctx)
    _still_usable(ctx)


def test_errors_c_boundary(ctx):
    L = ctx._L
    n, a = 9, 3
    d = np.ascontiguousarray(np.random.default_rng(13).integers(0, 8, (n, n)).astype(np.float64))
    lab = np.array([0, 0, 0, 0, 1, 1, 1, 2, 2], dtype=np.uint32)
    perms = np.array([lab[::-1], lab], dtype=np.uint32)

    def src(count=n, **kw):
        return given(d, count, **kw)

    def fails(out, code):
        assert (out if isinstance(out, int) else out[0]) == code
        assert b"dvs_permanova" in L.dvs_last_error(ctx._h), L.dvs_last_error(ctx._h)

    assert raw_call(ctx, src(), lab, a, perms)[0] == _lib.OK
    assert raw_call(ctx, src(), lab, a, None)[0] == _lib.OK
    fails(raw_call(ctx, given(d[:2, :2]), lab[:2], 2, None), _lib.ERR_VALUE)             # n < 3
    fails(raw_call(ctx, src(), np.zeros(n, np.uint32), 1, None), _lib.ERR_VALUE)          # one group
    fails(raw_call(ctx, src(), np.arange(n, dtype=np.uint32), n, None), _lib.ERR_VALUE)   # n groups
    fails(raw_call(ctx, src(), np.where(lab == 2, 3, lab), a, None), _lib.ERR_VALUE)      # a label >= n_groups
    fails(raw_call(ctx, src(), np.where(lab == 2, 1, lab), a, None), _lib.ERR_VALUE)      # an empty group
    moved = perms.copy()
    moved[1, 0] = 1                                                                        # one item changes its group
    out = raw_call(ctx, src(), lab, a, moved)
    fails(out, _lib.ERR_VALUE)
    assert b"permutation 1 " in L.dvs_last_error(ctx._h)
    moved[0, 8] = 7
    fails(raw_call(ctx, src(), lab, a, moved), _lib.ERR_VALUE)                             # a label >= n_groups in a row
    assert b"permutation 0:" in L.dvs_last_error(ctx._h)
    fails(raw_call(ctx, src(), None, a, None), _lib.ERR_VALUE)
    fails(raw_call(ctx, src(), lab, a, perms, total=False), _lib.ERR_VALUE)
    fails(raw_call(ctx, src(), lab, a, perms, within=False), _lib.ERR_VALUE)
    u = lab.ctypes.data_as(u32p)
    sst, ssw = C.c_double(), np.zeros(3)
    fails(L.dvs_permanova(ctx._h, src(), u, a, None, 2, C.byref(sst), ssw.ctypes.data_as(f64p), None, None), _lib.ERR_VALUE)
    fails(L.dvs_permanova(ctx._h, src(), u, a, perms.ctypes.data_as(u32p), 0, C.byref(sst), ssw.ctypes.data_as(f64p), None, None),
          _lib.ERR_VALUE)
    fails(L.dvs_permanova(ctx._h, None, u, a, None, 0, C.byref(sst), ssw.ctypes.data_as(f64p), None, None), _lib.ERR_VALUE)
    big = 70_000
    fails(raw_call(ctx, src(big), np.arange(big, dtype=np.uint32) % 65_536, 65_536, None), _lib.ERR_UNSUPPORTED)  # (before the matrix is looked at)
    assert raw_call(ctx, src(on_device=1), lab, a, perms)[0] == _lib.ERR_VALUE            # a host pointer said to be device memory
    huge = 200_000
    fails(raw_call(ctx, src(huge), np.arange(huge, dtype=np.uint32) % 2, 2, None), _lib.ERR_NOMEM)  # 320 GB of matrix
    seqs = [np.arange(60, dtype=np.uint8) % 4, np.arange(70, dtype=np.uint8) % 3, np.ones(50, np.uint8), np.arange(64, dtype=np.uint8) % 2]
    m = ctx.build_matrix(seqs, 2, 4)
    try:
        four, two = np.array([0, 1, 0, 1], np.uint32), 2
        listed = distance.make_source(_lib.SRC_JSD, m._h, 4, np.arange(4, dtype=np.uint32))
        fails(raw_call(ctx, listed, four, two, None), _lib.ERR_UNSUPPORTED)               # a row list
        fails(raw_call(ctx, distance.make_source(_lib.SRC_JSD, m._h, 3), four[:3], two, None), _lib.ERR_UNSUPPORTED)  # some of the rows
        assert raw_call(ctx, distance.make_source(_lib.SRC_JSD, m._h, 4), four, two, None)[0] == _lib.OK
    finally:
        m.close()
    _still_usable(ctx)


# ---- the Python layer and the app

def test_python_layer(ctx):
    case = next(c for c in pc.REAL_CASES if c.n == 300 and c.family == "grouped")
    D, lab = pc.case_matrix(case), pc.case_labels(case)
    names = [f"clade {g}" for g in lab]
    one = cluster.permanova(D, names, permutations=50, seed=12, ctx=ctx)
    assert same_result(cluster.permanova(D, names, permutations=50, seed=12, ctx=ctx), one)
    assert same_result(cluster.permanova(D, lab.tolist(), permutations=50, seed=12, ctx=ctx), one)
    ref = pc.permanova_ref(D, lab, case.a, pc.documented_permutations(lab, 50, 12))
    assert one.p_value == ref.p_value and one.permutations == 50
    assert abs(one.f - ref.f[0]) <= 1e-9 * ref.f[0] and abs(one.r2 - ref.r2) <= 1e-9
    assert one.ss_among == one.ss_total - one.ss_within
    assert not same_bits(cluster.permanova(D, names, permutations=50, seed=13, ctx=ctx).perm_f, one.perm_f)
    assert cluster.permanova(D, names, ctx=ctx).permutations == 999
    none = cluster.permanova(D, names, permutations=0, ctx=ctx)
    assert np.isnan(none.p_value) and none.perm_f.size == 0 and none.f == one.f
    # strata: labels move inside their block only; with the groups themselves as the blocks every vector is the observed one
    blocks = [i % 5 for i in range(case.n)]
    rows = pc.documented_permutations(lab, 20, 3, np.array(blocks))
    strat = cluster.permanova(D, names, permutations=20, seed=3, strata=blocks, ctx=ctx)
    want = pc.permanova_ref(D, lab, case.a, rows)
    assert strat.p_value == want.p_value and abs(strat.perm_f - want.f[1:]).max() <= 1e-9 * want.f[1:].max()
    frozen = cluster.permanova(D, names, permutations=20, seed=3, strata=names, ctx=ctx)
    assert frozen.p_value == 1.0 and (frozen.perm_f == frozen.f).all()
    # zero distances: SS_T == 0 gives nan; zero within the groups only gives inf
    assert np.isnan(cluster.permanova(np.zeros((6, 6)), list("aabbcc"), permutations=3, ctx=ctx).f)
    apart = (np.array(list("aabbcc"))[:, None] != np.array(list("aabbcc"))[None, :]).astype(np.float64)
    split = cluster.permanova(apart, list("aabbcc"), permutations=3, ctx=ctx)
    assert split.f == np.inf and split.ss_within == 0.0 and split.r2 == 1.0


def test_app(brca1):
    names = list(brca1)
    grouping = dict(zip(names, brca1_grouping(len(names))))
    got = apps.dvs_permanova(grouping, "jsd", k=5, sketch_size=None, permutations=25, seed=8)(brca1)
    fit = distance.permanova([brca1[n] for n in names], [grouping[n] for n in names], "jsd", k=5, permutations=25, seed=8)
    assert (got["f"], got["p_value"], got["r2"], got["permutations"]) == (fit.f, fit.p_value, fit.r2, 25)
    assert got["groups"] == ["first", "third", "even", "odd"]  # (in the order of their first sequence)
    assert list(got["group_sizes"].values()) == fit.group_sizes.tolist() and list(got["group_ss"].values()) == fit.group_ss.tolist()
    assert (got["ss_total"], got["ss_within"], got["ss_among"]) == (fit.ss_total, fit.ss_within, fit.ss_among)
    with pytest.raises(ValueError, match="no group"):
        apps.dvs_permanova({names[0]: "x"}, "jsd", k=5, sketch_size=None)(brca1)
