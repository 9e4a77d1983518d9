"""k-medoids on the GPU (csrc/kmedoids.hip) against the yardstick of tests/kmedoids_cases.py, whose own pinning and the
conditions of every case here are in test_kmedoids_host.py.  Exact families bit for bit; general input by the unique
exchange sequence its gaps make, the state recomputed from the returned medoids, td within (n + 8) 2^-52 of the
long-double sum and no Delta of the final state below minus the band; the three modes and a caller's matrix in host and
device memory; every batch length and poisoned blocks; every error of the C boundary."""
import ctypes as C

import numpy as np
import pytest

from diverseseq_amd import _lib, apps, cluster, distance, engine
import kmedoids_cases as kc
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
    """two KMedoids (or lists of arrays), every field bit for bit"""
    return len(a) == len(b) and all(same_bits(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def assert_is_ref(got, ref: kc.Ref, label: str):
    """every field of a KMedoids equal to the yardstick's as arrays (0.0 == -0.0, inf == inf)"""
    assert np.array_equal(got.medoids, ref.medoids), label
    assert np.array_equal(got.swaps, ref.swaps), label
    assert np.array_equal(got.td, ref.td), label
    assert np.array_equal(got.labels, ref.labels), label
    assert np.array_equal(got.dist, ref.dist), label
    assert np.array_equal(got.second, ref.second), label
    assert (got.stop, got.passes) == (ref.stop, ref.passes), label


def init_of(case):
    return "build" if case.init == "build" else kc.given_medoids(case)


# ---- exact families, bit for bit

@pytest.mark.parametrize("case", kc.EXACT_CASES, ids=lambda c: c.id)
def test_exact_families_bit_for_bit(ctx, case):
    D, ref = kc.case_matrix(case), kc.case_ref(case)
    got = cluster.kmedoids(D, case.k, init=init_of(case), max_swaps=case.max_swaps, ctx=ctx)
    if case.init == "build":  # BUILD's own medoids: what a run without exchanges returns
        assert np.array_equal(cluster.kmedoids(D, case.k, max_swaps=0, ctx=ctx).medoids, ref.build), case.id
    assert_is_ref(got, ref, case.id)
    if 0 < case.max_swaps <= 2 and case.n == 257 and len(ref.swaps) == case.max_swaps:
        longer = kc.kmedoids_ref(D, case.k, init_of(case), 300)
        if len(longer.swaps) > case.max_swaps:
            assert got.stop == 0 and np.array_equal(got.swaps, longer.swaps[:case.max_swaps])


def raw_call(ctx, src, n, k, init, max_swaps, medoids=None, *, second=True, swaps=True, td=True):
    """dvs_kmedoids itself -> (rc, medoids, labels, dist, second, swaps, td, info); the optional outputs NULL on demand"""
    p = _lib.KmedoidsParams(k, init, max_swaps, 0)
    info = _lib.KmedoidsInfo()
    med = np.zeros(max(k, 1), dtype=np.uint32) if medoids is None else np.array(medoids, dtype=np.uint32)
    labels, dist, sec = np.zeros(n, np.uint32), np.zeros(n), np.full(n, -7.0)
    sw, tds = np.full((max(max_swaps, 1), 2), 99, np.uint32), np.full(max_swaps + 1, -7.0)
    rc = ctx._L.dvs_kmedoids(ctx._h, src, C.byref(p), med.ctypes.data_as(u32p), labels.ctypes.data_as(u32p),
                             dist.ctypes.data_as(f64p), sec.ctypes.data_as(f64p) if second else None,
                             sw.ctypes.data_as(u32p) if swaps else None, tds.ctypes.data_as(f64p) if td else None, C.byref(info))
    return rc, med, labels, dist, sec, sw, tds, info


def test_c_entry_outputs_and_optional_ones(ctx):
    case = next(c for c in kc.EXACT_CASES if c.n == 257 and c.k == 7 and c.init == "given" and c.max_swaps == 300
                and len(kc.case_ref(c).swaps) >= 2)
    D, ref = np.ascontiguousarray(kc.case_matrix(case)), kc.case_ref(case)
    src = distance.make_source(_lib.SRC_GIVEN, D.ctypes.data, case.n, keep=D)
    m = len(ref.swaps)
    for opt in (dict(), dict(second=False, swaps=False, td=False)):
        rc, med, labels, dist, sec, sw, tds, info = raw_call(ctx, src, case.n, case.k, 1, 300, kc.given_medoids(case), **opt)
        assert rc == _lib.OK
        assert np.array_equal(med, ref.medoids) and np.array_equal(labels, ref.labels) and np.array_equal(dist, ref.dist)
        assert (info.n_swaps, info.stop, info.passes, info.td_init, info.td) == (m, 1, ref.passes, ref.td[0], ref.td[-1])
        if opt:
            assert (sec == -7.0).all() and (sw == 99).all() and (tds == -7.0).all()
        else:
            assert np.array_equal(sec, ref.second) and np.array_equal(sw[:m], ref.swaps) and np.array_equal(tds[:m + 1], ref.td)
            assert (sw[m:] == 99).all() and (tds[m + 1:] == -7.0).all()  # (behind the exchanges made: left as it was)


# ---- general input

@pytest.mark.parametrize("case", kc.GENERAL_CASES, ids=lambda c: c.id)
def test_general_input(ctx, case):
    D, ref = kc.case_matrix(case), kc.case_ref(case)
    n = case.n
    got = cluster.kmedoids(D, case.k, init=init_of(case), max_swaps=case.max_swaps, ctx=ctx)
    if case.init == "build":
        assert np.array_equal(cluster.kmedoids(D, case.k, max_swaps=0, ctx=ctx).medoids, ref.build)
    assert np.array_equal(got.swaps, ref.swaps) and np.array_equal(got.medoids, ref.medoids)
    assert (got.stop, got.passes) == (1, ref.passes)
    near, dn, ds = kc.state_of(kc.zero_diagonal(D), got.medoids)
    assert np.array_equal(got.labels, near) and np.array_equal(got.dist, dn) and np.array_equal(got.second, ds)
    med = ref.build.copy()
    for t in range(len(got.td)):
        if t:
            med[got.swaps[t - 1, 1]] = got.swaps[t - 1, 0]
        exact = kc.state_of(kc.zero_diagonal(D), med)[1].astype(np.longdouble).sum()
        print(case.id, t, float(got.td[t]), float(abs(got.td[t] - exact) / exact))
        assert abs(got.td[t] - exact) <= kc.td_bound(n) * exact
    off = D[~np.eye(n, dtype=bool)]
    assert not (kc.delta_truth(D, got.medoids) < -kc.band(n, float(off.max()))).any()


# ---- sources

@pytest.fixture(scope="module")
def brca1_arrays(brca1):
    return [brca1[name] for name in brca1]


def _mode_call(mode):
    if mode == "mash":
        return (10, 500), dict()
    return (5,), dict()


@pytest.mark.parametrize("mode", ["mash", "euclidean", "jsd"])
def test_brca1_fused_equals_the_matrix_route(ctx, brca1, brca1_arrays, mode):
    args, _ = _mode_call(mode)
    dist = distance.MODES[mode][0](brca1_arrays, *args, ctx=ctx)
    for k, init in ((1, "build"), (4, "build"), (9, "maxmin"), (4, [5, 1, 30, 2])):
        fused = distance.KMEDOIDS_MODES[mode](brca1_arrays, *args, n_medoids=k, init=init, ctx=ctx)
        assert same_result(cluster.kmedoids(dist, k, init=init, ctx=ctx), fused), (mode, k, init)
        assert fused.stop == 1 and (np.diff(fused.td) < 0).all()
        near, dn, ds = kc.state_of(kc.zero_diagonal(dist), fused.medoids)
        assert np.array_equal(fused.labels, near) and np.array_equal(fused.dist, dn) and np.array_equal(fused.second, ds)
    kw = dict(k=args[0], sketch_size=args[1] if mode == "mash" else None)
    assert same_result(distance.kmedoids(brca1_arrays, 4, mode, ctx=ctx, **kw),
                       distance.KMEDOIDS_MODES[mode](brca1_arrays, *args, n_medoids=4, ctx=ctx))
    names, sizes, labels, fit = cluster.representatives(brca1, 4, distance_mode=mode, **kw)
    assert names == [list(brca1)[i] for i in fit.medoids] and sizes.sum() == len(brca1) and np.array_equal(labels, fit.labels)
    assert np.array_equal(sizes, np.bincount(fit.labels, minlength=4))
    assert same_result(fit, cluster.kmedoids(dist, 4, ctx=ctx))


def test_brca1_count_widths_canonical_rows_and_handles(ctx, monkeypatch, brca1_arrays):
    narrow = distance.jsd_kmedoids(brca1_arrays, 5, n_medoids=5, ctx=ctx)
    monkeypatch.setenv("DVS_COUNTS_U32", "1")
    wide_ctx = engine.Context(0)
    try:
        assert same_result(distance.jsd_kmedoids(brca1_arrays, 5, n_medoids=5, ctx=wide_ctx), narrow)
    finally:
        wide_ctx.close()
    monkeypatch.delenv("DVS_COUNTS_U32")
    folded = distance.jsd_kmedoids(brca1_arrays, 5, n_medoids=5, ctx=ctx, canonical=True)
    assert same_result(cluster.kmedoids(distance.jsd_distances(brca1_arrays, 5, ctx=ctx, canonical=True), 5, ctx=ctx), folded)
    m = ctx.build_matrix(brca1_arrays, 5, 4)
    try:
        assert same_result(distance.matrix_kmedoids(m, 5), narrow)
        assert same_result(distance.matrix_kmedoids(m, 3, mode="euclidean"),
                           distance.euclidean_kmedoids(brca1_arrays, 5, n_medoids=3, ctx=ctx))
    finally:
        m.close()
    sk = distance.Sketches(brca1_arrays, 10, 500, 4, False, ctx=ctx)
    try:
        assert same_result(sk.kmedoids(3), distance.mash_kmedoids(brca1_arrays, 10, 500, n_medoids=3, ctx=ctx))
    finally:
        sk.close()


def test_device_tensor_is_only_read_and_gives_the_same_bits(ctx):
    import torch

    case = next(c for c in kc.GENERAL_CASES if c.n == 300 and c.k == 5 and c.init == "build")
    D = np.array(kc.case_matrix(case))
    host = cluster.kmedoids(D, 5, ctx=ctx)
    assert same_result(cluster.kmedoids(D, 5, ctx=ctx), host)
    t = torch.from_numpy(D).to("cuda:0")
    assert same_result(cluster.kmedoids(t, 5, ctx=ctx), host)
    assert same_result(cluster.kmedoids(t, 5, init="maxmin", ctx=ctx), cluster.kmedoids(D, 5, init="maxmin", ctx=ctx))
    assert same_bits(t.cpu().numpy(), D)  # only read (NaN diagonal and all)
    with pytest.raises(ValueError):
        cluster.kmedoids(torch.zeros((4, 5), dtype=torch.float64, device="cuda:0"), 2, ctx=ctx)
    with pytest.raises(ValueError):
        cluster.kmedoids(torch.zeros((5, 5), dtype=torch.float32, device="cuda:0"), 2, ctx=ctx)


def test_init_maxmin_is_the_composition_by_hand(ctx, brca1_arrays):
    dist = distance.jsd_distances(brca1_arrays, 5, ctx=ctx)
    picks = cluster.maxmin(dist, 6, ctx=ctx).picks
    by_hand = cluster.kmedoids(dist, 6, init=picks, ctx=ctx)
    assert same_result(cluster.kmedoids(dist, 6, init="maxmin", ctx=ctx), by_hand)
    assert same_result(distance.jsd_kmedoids(brca1_arrays, 5, n_medoids=6, init="maxmin", ctx=ctx), by_hand)
    scored = cluster.kmedoids(dist, 6, init=picks, max_swaps=0, ctx=ctx)  # the picks scored as representatives
    assert scored.stop == 0 and np.array_equal(scored.medoids, picks) and scored.td[0] == by_hand.td[0]
    assert by_hand.td[-1] <= scored.td[0]


def test_sampled_kmedoids_is_its_composition(ctx):
    seqs = family_seqs(6, 12, 1500, seed=5)
    names, medoids, labels, dist, marks, fit = cluster.sampled_kmedoids(seqs, 4, 20, k=5, sketch_size=None, distance_mode="jsd")
    arrays = [seqs[s] for s in seqs]
    assert names == list(seqs)
    with distance.device_side(arrays, "jsd", 5, 4, ctx=ctx) as dev:
        m = dev.maxmin(20, seeds=(0,)).picks
        f = cluster.kmedoids(dev.cross_distances(dev, m, m), 4, ctx=ctx)
        idx, d = dev.nearest(dev, 1, None, m[f.medoids])
        again = cluster.sampled_kmedoids(dev, 4, 20)
    assert np.array_equal(marks, m) and same_result(fit, f) and np.array_equal(medoids, m[f.medoids])
    assert np.array_equal(labels, idx[:, 0]) and same_bits(dist, d[:, 0])
    assert again[0] is None and np.array_equal(again[1], medoids) and np.array_equal(again[2], labels)
    assert (labels[medoids] == np.arange(4)).all() and (dist[medoids] == 0).all()


def test_app(brca1):
    kw = dict(k=5, sketch_size=None, distance_mode="jsd")
    got = apps.dvs_kmedoids(4, init="maxmin", max_swaps=50, **kw)(brca1)
    names, sizes, labels, fit = cluster.representatives(brca1, 4, init="maxmin", max_swaps=50, **kw)
    assert got["representatives"] == names and got["sizes"] == sizes.tolist() and got["converged"] == bool(fit.stop)
    assert got["total_distance"] == fit.td[-1]
    all_names = list(brca1)
    assert got["representative"] == {name: names[l] for name, l in zip(all_names, labels)}
    assert [got["distance"][name] for name in all_names] == fit.dist.tolist()
    assert all(got["representative"][r] == r and got["distance"][r] == 0.0 for r in names)


# ---- the schedule changes no bit

def _schedule_case(c):
    out = []
    for case in (next(x for x in kc.GENERAL_CASES if x.n == 300 and x.k == 33 and x.init == "given"),
                 next(x for x in kc.EXACT_CASES if x.n == 257 and x.k == 7 and x.init == "build" and x.family == "clustered"),
                 next(x for x in kc.EXACT_CASES if x.n == 65 and x.k == 1 and x.init == "given")):
        got = cluster.kmedoids(kc.case_matrix(case), case.k, init=init_of(case), max_swaps=case.max_swaps, ctx=c)
        assert np.array_equal(got.swaps, kc.case_ref(case).swaps)
        out += list(got)
    seqs = family_seqs(5, 8, 1500, seed=21)
    arrays = [seqs[s] for s in seqs]
    out += list(distance.jsd_kmedoids(arrays, 4, n_medoids=5, ctx=c))
    out += list(distance.mash_kmedoids(arrays, 8, 200, n_medoids=3, init="maxmin", ctx=c))
    with pytest.raises(ValueError, match="negative"):  # a failing call, then the same context again
        cluster.kmedoids(-np.ones((9, 9)), 2, ctx=c)
    out += list(distance.euclidean_kmedoids(arrays, 4, n_medoids=4, ctx=c))
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


@pytest.mark.parametrize("batch", kc.BATCHES)
def test_batch_length_changes_no_bit(monkeypatch, schedule_clean, batch):
    if batch is not None:
        monkeypatch.setenv("DVS_KMEDOIDS_BATCH", str(batch))
    assert same_result(_fresh(1)[0], schedule_clean)


def test_poisoned_blocks_change_no_bit(monkeypatch, schedule_clean):
    monkeypatch.setenv("DVS_TEST_KNOBS", POISON)
    first, again = _fresh(2)
    assert same_result(first, schedule_clean) and same_result(again, schedule_clean)


# ---- errors; the context stays usable after each

def _still_usable(ctx):
    got = cluster.kmedoids(kc.exact_matrix("random", 33, 9), 3, ctx=ctx)
    assert_is_ref(got, kc.kmedoids_ref(kc.exact_matrix("random", 33, 9), 3), "after an error")


def test_bad_entries(ctx):
    n = 65
    d = np.array(kc.exact_matrix("random", n, 11))
    for where in ((0, 1), (7, 2), (n - 1, n - 2)):
        for value, match in ((np.nan, "NaN or infinity"), (np.inf, "NaN or infinity"), (-np.inf, "NaN or infinity"),
                             (-0.5, "negative")):
            bad = d.copy()
            bad[where] = value
            for init in ("build", [3, 1]):
                with pytest.raises(ValueError, match=match) as err:
                    cluster.kmedoids(bad, 2, init=init, ctx=ctx)
                assert "dvs_kmedoids" in str(err.value)
        _still_usable(ctx)
    for value in (np.nan, np.inf, -1.0, 5.0):  # an entry on the diagonal is ignored
        weird = d.copy()
        weird[4, 4] = weird[n - 1, n - 1] = value
        assert same_result(cluster.kmedoids(weird, 3, ctx=ctx), cluster.kmedoids(d, 3, ctx=ctx))
    no_kmers = [np.full(50, 4, np.uint8), np.arange(50, dtype=np.uint8) % 4, np.ones(50, np.uint8), np.arange(50, dtype=np.uint8) % 3]
    for mode in ("euclidean", "jsd"):
        with pytest.raises(ValueError, match="NaN or infinity"):
            distance.KMEDOIDS_MODES[mode](no_kmers, 3, n_medoids=2, ctx=ctx)
    empty = [np.zeros(3, np.uint8), np.ones(2, np.uint8), np.arange(40, dtype=np.uint8) % 4]
    with pytest.raises(ZeroDivisionError):
        distance.mash_kmedoids(empty, 8, 10, n_medoids=2, ctx=ctx)
    _still_usable(ctx)
    one = distance.jsd_kmedoids([np.arange(40, dtype=np.uint8) % 4], 3, n_medoids=1, ctx=ctx)
    assert one.medoids.tolist() == [0] and one.labels.tolist() == [0] and one.td.tolist() == [0.0] and one.stop == 1
    assert cluster.kmedoids(np.zeros((1, 1)), 1, ctx=ctx).medoids.tolist() == [0]


def test_errors_c_boundary(ctx):
    L = ctx._L
    n = 9
    d = np.ascontiguousarray(kc.exact_matrix("random", n, 13))

    def given(count=n, on_device=0, handle=d.ctypes.data, rows=None):
        return distance.make_source(_lib.SRC_GIVEN, handle, count, rows, on_device=on_device)

    def call(src, k=2, init=0, max_swaps=10, medoids=None, count=n):
        return raw_call(ctx, src, count, k, init, max_swaps, medoids)[0]

    def fails(rc, code):
        assert rc == code
        assert b"dvs_kmedoids" in L.dvs_last_error(ctx._h), L.dvs_last_error(ctx._h)

    assert call(given()) == _lib.OK
    fails(call(given(), k=0), _lib.ERR_VALUE)
    fails(call(given(), k=n + 1), _lib.ERR_VALUE)
    fails(call(given(0, handle=None), count=1), _lib.ERR_VALUE)          # n == 0
    fails(call(given(), init=2), _lib.ERR_VALUE)
    fails(call(given(), init=1, medoids=[0, n]), _lib.ERR_VALUE)         # an initial medoid >= n
    fails(call(given(), init=1, medoids=[3, 3]), _lib.ERR_VALUE)         # repeated
    p = _lib.KmedoidsParams(2, 0, 10, 1)
    info = _lib.KmedoidsInfo()
    med, labels, dist = np.zeros(2, np.uint32), np.zeros(n, np.uint32), np.zeros(n)
    out = (med.ctypes.data_as(u32p), labels.ctypes.data_as(u32p), dist.ctypes.data_as(f64p))
    fails(L.dvs_kmedoids(ctx._h, given(), C.byref(p), *out, None, None, None, C.byref(info)), _lib.ERR_VALUE)  # flags
    p.flags = 0
    assert L.dvs_kmedoids(ctx._h, given(), C.byref(p), *out, None, None, None, C.byref(info)) == _lib.OK
    fails(L.dvs_kmedoids(ctx._h, given(), None, *out, None, None, None, C.byref(info)), _lib.ERR_VALUE)
    fails(L.dvs_kmedoids(ctx._h, given(), C.byref(p), None, out[1], out[2], None, None, None, C.byref(info)), _lib.ERR_VALUE)
    fails(L.dvs_kmedoids(ctx._h, given(), C.byref(p), out[0], None, out[2], None, None, None, C.byref(info)), _lib.ERR_VALUE)
    fails(L.dvs_kmedoids(ctx._h, given(), C.byref(p), out[0], out[1], None, None, None, None, C.byref(info)), _lib.ERR_VALUE)
    fails(L.dvs_kmedoids(ctx._h, given(), C.byref(p), *out, None, None, None, None), _lib.ERR_VALUE)
    fails(L.dvs_kmedoids(ctx._h, None, C.byref(p), *out, None, None, None, C.byref(info)), _lib.ERR_VALUE)
    fails(call(given(2000), k=1025, count=2000), _lib.ERR_UNSUPPORTED)   # (before the matrix is looked at)
    fails(call(given(), max_swaps=65536), _lib.ERR_UNSUPPORTED)
    assert call(given(on_device=1)) == _lib.ERR_VALUE                    # a host pointer said to be device memory
    fails(call(given(200_000), count=200_000), _lib.ERR_NOMEM)           # 320 GB of matrix
    m = ctx.build_matrix([np.arange(60, dtype=np.uint8) % 4, np.arange(70, dtype=np.uint8) % 3, np.ones(50, np.uint8)], 2, 4)
    try:
        listed = distance.make_source(_lib.SRC_JSD, m._h, 3, np.arange(3, dtype=np.uint32))
        fails(call(listed, count=3), _lib.ERR_UNSUPPORTED)               # a row list
        fails(call(distance.make_source(_lib.SRC_JSD, m._h, 2), count=2), _lib.ERR_UNSUPPORTED)  # some of the rows
        assert call(distance.make_source(_lib.SRC_JSD, m._h, 3), count=3) == _lib.OK
        fails(call(distance.make_source(_lib.SRC_EUCLIDEAN, m._h, 3), k=4, count=3), _lib.ERR_VALUE)
    finally:
        m.close()
    _still_usable(ctx)
