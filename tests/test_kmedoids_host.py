"""k-medoids without a GPU: the yardstick of tests/kmedoids_cases.py pinned three ways -- its final state is a
swap-local optimum by the long-double truth and no better than the brute-force optimum, its BUILD is the definition's
own loops, its special cases come out as include/dvs_hip.h says -- then the conditions every GPU case of
test_gpu_kmedoids.py rests on, asserted on the yardstick alone, the names of the feature, and every argument error of
the Python layer against a stand-in that fails the test when a context is touched."""
import itertools

import numpy as np
import pytest

from diverseseq_amd import _lib, apps, cluster, distance
import kmedoids_cases as kc
from test_cross_host import _NoContext


def _small(seed: int, n: int, symmetric: bool = True) -> np.ndarray:
    rng = np.random.default_rng([seed, n])
    D = rng.integers(1, 64, size=(n, n)) / 8.0
    if symmetric:
        D = np.triu(D, 1) + np.triu(D, 1).T
    np.fill_diagonal(D, np.nan)
    return D


def _td_of(D, med) -> float:
    return float(kc.state_of(kc.zero_diagonal(D), np.array(med, dtype=np.int64))[1].sum())


# ---- the yardstick

@pytest.mark.parametrize("n,k", [(n, k) for n in (2, 4, 6, 9) for k in (1, 2, 3) if k <= n])
@pytest.mark.parametrize("symmetric", (True, False))
def test_final_state_is_a_local_optimum_and_not_below_the_global_one(n, k, symmetric):
    for seed in range(4):
        D = _small(seed, n, symmetric)
        for init in ("build", np.arange(k)):
            ref = kc.kmedoids_ref(D, k, init)
            assert ref.stop == 1
            assert sorted(set(ref.medoids.tolist())) == sorted(ref.medoids.tolist())
            truth = kc.delta_truth(D, ref.medoids)
            assert not (truth < 0).any(), "an exchange still lowers td"
            best = min(_td_of(D, c) for c in itertools.combinations(range(n), k))
            assert ref.td[-1] >= best
            assert ref.td[-1] == _td_of(D, ref.medoids)
            assert (np.diff(ref.td) < 0).all()
            assert len(ref.td) == len(ref.swaps) + 1
            # every recorded exchange is the least Delta of its round by the truth (the entries are eighths: exact)
            med = ref.build.copy()
            for x, l in ref.swaps:
                t = kc.delta_truth(D, med)
                assert divmod(int(np.argmin(t)), k) == (x, l)
                med[l] = x
            assert (med == ref.medoids).all()


def test_split_deltas_are_the_truth_where_the_arithmetic_is_exact():
    for n, k in ((7, 2), (9, 3), (30, 5), (30, 1)):
        D = _small(5, n, symmetric=False)
        med = np.random.default_rng(n).permutation(n)[:k]
        D0 = kc.zero_diagonal(D)
        split = kc.round_deltas(D0, med, *kc.state_of(D0, med))
        truth = kc.delta_truth(D, med)
        assert (split == truth.astype(np.float64)).all()


@pytest.mark.parametrize("n,k", [(5, 1), (5, 5), (8, 3), (12, 4), (12, 11)])
def test_build_is_the_direct_loop(n, k):
    for seed in range(3):
        for symmetric in (True, False):
            D = _small(seed + 10, n, symmetric)
            assert kc.build_ref(kc.zero_diagonal(D), k).tolist() == kc.build_direct(D.tolist(), k)
    small = kc.exact_matrix("small_integer", n, 4)
    assert kc.build_ref(kc.zero_diagonal(small), k).tolist() == kc.build_direct(small.tolist(), k)


def test_special_cases_come_out_as_defined():
    D = _small(1, 6)
    one = kc.kmedoids_ref(D, 1)
    sums = np.nansum(D, axis=1)
    assert one.medoids.tolist() == [int(np.argmin(sums))] and one.td[-1] == sums.min()
    assert np.isinf(one.second).all() and (one.labels == 0).all() and one.stop == 1
    every = kc.kmedoids_ref(D, 6)
    assert sorted(every.medoids.tolist()) == list(range(6)) and every.stop == 1 and every.td.tolist() == [0.0]
    assert every.labels[every.medoids].tolist() == list(range(6)) and every.passes == 6 and len(every.swaps) == 0
    assert kc.kmedoids_ref(D, 6, np.arange(6), 0).stop == 1  # (k == n: converged at once, whatever max_swaps)
    zero = kc.kmedoids_ref(kc.exact_matrix("zero", 7, 1), 3)
    assert zero.medoids.tolist() == [0, 1, 2] and zero.td.tolist() == [0.0] and zero.stop == 1
    assert zero.labels.tolist() == [0, 1, 2, 0, 0, 0, 0]  # (equal distances: the lowest slot; a medoid: its own)
    const = kc.kmedoids_ref(kc.exact_matrix("constant", 7, 1), 2)
    assert const.medoids.tolist() == [0, 1] and const.td.tolist() == [7.5] and len(const.swaps) == 0
    assert const.labels.tolist() == [0, 1, 0, 0, 0, 0, 0] and (const.second[2:] == 1.5).all()
    # two copies of one row: the second copy is at distance 0, a medoid's own distance is 0 whatever the other's
    dup = _small(3, 5)
    dup = np.vstack([np.hstack([dup, dup[:, :1]]), np.hstack([dup[:1], [[np.nan]]])])
    dup[0, 5] = dup[5, 0] = 0.0
    ref = kc.kmedoids_ref(dup, 2, np.array([5, 0]), 0)
    assert ref.labels[0] == 1 and ref.labels[5] == 0 and ref.dist[0] == 0.0 and ref.second[0] == 0.0 and ref.stop == 0
    assert (ref.labels[1:5] == 0).all()  # (both medoids equally far: the lowest slot)
    scored = kc.kmedoids_ref(D, 2, np.array([4, 1]), 0)
    assert scored.medoids.tolist() == [4, 1] and scored.stop == 0 and scored.passes == 1 and len(scored.td) == 1


# ---- the conditions of the GPU cases

def test_exact_families_are_exact():
    assert max(c.n for c in kc.EXACT_CASES) <= 4096
    seen = set()
    for case in kc.EXACT_CASES:
        if (case.family, case.n, case.seed) in seen:
            continue
        seen.add((case.family, case.n, case.seed))
        D = kc.case_matrix(case)
        off = D[~np.eye(case.n, dtype=bool)]
        assert np.isnan(np.diag(D)).all(), "the diagonal must never be read"
        assert (off >= 0).all() and (off < 4).all() and (off * 1024 == np.round(off * 1024)).all(), case.id


def test_exact_cases_cover_the_grid():
    pairs = {(c.n, c.k) for c in kc.EXACT_CASES}
    for n in kc.SIZES:
        for k in kc.KS:
            k = min(k, n) if k == 1024 else k
            if k <= n:
                for init in ("build", "given"):
                    assert any(c.n == n and c.k == k and c.init == init for c in kc.EXACT_CASES), (n, k, init)
    assert {c.family for c in kc.EXACT_CASES} == set(kc.EXACT_FAMILIES)
    assert any(c.max_swaps == 0 for c in kc.EXACT_CASES)
    short = [c for c in kc.EXACT_CASES if 0 < c.max_swaps <= 2 and c.n == 257]
    assert short and any(kc.case_ref(c).stop == 0 and len(kc.case_ref(c).swaps) == c.max_swaps for c in short)
    assert len(pairs) >= 46


@pytest.mark.parametrize("case", kc.GENERAL_CASES, ids=lambda c: c.id)
def test_general_cases_have_their_gap(case):
    D, ref = kc.case_matrix(case), kc.case_ref(case)
    assert ref.stop == 1
    off = D[~np.eye(case.n, dtype=bool)]
    assert (off >= 0).all() and np.isfinite(off).all()
    swap_gap, build_gap, stop_gap = kc.gaps_of_run(D, ref, case.init == "build")
    b = kc.band(case.n, float(off.max()))
    assert swap_gap > 2 * b and build_gap > 2 * b and stop_gap > 2 * b, (swap_gap, build_gap, stop_gap, b)
    assert not (kc.delta_truth(D, ref.medoids) < -b).any()


# ---- the names

def test_the_names_exist():
    assert "dvs_kmedoids" in _lib.EXPORTS and "dvs_kmedoids" in apps.__all__
    for name in ("KMedoids", "check_kmedoids_args", "run_kmedoids", "matrix_kmedoids", "mash_kmedoids", "euclidean_kmedoids",
                 "jsd_kmedoids", "kmedoids"):
        assert hasattr(distance, name), name
    assert callable(distance.DeviceSide.kmedoids) and callable(distance.Sketches.kmedoids)
    assert set(distance.KMEDOIDS_MODES) == set(distance.DeviceSide.MODE_NAMES)
    for name in ("kmedoids", "representatives", "sampled_kmedoids"):
        assert callable(getattr(cluster, name)), name
    assert distance.KMedoids._fields == ("medoids", "labels", "dist", "second", "swaps", "td", "stop", "passes")
    assert (_lib.KMEDOIDS_INIT_BUILD, _lib.KMEDOIDS_INIT_GIVEN) == (0, 1)
    import ctypes as C
    assert C.sizeof(_lib.KmedoidsParams) == 16 and C.sizeof(_lib.KmedoidsInfo) == 32


def test_the_abi_version_is_5():
    import pathlib
    import re
    header = (pathlib.Path(__file__).resolve().parent.parent / "include" / "dvs_hip.h").read_text()
    assert re.search(r"#define\s+DVS_ABI_VERSION\s+5\b", header)
    assert "int dvs_kmedoids(dvs_ctx *ctx, const dvs_source *src" in header
    assert re.search(r"#define\s+DVS_KMEDOIDS_INIT_BUILD\s+0", header) and re.search(r"#define\s+DVS_KMEDOIDS_INIT_GIVEN\s+1", header)


# ---- the argument errors of the Python layer

BAD_ARGS = (  # (n_medoids, init, max_swaps, exception, match) over 5 rows
    (0, "build", 300, ValueError, "n_medoids"), (6, "build", 300, ValueError, "n_medoids"), (2.0, "build", 300, ValueError, "n_medoids"),
    (True, "build", 300, ValueError, "n_medoids"), (None, "build", 300, ValueError, "n_medoids"),
    (2, "build", -1, ValueError, "max_swaps"), (2, "build", 1.5, ValueError, "max_swaps"), (2, "build", None, ValueError, "max_swaps"),
    (2, "build", 65536, NotImplementedError, "max_swaps"),
    (2, "pam", 300, ValueError, "init"), (2, 7, 300, ValueError, "init"), (2, [0], 300, ValueError, "initial medoids"),
    (2, [0, 5], 300, ValueError, "outside"), (2, [-1, 0], 300, ValueError, "outside"), (2, [1, 1], 300, ValueError, "more than once"),
    (2, [0.5, 1.0], 300, ValueError, "row indices"), (2, [[0, 1]], 300, ValueError, "row indices"),
)


def test_check_kmedoids_args():
    assert distance.check_kmedoids_args(5, 2, "build", 300) == (2, "build", None, 300)
    assert distance.check_kmedoids_args(5, np.int64(5), "maxmin", 0) == (5, "maxmin", None, 0)
    k, kind, rows, ms = distance.check_kmedoids_args(5, 2, (4, 1), 7)
    assert (k, kind, ms) == (2, "given", 7) and rows.dtype == np.uint32 and rows.tolist() == [4, 1]
    for n_medoids, init, max_swaps, exc, match in BAD_ARGS:
        with pytest.raises(exc, match=match):
            distance.check_kmedoids_args(5, n_medoids, init, max_swaps)
    with pytest.raises(NotImplementedError, match="1024"):
        distance.check_kmedoids_args(3000, 1025, "build", 300)
    with pytest.raises(ValueError, match="at least one row"):
        distance.check_kmedoids_args(0, 1, "build", 300)


def test_argument_errors_need_no_context():
    ctx = _NoContext()
    a = [np.zeros(30, np.uint8), np.ones(30, np.uint8), np.arange(30, dtype=np.uint8) % 4, np.arange(30, dtype=np.uint8) % 3,
         np.arange(30, dtype=np.uint8) % 2]
    with pytest.raises(ValueError, match="Unexpected distance 'manhattan'"):
        distance.kmedoids(a, 2, "manhattan", k=3, ctx=ctx)
    with pytest.raises(ValueError, match="Expected sketch size"):
        distance.kmedoids(a, 2, "mash", k=3, ctx=ctx)
    with pytest.raises(ValueError, match="Sketch size"):
        distance.kmedoids(a, 2, "jsd", k=3, sketch_size=10, ctx=ctx)
    d = np.ones((5, 5))
    for n_medoids, init, max_swaps, exc, match in BAD_ARGS:
        with pytest.raises(exc, match=match):
            distance.kmedoids(a, n_medoids, "jsd", k=3, init=init, max_swaps=max_swaps, ctx=ctx)
        with pytest.raises(exc, match=match):
            distance.mash_kmedoids(a, 3, 10, n_medoids=n_medoids, init=init, max_swaps=max_swaps, ctx=ctx)
        with pytest.raises(exc, match=match):
            distance.jsd_kmedoids(a, 3, n_medoids=n_medoids, init=init, max_swaps=max_swaps, ctx=ctx)
        with pytest.raises(exc, match=match):
            distance.euclidean_kmedoids(a, 3, n_medoids=n_medoids, init=init, max_swaps=max_swaps, ctx=ctx)
        with pytest.raises(exc, match=match):
            cluster.kmedoids(d, n_medoids, init=init, max_swaps=max_swaps, ctx=ctx)
        with pytest.raises(exc, match=match):
            cluster.representatives({str(i): s for i, s in enumerate(a)}, n_medoids, k=3, distance_mode="jsd", sketch_size=None,
                                    init=init, max_swaps=max_swaps)
    with pytest.raises(ValueError, match="square"):
        cluster.kmedoids(np.ones((3, 4)), 2, ctx=ctx)
    seqs = {str(i): s for i, s in enumerate(a)}
    with pytest.raises(ValueError, match="n_medoids"):
        cluster.sampled_kmedoids(seqs, 4, 3, k=3, distance_mode="jsd", sketch_size=None)
    with pytest.raises(ValueError, match="n_select"):
        cluster.sampled_kmedoids(seqs, 2, 6, k=3, distance_mode="jsd", sketch_size=None)
    with pytest.raises(ValueError, match="Unexpected distance"):
        cluster.sampled_kmedoids(seqs, 2, 3, k=3, distance_mode="manhattan")

    class _Matrix:
        nrows, ctx = 5, _NoContext()

    with pytest.raises(ValueError, match="Unexpected distance 'mash'"):
        distance.matrix_kmedoids(_Matrix(), 2, mode="mash")
    with pytest.raises(ValueError, match="n_medoids"):
        distance.matrix_kmedoids(_Matrix(), 6)
    with pytest.raises(ValueError, match="init"):
        distance.DeviceSide(_Matrix(), "jsd").kmedoids(2, init="pam")


def test_app_constructor_checks():
    app = apps.dvs_kmedoids(3, "jsd", k=4)
    assert app._n == 3 and app._init == "build" and app._max_swaps == 300
    for kwargs, match in ((dict(n=0), "n must be"), (dict(n=True), "n must be"), (dict(n=1.5), "n must be"), (dict(n=1025), "n must be"),
                          (dict(n=2, init="pam"), "init"), (dict(n=2, init=[0, 1]), "init"), (dict(n=2, max_swaps=-1), "max_swaps"),
                          (dict(n=2, max_swaps=65536), "max_swaps"), (dict(n=2, distance_mode="manhattan"), "Unexpected distance"),
                          (dict(n=2, distance_mode="mash", canonical=True), "Canonical")):
        with pytest.raises(ValueError, match=match):
            apps.dvs_kmedoids(**kwargs)
