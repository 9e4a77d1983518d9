"""PERMANOVA without a GPU: the yardstick of tests/permanova_cases.py pinned against independent statements of the same
statistic, the conditions every case of tests/test_gpu_permanova.py rests on, the rule of the permutations, the argument
checks of the Python layer, and the boundary (the header declares dvs_permanova, _lib lists it, the ABI is still 5)."""
import pathlib
import re

import numpy as np
import pytest

import permanova_cases as pc
from diverseseq_amd import _lib, apps, cluster, distance

ROOT = pathlib.Path(__file__).resolve().parent.parent


# ---- the yardstick against independent statements

@pytest.mark.parametrize("n,a,seed", [(12, 2, 0), (60, 3, 1), (200, 7, 2)])
def test_f_is_anovas_f_for_points_on_a_line(n, a, seed):
    """one-dimensional points with euclidean distances: PERMANOVA's pseudo-F is the F of a one-way ANOVA"""
    from scipy.stats import f_oneway

    rng = np.random.default_rng(seed)
    lab = pc.encode(np.concatenate([np.arange(a), rng.integers(0, a, n - a)]).tolist())
    x = rng.normal(size=n) + 0.7 * lab
    ref = pc.permanova_ref(np.abs(x[:, None] - x[None, :]), lab, a, np.zeros((0, n), np.uint32))
    want = f_oneway(*[x[lab == g] for g in range(a)]).statistic
    assert abs(ref.f[0] - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("n,a,d,seed", [(30, 3, 2, 3), (150, 6, 5, 4)])
def test_ss_within_is_the_squared_distance_to_the_centroids(n, a, d, seed):
    rng = np.random.default_rng(seed)
    lab = pc.encode(np.concatenate([np.arange(a), rng.integers(0, a, n - a)]).tolist())
    x = rng.normal(size=(n, d)) + rng.normal(size=(a, d))[lab]
    D = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
    ss_total, ss_within, group_ss = pc.sums(D, lab, a, np.zeros((0, n), np.uint32))
    per_group = np.array([((x[lab == g] - x[lab == g].mean(axis=0)) ** 2).sum() for g in range(a)])
    assert np.allclose(group_ss, per_group, rtol=1e-11, atol=0)
    assert abs(ss_within[0] - per_group.sum()) <= 1e-11 * per_group.sum()
    assert abs(ss_total - ((x - x.mean(axis=0)) ** 2).sum()) <= 1e-11 * ss_total


def test_renaming_the_groups_changes_nothing():
    case = next(c for c in pc.REAL_CASES if c.n == 300)
    D, lab = pc.case_matrix(case), pc.case_labels(case).astype(np.int64)
    rename = np.random.default_rng(5).permutation(case.a)
    one = pc.sums(D, lab, case.a, pc.case_perms(case)[:3])
    two = pc.sums(D, rename[lab], case.a, rename[pc.case_perms(case)[:3].astype(np.int64)])
    assert one[0] == two[0] and np.array_equal(one[1], two[1]) and np.array_equal(one[2], two[2][rename])
    assert np.array_equal(one[0] - one[1], two[0] - two[1])


def test_statistics_at_the_edges():
    ssa, f, r2 = pc.statistics(10, 3, 5.0, np.array([0.0, 5.0, 2.0]))
    assert f[0] == np.inf and f[1] == 0.0 and f[2] == (3.0 / 2) / (2.0 / 7) and r2[0] == 1.0
    assert np.isnan(pc.statistics(10, 3, 0.0, np.array([0.0]))[1]).all()
    got = distance.permanova_statistics(10, 3, 5.0, np.array([0.0, 5.0, 2.0]))
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(got, (ssa, f, r2)))
    assert np.isnan(distance.permanova_statistics(10, 3, 0.0, np.array([0.0]))[1]).all()


# ---- the cases

def test_the_cases_cover_what_the_device_tests_need():
    ns = {c.n for c in pc.EXACT_CASES}
    assert set(pc.SIZES) | set(pc.BOUND_SIZES) <= ns
    for bound in (pc.UNROLL, pc.WAVE, pc.TILE_ROWS, pc.TILE_COLS, pc.ENTRY_CHUNK):
        assert {bound, bound + 1} <= ns, bound
    tiles = lambda n: -(-n // pc.TILE_COLS) * -(-n // pc.TILE_ROWS)  # noqa: E731
    assert tiles(2816) <= pc.FINAL_THREADS < tiles(2817) and {2816, 2817} <= ns
    assert {c.a for c in pc.EXACT_CASES} >= {2, 3, 16, 255, 256, 257} and any(c.a == c.n - 1 for c in pc.EXACT_CASES)
    B = pc.DEFAULT_BATCH
    assert {c.P for c in pc.EXACT_CASES} >= {0, 1, B - 1, B, B + 1, 3 * B + 5} == set(pc.PERMS)
    assert len({c.id for c in pc.EXACT_CASES + pc.REAL_CASES}) == len(pc.EXACT_CASES) + len(pc.REAL_CASES)
    for c in pc.EXACT_CASES:
        sizes = np.bincount(pc.case_labels(c), minlength=c.a)
        assert sizes.sum() == c.n and (sizes > 0).all() and (sizes & (sizes - 1) == 0).all(), c.id
    assert any((np.bincount(pc.case_labels(c)) == 1).any() and (np.bincount(pc.case_labels(c)) > 1).any() for c in pc.EXACT_CASES)


@pytest.mark.parametrize("case", pc.EXACT_CASES, ids=lambda c: c.id)
def test_exact_families_have_one_answer(case):
    """small integers and power-of-two groups: the float64 yardstick and the long-double run agree as arrays"""
    D = pc.case_matrix(case)
    assert np.array_equal(D, np.round(D)) and D.min() >= 0 and D.max() < 8
    ref, truth = pc.case_ref(case), pc.case_truth(case)
    assert ref.ss_within.shape == (case.P + 1,) and ref.group_ss.shape == (case.a,)
    assert np.array_equal(ref.ss_within.astype(np.longdouble), truth[1])
    assert np.array_equal(ref.group_ss.astype(np.longdouble), truth[2])
    assert abs(np.longdouble(ref.ss_total) - truth[0]) <= 2.0 ** -53 * truth[0]  # (one division by n, rounded once)
    assert ref.ss_within[0] == pc.chain(ref.group_ss, np.float64)
    for p in range(case.P):
        assert np.array_equal(np.bincount(pc.case_perms(case)[p], minlength=case.a), np.bincount(pc.case_labels(case)))


@pytest.mark.parametrize("case", pc.REAL_CASES, ids=lambda c: c.id)
def test_real_cases_have_a_unique_count(case):
    """no permutation's SS_W within twice the band of the observed one, by the long-double truth, unless it makes the
    observed partition: n_le and p are then the same for every evaluation that keeps within the band"""
    truth = pc.case_truth(case)[1]
    lab, perms = pc.case_labels(case), pc.case_perms(case)
    limit = 2 * pc.band(case.n)
    for p in range(case.P):
        if np.array_equal(pc.encode(perms[p].tolist()), lab):
            continue
        gap = abs(truth[p + 1] - truth[0])
        assert gap > limit * max(truth[p + 1], truth[0]), (case.id, p, float(gap))
    ref = pc.case_ref(case)
    assert np.all(np.abs(ref.ss_within.astype(np.longdouble) - truth) <= pc.band(case.n) * truth)
    assert ref.n_le == int((truth[1:] <= truth[0]).sum())


# ---- the rule of the permutations and the argument checks of the Python layer

def test_permutations_follow_the_documented_rule():
    lab = pc.encode(list("aabbbcccdd" * 3))
    strata = pc.encode([i % 4 for i in range(30)])
    for seed in (0, 11):
        assert np.array_equal(distance.permuted_labels(lab, 7, seed), pc.documented_permutations(lab, 7, seed))
        got = distance.permuted_labels(lab, 7, seed, strata)
        assert np.array_equal(got, pc.documented_permutations(lab, 7, seed, strata))
        for row in got:
            for s in range(4):  # every block keeps its own labels
                assert sorted(row[strata == s].tolist()) == sorted(lab[strata == s].tolist())
        assert not np.array_equal(got, distance.permuted_labels(lab, 7, seed))
    rng = np.random.default_rng(3)
    first = rng.permutation(30)
    assert np.array_equal(distance.permuted_labels(lab, 2, 3)[0], lab[first])
    assert np.array_equal(distance.permuted_labels(lab, 2, 3)[1], lab[rng.permutation(30)])
    assert distance.permuted_labels(lab, 0, 3).shape == (0, 30)


def test_grouping_is_encoded_in_order_of_first_appearance():
    lab, names = distance.encode_grouping(["site B", "site A", "site B", ("x", 1), "site A"], 5)
    assert lab.tolist() == [0, 1, 0, 2, 1] and names == ["site B", "site A", ("x", 1)] and lab.dtype == np.uint32
    assert distance.encode_grouping(np.array([3, 3, 1]), 3)[0].tolist() == [0, 0, 1]
    labels, a, perms = distance.check_permanova_args(5, ["u", "v", "u", "v", "w"], 4, 9, None)
    assert (labels.tolist(), a, perms.shape, perms.dtype) == ([0, 1, 0, 1, 2], 3, (4, 5), np.uint32)


def test_argument_errors_before_any_device_work():
    ok = list("aabbc")
    for n, grouping, kw in ((2, "ab", {}), (5, list("aaaaa"), {}), (5, list("abcde"), {}), (5, list("aabb"), {}),
                            (5, "aabbc", {}), (5, 7, {}), (5, ok, {"permutations": -1}), (5, ok, {"permutations": 2.5}),
                            (5, ok, {"permutations": True}), (5, ok, {"strata": [0, 1]}), (5, [[1], [2], [1], [2], [1]], {})):
        args = dict(permutations=9, seed=0, strata=None)
        args.update(kw)
        with pytest.raises(ValueError):
            distance.check_permanova_args(n, list(grouping) if isinstance(grouping, str) and n == 2 else grouping, **args)
    with pytest.raises(ValueError):
        cluster.permanova(np.zeros((4, 5)), list("aabb"))
    with pytest.raises(ValueError):
        cluster.permanova(np.zeros((4, 4)), list("aab"))
    with pytest.raises(ValueError, match="Unexpected distance"):
        distance.permanova([b"\x00\x01"] * 4, list("aabb"), "hamming", k=2)
    with pytest.raises(ValueError, match="Expected sketch size"):
        distance.permanova([b"\x00\x01"] * 4, list("aabb"), "mash", k=2)
    with pytest.raises(ValueError):
        apps.dvs_permanova(list("aabb"))
    with pytest.raises(ValueError):
        apps.dvs_permanova({"s": 1}, permutations=-3)
    app = apps.dvs_permanova({"s1": "x", "s2": "y"}, "jsd", k=4, permutations=5, seed=2)
    assert (app._k, app._sketch_size, app._distance_mode, app._permutations) == (4, None, "jsd", 5)


# ---- the boundary

def test_the_boundary_declares_the_entry():
    header = (ROOT / "include" / "dvs_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    found = re.findall(r"\bint\s+dvs_permanova\s*\(([^)]*)\)\s*;", text)
    assert len(found) == 1 and re.match(r"\s*dvs_ctx\s*\*\s*ctx\s*,\s*const\s+dvs_source\s*\*", found[0])
    assert re.search(r"typedef struct dvs_permanova_info \{\s*uint32_t n_le, passes, batch;\s*\} dvs_permanova_info;", header)
    assert re.search(r"#define\s+DVS_ABI_VERSION\s+5\b", header)
    assert "dvs_permanova" in _lib.EXPORTS and "dvs_permanova" in apps.__all__ and callable(apps.dvs_permanova)
    assert [n for n, _ in _lib.PermanovaInfo._fields_] == ["n_le", "passes", "batch"]
    lib = _lib.load()
    assert lib.dvs_abi_version() == 5 and hasattr(lib, "dvs_permanova")
    assert lib.dvs_permanova.argtypes[1] == __import__("ctypes").POINTER(_lib.Source)
    csrc = ROOT / "diverseseq_amd" / "csrc"
    assert "permanova.hip" in (csrc / "Makefile").read_text()
    assert "DVS_PERMANOVA_BATCH" in (csrc / "api.cpp").read_text() and "DVS_PERMANOVA_BATCH" in (ROOT / "INTEGRATION.md").read_text()
    kernel = (csrc / "permanova.hip").read_text()
    for name, value in (("PV_ROWS", pc.TILE_ROWS), ("PV_UNROLL", pc.UNROLL), ("PV_BATCH", pc.DEFAULT_BATCH),
                        ("PV_MAX_BATCH", pc.MAX_BATCH), ("PV_MAX_GROUPS", pc.MAX_GROUPS), ("PV_THREADS", pc.TILE_COLS)):
        assert re.search(rf"constexpr \w+ {name} = {value};", kernel), name
    assert pc.FINAL_THREADS == pc.TILE_COLS and f"64 * PV_UNROLL" in kernel and pc.ENTRY_CHUNK == 64 * pc.UNROLL
    assert "atomicAdd" not in kernel  # no floating-point atomic
    for cls in (distance.DeviceSide, distance.Sketches):
        assert callable(getattr(cls, "permanova"))
    assert "permanova" in vars(distance.DeviceSide)  # (defined there, as every operation is)
    assert set(distance.PERMANOVA_MODES) == {"mash", "euclidean", "jsd"}
    assert distance.PERMANOVA._fields == ("f", "p_value", "r2", "ss_total", "ss_within", "ss_among", "group_ss", "group_sizes",
                                          "perm_f", "permutations")
