"""The yardstick and the cases of the Mantel tests (mantel_cases.py), pinned without a GPU: the yardstick's r against
scipy.stats.pearsonr over explicitly permuted matrices and its counts against a plain loop; the condition every case
states; the rule of the permutations held to distance.permuted_labels; every argument error of the Python layer, raised
before any device work; and the boundary -- the header, the exports, the ABI version, the Makefile, the knob -- with the
import graph of the new module."""
import ast
import re
import types

import numpy as np
import pytest
import scipy.stats

from conftest import ROOT
from diverseseq_amd import _lib, apps, cluster, distance, engine, mantel
import mantel_cases as mc


# ---- the yardstick

def permuted_copy(Y, pi):
    """Y with its items permuted, as a full symmetric matrix: cell (i, j) is y(pi[i], pi[j])"""
    return mc.symmetric_from_upper(Y)[np.ix_(pi, pi)]


@pytest.mark.parametrize("case", [c for c in mc.REAL_CASES if c.n <= 300] + [c for c in mc.EXACT_CASES if c.id in ("plain-n65-P33", "ties-n65-P33")],
                         ids=lambda c: c.id)
def test_r_is_pearsons_r_of_the_permuted_cells(case):
    X, Y = mc.case_matrices(case)
    perms = mc.case_perms(case)
    r = mc.case_stats(case).r
    x = mc.upper_cells(X)
    rows = [np.arange(case.n), *perms.astype(np.int64)]
    for p in (0, 1, 2, len(rows) - 1):
        want = scipy.stats.pearsonr(x, mc.upper_cells(permuted_copy(Y, rows[p])))[0]
        assert abs(r[p] - want) <= 1e-11, (case.id, p, r[p], want)
    assert abs(np.longdouble(r[0]) - mc.pearson_truth(X, Y)) <= 4 * mc.band(case.n)


def test_counts_are_a_plain_loop():
    for case in (mc.REAL_CASES[0], next(c for c in mc.EXACT_CASES if c.id == "ties-n65-P33"),
                 next(c for c in mc.EXACT_CASES if c.id == "identity-n65-P33")):
        s, st = mc.case_sums(case), mc.case_stats(case)
        c0 = (float(s.A) * float(s.B)) / mc.pairs_of(case.n)
        ge = le = ab = 0
        for zp in s.z[1:]:
            ge += zp >= s.z[0]
            le += zp <= s.z[0]
            ab += abs(zp - c0) >= abs(s.z[0] - c0)
        assert (st.n_ge, st.n_le, st.n_abs_ge) == (ge, le, ab), case.id
        assert st.p_value == {"two-sided": (1 + ab) / (1 + case.P), "greater": (1 + ge) / (1 + case.P),
                              "less": (1 + le) / (1 + case.P)}
    identity = next(c for c in mc.EXACT_CASES if c.id == "identity-n65-P33")
    assert mc.case_stats(identity).n_ge >= 4 and mc.case_stats(identity).n_le >= 4  # the identity counts towards p
    none = next(c for c in mc.EXACT_CASES if c.P == 0)
    assert all(np.isnan(p) for p in mc.case_stats(none).p_value.values())


# ---- the cases' conditions

def test_the_case_lists():
    ids = [c.id for c in mc.EXACT_CASES + mc.REAL_CASES]
    assert len(set(ids)) == len(ids)
    assert {c.n for c in mc.EXACT_CASES} == set(mc.SIZES + mc.BOUND_SIZES)
    for bound in (mc.WAVE, mc.ROW_CHUNK, mc.SCORE_THREADS, mc.SCORE_CHUNK, mc.FINAL_THREADS):  # both sides of every bound
        sizes = {c.n for c in mc.EXACT_CASES}
        assert bound in sizes and bound + 1 in sizes and (bound - 1 in sizes), bound
    for n in (65, 257):
        assert {c.P for c in mc.EXACT_CASES if c.n == n and c.family == "plain"} >= set(mc.PERMS)
    assert {c.family for c in mc.EXACT_CASES} == set(mc.SUB_FAMILIES)
    assert all(c.P == mc.LARGE_PERMS for c in mc.EXACT_CASES if c.n >= mc.LARGE)
    assert {(c.family, c.n) for c in mc.REAL_CASES} == {(f, n) for f in mc.REAL_FAMILIES for n in (40, 300, 1025)}


@pytest.mark.parametrize("case", mc.EXACT_CASES, ids=lambda c: c.id)
def test_exact_cases_are_exact(case):
    X, Y = mc.case_matrices(case)
    n, m = case.n, mc.pairs_of(case.n)
    assert np.isnan(X[np.tril_indices(n)]).all() and np.isnan(Y[np.tril_indices(n)]).all()
    for M in (X, Y):
        cells = mc.upper_cells(M)
        c = cells.sum() / m
        assert c == round(c) and (cells == np.round(cells)).all() and np.abs(cells - c).max() <= 256 and cells.min() >= 0
    s64, sld = mc.case_sums(case), mc.sums(X, Y, mc.case_perms(case), np.longdouble)
    assert (s64.s_x, s64.s_y) == (sld.s_x, sld.s_y) and s64.A == 0 and s64.B == 0
    assert np.array_equal(s64.moments, sld.moments) and np.array_equal(s64.z, sld.z.astype(np.float64))
    assert (s64.z == np.round(s64.z)).all() and np.abs(s64.z).max() < 2.0 ** 52
    st = mc.case_stats(case)
    if case.family == "same":
        assert st.r[0] == 1.0
    if case.family == "negated":
        assert st.r[0] == -1.0
    if case.family == "constant":
        assert np.isnan(st.r).all() and all(np.isnan(p) for p in st.p_value.values())
    if case.family == "identity":
        perms = mc.case_perms(case)
        at = [p for p in range(case.P) if np.array_equal(perms[p], np.arange(n))]
        assert len(at) >= 4 and all(s64.z[p + 1] == s64.z[0] for p in at)
        assert {0, mc.DEFAULT_BATCH - 1, mc.DEFAULT_BATCH} <= set(at)  # vectors 1, B and B + 1: the end of a batch, the start of the next
    if case.family == "automorph":
        perms = mc.case_perms(case)
        assert not np.array_equal(perms[2], np.arange(n)) and s64.z[3] == s64.z[0]
        ysym = mc.symmetric_from_upper(Y)
        assert np.array_equal(ysym[np.ix_(perms[2], perms[2])], ysym)
    if case.family == "stratified":
        strata = mc.case_strata(case)
        assert all(np.array_equal(strata[row], strata) for row in mc.case_perms(case))
    if case.family == "ties":
        assert set(np.unique(mc.upper_cells(X) - mc.CX)) <= {-1.0, 0.0, 1.0}


@pytest.mark.parametrize("case", mc.REAL_CASES, ids=lambda c: c.id)
def test_real_cases_have_unique_counts(case):
    """no permuted Z within 2 band sqrt(S_uu S_vv) of Z(id), or of its mirror about c0"""
    s = mc.case_sums(case)
    n = case.n
    gap = 2 * mc.band(n) * np.sqrt(float(s.S_uu) * float(s.S_vv))
    c0 = float(s.A) * float(s.B) / mc.pairs_of(n)
    z = np.asarray(s.z, dtype=np.float64)
    assert np.abs(z[1:] - z[0]).min() > gap
    assert np.abs(np.abs(z[1:] - c0) - abs(z[0] - c0)).min() > gap
    r = mc.case_stats(case).r
    assert 0.05 < r[0] < 0.999 and np.abs(r[1:]).max() < r[0]  # correlated, and no permutation as much
    if case.family == "crowded":
        cells = mc.upper_cells(mc.case_matrices(case)[0])
        assert (cells.max() - cells.min()) / cells.mean() <= 1e-3
    # the float64 yardstick is itself within the band of the long-double truth over its own shifts
    X, Y = mc.case_matrices(case)
    truth = mc.sums(X, Y, mc.case_perms(case), np.longdouble, shifts=(s.s_x, s.s_y))
    mag = mc.magnitudes(X, Y, mc.case_perms(case), (s.s_x, s.s_y))
    for name in ("A", "B", "S_uu", "S_vv"):
        assert abs(np.longdouble(getattr(s, name)) - getattr(truth, name)) <= mc.band(n) * getattr(mag, name), name
    assert (np.abs(z.astype(np.longdouble) - truth.z) <= mc.band(n) * mag.z).all()


# ---- the rule of the permutations

def test_permutations_follow_the_rule_of_permuted_labels():
    rng = np.random.default_rng(5)
    for n, P, seed, strata in ((7, 4, 0, None), (40, 9, 11, None), (33, 6, 3, np.arange(33) % 5), (12, 5, 8, list("aabbccaabbcc"))):
        got = mantel.permutations(n, P, seed, strata)
        assert got.dtype == np.uint32 and got.shape == (P, n)
        assert all(sorted(row.tolist()) == list(range(n)) for row in got)
        blocks = None if strata is None else np.unique(np.asarray(strata), return_inverse=True)[1]
        assert np.array_equal(got, mc.documented_permutations(n, P, seed, blocks))
        labels = rng.integers(0, 5, n).astype(np.uint32)
        codes = None if strata is None else distance.encode_grouping(strata, n, "strata")[0]
        assert np.array_equal(distance.permuted_labels(labels, P, seed, codes), labels[got])
        if strata is not None:
            assert all(np.array_equal(np.asarray(strata)[row], np.asarray(strata)) for row in got)
    assert mantel.permutations(5, 0).shape == (0, 5)


def test_statistics_of_the_python_layer_are_the_yardsticks():
    for case in (mc.REAL_CASES[0], next(c for c in mc.EXACT_CASES if c.id == "constant-n65-P33"),
                 next(c for c in mc.EXACT_CASES if c.id == "same-n65-P33")):
        s = mc.case_sums(case)
        got = mantel.mantel_statistics(case.n, s.moments, s.z)
        assert got.dtype == np.float64 and np.array_equal(got, mc.case_stats(case).r, equal_nan=True), case.id


# ---- the argument errors of the Python layer, before any device work

def fake_side(n, ctx):
    handle = types.SimpleNamespace(nrows=n, _h=None, ctx=ctx)
    return distance.DeviceSide(handle, "jsd")


def test_argument_errors_before_any_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device work")

    monkeypatch.setattr(mantel, "run_mantel", no_device)
    monkeypatch.setattr(engine, "default_context", no_device)
    five, six = np.ones((5, 5)), np.ones((6, 6))
    with pytest.raises(ValueError, match="alternative"):
        mantel.mantel(five, five, alternative="both")
    for bad in (-1, 2.5, True, None):
        with pytest.raises(ValueError, match="permutations"):
            mantel.mantel(five, five, permutations=bad)
    with pytest.raises(ValueError, match="5 rows against one of 6"):
        mantel.mantel(five, six)
    with pytest.raises(ValueError, match="three"):
        mantel.mantel(np.ones((2, 2)), np.ones((2, 2)))
    with pytest.raises(ValueError, match="square"):
        mantel.mantel(np.ones((3, 4)), five)
    with pytest.raises(ValueError, match="4 values of strata for 5 rows"):
        mantel.mantel(five, five, strata=[0, 1, 0, 1])
    a, b = object(), object()
    with pytest.raises(ValueError, match="one context"):
        mantel.mantel(fake_side(5, a), fake_side(5, b))
    with pytest.raises(ValueError, match="one context"):
        mantel.mantel(fake_side(5, a), five, ctx=b)
    with pytest.raises(ValueError, match="5 rows against one of 6"):
        mantel.mantel(fake_side(5, a), fake_side(6, a))
    seqs = [np.arange(30, dtype=np.uint8) % 4] * 4
    jsd, mash = {"distance_mode": "jsd", "k": 3}, {"distance_mode": "mash", "k": 5, "sketch_size": 20}
    with pytest.raises(ValueError, match="Expected sketch size"):
        mantel.of_sequences(seqs, jsd, {"distance_mode": "mash", "k": 5})
    with pytest.raises(ValueError, match="Sketch size should only"):
        mantel.of_sequences(seqs, {**jsd, "sketch_size": 10}, mash)
    with pytest.raises(ValueError, match="Unexpected distance"):
        mantel.of_sequences(seqs, {"distance_mode": "hamming", "k": 3}, mash)
    with pytest.raises(ValueError, match="unknown key"):
        mantel.of_sequences(seqs, {**jsd, "kk": 3}, mash)
    with pytest.raises(ValueError, match="x_mode"):
        mantel.of_sequences(seqs, "jsd", mash)
    with pytest.raises(ValueError, match="three"):
        mantel.of_sequences(seqs[:2], jsd, mash)
    with pytest.raises(ValueError, match="alternative"):
        mantel.of_sequences(seqs, jsd, mash, alternative="more")
    with pytest.raises(ValueError, match="permutations"):
        mantel.of_sequences(seqs, jsd, mash, permutations=-3)
    with pytest.raises(ValueError, match="strata"):
        mantel.of_sequences(seqs, jsd, mash, strata=[1, 2])
    # the app checks its modes when it is made
    mantel.dvs_mantel({"distance_mode": "jsd", "k": 4}, {"distance_mode": "mash", "k": 8, "sketch_size": 100})
    with pytest.raises(ValueError, match="Unexpected distance"):
        mantel.dvs_mantel({"distance_mode": "x"}, mash)
    with pytest.raises(ValueError, match="Expected sketch size"):
        mantel.dvs_mantel(jsd, {"distance_mode": "mash", "sketch_size": None})
    with pytest.raises(ValueError, match="alternative"):
        mantel.dvs_mantel(jsd, mash, alternative="up")
    with pytest.raises(ValueError, match="permutations"):
        mantel.dvs_mantel(jsd, mash, permutations=-1)
    with pytest.raises(ValueError, match="y_mode"):
        mantel.dvs_mantel(jsd, None)


# ---- the boundary

def test_the_c_boundary():
    header = (ROOT / "include" / "dvs_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    found = re.findall(r"\bint\s+dvs_mantel\s*\(([^)]*)\)\s*;", text)
    assert len(found) == 1, found
    assert re.match(r"\s*dvs_ctx\s*\*\s*ctx\s*,\s*const\s+dvs_source\s*\*\s*x\s*,\s*const\s+dvs_source\s*\*\s*y\s*,", found[0]), found[0]
    assert re.search(r"typedef\s+struct\s+dvs_mantel_info\s*\{\s*uint32_t\s+n_ge,\s*n_le,\s*n_abs_ge,\s*passes,\s*batch;", text)
    assert "dvs_mantel" in _lib.EXPORTS and _lib.EXPORTS.count("dvs_mantel") == 1
    assert [f[0] for f in _lib.MantelInfo._fields_] == ["n_ge", "n_le", "n_abs_ge", "passes", "batch"]
    assert re.search(r"#define\s+DVS_ABI_VERSION\s+5\b", header) or "dvs_abi_version() != 5" in (ROOT / "diverseseq_amd" / "_lib.py").read_text()
    assert _lib.load().dvs_abi_version() == 5 and hasattr(_lib.load(), "dvs_mantel")
    makefile = (ROOT / "diverseseq_amd" / "csrc" / "Makefile").read_text()
    assert re.search(r"^SRCS\s*=.*\bmantel\.hip\b", makefile, flags=re.M)
    api = (ROOT / "diverseseq_amd" / "csrc" / "api.cpp").read_text()
    internal = (ROOT / "diverseseq_amd" / "csrc" / "dvs_internal.h").read_text()
    integration = (ROOT / "INTEGRATION.md").read_text()
    knob = "DVS_MANTEL_BATCH"
    assert f'getenv("{knob}")' in api and knob in internal and f"`{knob}`" in integration
    # no runtime allocation call outside api.cpp
    assert not re.search(r"\bhip(Malloc|Free|HostMalloc|HostFree|MallocAsync|FreeAsync)\w*\s*\(", (ROOT / "diverseseq_amd" / "csrc" / "mantel.hip").read_text())


def test_nothing_imports_the_module_back():
    """diverseseq_amd.mantel imports downwards; no module of the package imports it"""
    pkg = ROOT / "diverseseq_amd"
    for py in pkg.rglob("*.py"):
        if py == pkg / "mantel.py":
            continue
        for node in ast.walk(ast.parse(py.read_text())):
            if isinstance(node, ast.Import):
                assert not any(a.name.endswith(".mantel") or a.name == "mantel" for a in node.names), py
            elif isinstance(node, ast.ImportFrom):
                assert (node.module or "").split(".")[-1] != "mantel", py
                assert not any(a.name == "mantel" for a in node.names), py
    imported = {a.name for node in ast.walk(ast.parse((pkg / "mantel.py").read_text())) if isinstance(node, ast.ImportFrom)
                and node.level == 1 and node.module is None for a in node.names}
    assert imported == {"_lib", "apps", "cluster", "distance", "engine"}


def test_the_public_names_of_the_layers_below_are_untouched():
    for mod in (distance, cluster, apps, engine):
        for name, value in vars(mod).items():
            assert name != "mantel" and getattr(value, "__module__", None) != "diverseseq_amd.mantel", (mod.__name__, name)
        assert not any("mantel" in name.lower() for name in dir(mod)), mod.__name__
    assert "dvs_mantel" not in apps.__all__
    assert "mantel" not in (ROOT / "pyproject.toml").read_text()
