"""The minimum spanning tree without a GPU: the yardsticks of tests/mst_cases.py pinned against each other and against
scipy, dvs_linkage_from_mst (host only) against scipy's single linkage, the names the feature adds, and the argument
checks of the Python layer and of the app, all of which come before any device work."""
import ctypes as C
import re

import numpy as np
import pytest
from scipy.cluster.hierarchy import linkage as scipy_linkage
from scipy.sparse.csgraph import minimum_spanning_tree as scipy_mst

import mst_cases as mc
from conftest import ROOT
from diverseseq_amd import _lib, apps, cluster, distance

PIN_SIZES = (2, 3, 64, 65, 257)  # (the yardsticks at the larger sizes are computed by the GPU tests that use them)


def condensed(d):
    return np.asarray(d)[np.triu_indices(d.shape[0], 1)]


# ------------------------------------------------------------------ the yardsticks

@pytest.mark.parametrize("family,n", [(f, n) for f in mc.FAMILIES for n in PIN_SIZES] + [("ruler", 1025)])
def test_kruskal_is_boruvka(family, n):
    d = mc.FAMILIES[family](n)
    ke, kw = mc.kruskal(d)
    be, bw, rounds = mc.boruvka(d)
    assert np.array_equal(ke, be) and np.array_equal(kw, bw)
    assert (be[:, 0] < be[:, 1]).all() and rounds <= max(int(np.ceil(np.log2(n))), 1) + 1
    connected = not np.isnan(d).any()
    assert kw.size == (n - 1 if connected else n - 2)
    if connected:  # the sorted weights are the heights of scipy's single-linkage tree, ties or not
        assert np.array_equal(kw, scipy_linkage(condensed(d), "single")[:, 2])
    if family == "ruler" and n in mc.RULER_ROUNDS:
        assert rounds == mc.RULER_ROUNDS[n]


@pytest.mark.parametrize("n,core", [(n, c) for n in PIN_SIZES for c in ("given", "m1", "m5") if c == "given" or int(c[1:]) <= n])
def test_kruskal_is_boruvka_under_mutual_reachability(n, core):
    d = mc.euclid_points(n)
    c =mc.core_of(n) if core == "given" else mc.kth_smallest(d, int(core[1:]))
    W = mc.reachability(d, c)
    ke, kw = mc.kruskal(W)
    be, bw, _ = mc.boruvka(d, c)
    assert np.array_equal(ke, be) and np.array_equal(kw, bw)
    assert np.array_equal(kw, scipy_linkage(condensed(W), "single")[:, 2])
    if core == "m1":  # the smallest cell of a row is its own: the plain tree
        pe, pw = mc.kruskal(d)
        assert np.array_equal(ke, pe) and np.array_equal(kw, pw)


@pytest.mark.parametrize("n", [3, 65, 257])
def test_total_weight_is_scipys_on_tie_free_input(n):
    d = mc.euclid_points(n)
    e, w = mc.kruskal(d)
    t = scipy_mst(np.triu(d, 1)).tocoo()
    assert sorted(zip(np.minimum(t.row, t.col).tolist(), np.maximum(t.row, t.col).tolist())) == sorted(map(tuple, e.tolist()))
    assert np.array_equal(np.sort(t.data), w)


@pytest.mark.parametrize("n", PIN_SIZES)
def test_numpy_linkage_from_mst_is_scipys_z_on_tie_free_input(n):
    d = mc.euclid_points(n)
    e, w = mc.kruskal(d)
    assert np.array_equal(mc.linkage_from_mst(n, e, w), scipy_linkage(condensed(d), "single"))


def test_the_cases_cross_every_bound():
    for bound in (mc.WAVE, mc.MST_THREADS, mc.MST_WAVE_ROW):
        assert any(n <= bound for n in mc.SIZES) and any(n > bound for n in mc.SIZES), bound
    assert mc.MST_WAVE_ROW in mc.SIZES and mc.MST_WAVE_ROW + 1 in mc.SIZES
    src = (ROOT / "diverseseq_amd" / "csrc" / "mst.hip").read_text()
    assert re.search(rf"MST_WAVE_ROW = {mc.MST_WAVE_ROW};", src) and re.search(rf"MST_THREADS = {mc.MST_THREADS};", src)
    assert {2, 3, 64, 65, 257, 1025, 2049} <= set(mc.SIZES)
    assert {n for f, n in mc.matrix_cases() if f == "ruler"} >= set(mc.RULER_ROUNDS)


# ------------------------------------------------------------------ dvs_linkage_from_mst, through ctypes, no context

def c_linkage_from_mst(n, edges, weights):
    L = _lib.load()
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.uint32).ravel())
    w = np.ascontiguousarray(weights, dtype=np.float64)
    pairs, heights, sizes = distance.tree_outputs(n)
    rc = L.dvs_linkage_from_mst(None, n, _lib.ptr(e, C.c_uint32), _lib.ptr(w, C.c_double), _lib.ptr(pairs, C.c_uint32),
                                _lib.ptr(heights, C.c_double), _lib.ptr(sizes, C.c_uint32))
    return rc, distance.linkage_matrix(pairs, heights, sizes)


@pytest.mark.parametrize("n", PIN_SIZES)
def test_c_linkage_from_mst_is_scipys_z_on_tie_free_input(n):
    d = mc.euclid_points(n)
    e, w = mc.kruskal(d)
    rc, Z = c_linkage_from_mst(n, e, w)
    assert rc == _lib.OK and np.array_equal(Z, scipy_linkage(condensed(d), "single"))
    assert np.array_equal(cluster.mst_linkage(distance.MST(e, w, n, 0)), Z)


@pytest.mark.parametrize("n", PIN_SIZES)
def test_c_linkage_from_mst_on_ties_has_scipys_heights_and_cuts(n):
    d = mc.hamming10(n)
    e, w = mc.kruskal(d)
    rc, Z = c_linkage_from_mst(n, e, w)
    want = scipy_linkage(condensed(d), "single")
    assert rc == _lib.OK and np.array_equal(Z[:, 2], want[:, 2]) and np.array_equal(Z, mc.linkage_from_mst(n, e, w))
    assert Z[-1, 3] == n and (Z[:, 0] < Z[:, 1]).all()
    for h in np.unique(w).tolist():
        assert np.array_equal(cluster.cut_tree(Z, height=h), cluster.cut_tree(want, height=h)), h


def test_c_linkage_from_mst_refuses():
    n = 6
    e, w = mc.kruskal(mc.euclid_points(n))
    assert c_linkage_from_mst(n, e, w)[0] == _lib.OK
    assert c_linkage_from_mst(n, e[::-1], w[::-1])[0] == _lib.ERR_VALUE                     # not ascending
    bad_w = w.copy()
    bad_w[2] = np.nan
    assert c_linkage_from_mst(n, e, bad_w)[0] == _lib.ERR_VALUE
    cyc = e.copy()
    cyc[-1] = cyc[0]
    assert c_linkage_from_mst(n, cyc, w)[0] == _lib.ERR_VALUE                               # closes a cycle
    forest = np.full((n - 1, 2), 0xFFFFFFFF, dtype=np.uint32)
    forest[: n - 2] = e[: n - 2]
    assert c_linkage_from_mst(n, forest, w)[0] == _lib.ERR_VALUE                            # n - 2 edges: a forest
    assert c_linkage_from_mst(1, e, w)[0] == _lib.ERR_VALUE
    L = _lib.load()
    assert L.dvs_linkage_from_mst(None, n, None, None, None, None, None) == _lib.ERR_VALUE
    with pytest.raises(ValueError, match="forest"):
        cluster.mst_linkage(distance.MST(e[:-1], w[:-1], n, 3))
    with pytest.raises(ValueError, match="cycle"):
        cluster.mst_linkage(distance.MST(cyc, w, n, 3))
    with pytest.raises(ValueError):
        cluster.mst_linkage(distance.MST(e[:0], w[:0], 1, 0))


# ------------------------------------------------------------------ names

def test_names_of_the_feature():
    assert {"dvs_mst", "dvs_linkage_from_mst"} <= set(_lib.EXPORTS)
    lib = _lib.load()
    assert lib.dvs_mst.argtypes[1] == C.POINTER(_lib.Source) and lib.dvs_linkage_from_mst.argtypes is not None
    assert lib.dvs_abi_version() == 5
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dvs_hip.h").read_text(), flags=re.S)
    assert len(re.findall(r"\bint\s+dvs_mst\s*\(\s*dvs_ctx\s*\*\s*ctx\s*,\s*const\s+dvs_source\s*\*", header)) == 1
    assert len(re.findall(r"\bint\s+dvs_linkage_from_mst\s*\(", header)) == 1
    assert "dvs_mst" in apps.__all__ and callable(apps.dvs_mst)
    for name in ("MST", "run_mst", "matrix_mst", "mash_mst", "euclidean_mst", "jsd_mst", "mst"):
        assert hasattr(distance, name), name
    for name in ("minimum_spanning_tree", "mst_linkage", "mst_ctree", "mst_to_edges"):
        assert callable(getattr(cluster, name, None)), name
    assert distance.MST._fields == ("edges", "weights", "n", "n_rounds")
    assert "mst" in vars(distance.DeviceSide)
    assert callable(distance.DeviceSide.mst)
    tree = distance.MST(np.array([[0, 1]]), np.array([0.5]), 3, 2)
    assert not tree.connected and distance.MST(np.array([[0, 1], [1, 2]]), np.array([0.5, 1.0]), 3, 2).connected
    assert cluster.mst_to_edges(["a", "b", "c"], tree) == [("a", "b", 0.5)]
    with pytest.raises(ValueError):
        cluster.mst_to_edges(["a", "b"], tree)


# ------------------------------------------------------------------ argument checks, before any device work

def test_python_layer_refuses_before_any_device_work():
    d = mc.euclid_points(6)
    for bad in (0, -1, 65, 7, 2.0, True, "3"):
        with pytest.raises(ValueError, match="min_samples"):
            cluster.minimum_spanning_tree(d, min_samples=bad)
    asym = d.copy()
    asym[1, 4] += 0.5
    with pytest.raises(ValueError, match="symmetric"):
        cluster.minimum_spanning_tree(asym)
    one_nan = d.copy()
    one_nan[1, 4] = np.nan
    with pytest.raises(ValueError, match="symmetric"):
        cluster.minimum_spanning_tree(one_nan)
    for bad in (np.full(6, np.nan), np.full(6, np.inf), -np.ones(6), np.ones(5), np.ones((6, 1))):
        with pytest.raises(ValueError, match="core"):
            cluster.minimum_spanning_tree(d, core=bad)
    with pytest.raises(ValueError, match="position 3"):
        cluster.minimum_spanning_tree(d, core=[0, 0, 0, -1, 0, 0])
    with pytest.raises(ValueError, match="at most one"):
        cluster.minimum_spanning_tree(d, core=np.ones(6), min_samples=2)
    with pytest.raises(ValueError, match="square"):
        cluster.minimum_spanning_tree(np.ones((3, 4)))
    sparse = np.full((4, 4), np.nan)
    np.fill_diagonal(sparse, 0.0)
    with pytest.raises(ValueError, match="fewer than min_samples"):
        cluster.minimum_spanning_tree(sparse, min_samples=2)
    empty = cluster.minimum_spanning_tree(np.zeros((0, 0)))
    assert empty.n == 0 and empty.edges.shape == (0, 2) and empty.weights.size == 0 and not empty.connected
    seqs = [np.zeros(30, np.uint8)] * 3
    with pytest.raises(ValueError, match="Expected sketch size"):
        distance.mst(seqs, "mash", k=4)
    with pytest.raises(ValueError, match="Unexpected distance"):
        distance.mst(seqs, "hamming", k=4)
    with pytest.raises(ValueError, match="min_samples"):
        distance.mst(seqs, "jsd", k=4, min_samples=4)
    with pytest.raises(ValueError, match="core"):
        distance.mst(seqs, "jsd", k=4, core=[0.0, np.nan, 0.0])
    with pytest.raises(ValueError, match="at most one"):
        distance.mst(seqs, "jsd", k=4, core=[0.0] * 3, min_samples=1)
    with pytest.raises(ValueError, match="at least two"):
        cluster.mst_ctree({"a": seqs[0]}, k=4, sketch_size=None, distance_mode="jsd")
    got = distance.mst([], "jsd", k=4)
    assert got.n == 0 and got.n_rounds == 0 and got.edges.shape == (0, 2)


def test_app_constructor_checks():
    a = apps.dvs_mst("jsd", k=5, min_samples=3, tree=True)
    assert (a._k, a._sketch_size, a._distance_mode, a._min_samples, a._tree) == (5, None, "jsd", 3, True)
    assert apps.dvs_mst()._sketch_size == 3000 and not apps.dvs_mst()._tree
    with pytest.raises(ValueError, match="Unexpected distance"):
        apps.dvs_mst("hamming")
    with pytest.raises(ValueError, match="Expected sketch size"):
        apps.dvs_mst("mash", sketch_size=None)
    with pytest.raises(ValueError, match="Canonical kmers only supported"):
        apps.dvs_mst("mash", moltype="protein", mash_canonical_kmers=True)
    with pytest.raises(ValueError):
        apps.dvs_mst("mash", canonical=True)
    for bad in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match="min_samples"):
            apps.dvs_mst("jsd", min_samples=bad)
    with pytest.raises(ValueError, match="tree"):
        apps.dvs_mst("jsd", tree="newick")
