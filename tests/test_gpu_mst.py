"""The minimum spanning tree on the GPU (csrc/mst.hip, dvs_mst) against the yardsticks of tests/mst_cases.py, which
tests/test_mst_host.py pins on the CPU.  The tree is unique under the order (weight, lower position, higher position),
so every comparison is "equal as arrays": no tolerance anywhere in this file."""
import ctypes as C

import numpy as np
import pytest

import mst_cases as mc
from conftest import clades
from diverseseq_amd import _lib, apps, cluster, distance, engine
from test_blocks_host import POISON
from test_gpu_cross import _seqs

pytestmark = pytest.mark.gpu

CASES = mc.matrix_cases()
CASE_IDS = [f"{f}{n}" for f, n in CASES]


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context()


def assert_tree(got, want, n, what=""):
    """a `distance.MST` against (edges, weights, rounds) of the yardstick: equal as arrays, the weights bit for bit"""
    edges, weights, rounds = want
    assert got.edges.dtype == np.int64 and got.weights.dtype == np.float64 and got.edges.shape == (got.weights.size, 2), what
    assert np.array_equal(got.edges, edges), (what, "edges")
    assert np.array_equal(got.weights.view(np.uint64), np.ascontiguousarray(weights).view(np.uint64)), (what, "weights")
    assert got.n == n and got.n_rounds == rounds, (what, got.n_rounds, rounds)
    assert got.connected == (weights.size == n - 1), what


def assert_cuts(got, D, ctx, what=""):
    """cut_tree over the tree of a connected `MST` against the threshold clusters of the same distances, at a few merge
    heights, one ulp below each, and between two"""
    Z = cluster.mst_linkage(got)
    assert np.array_equal(Z[:, 2], got.weights) and Z[-1, 3] == got.n
    for h in mc.cut_heights(got.weights):
        want = cluster.threshold_clusters(D, h, ctx=ctx).labels
        assert np.array_equal(cluster.cut_tree(Z, height=h), want), (what, h)


# ------------------------------------------------------------------ 1. a caller's matrix, on the host and on the device

@pytest.mark.parametrize("family,n", CASES, ids=CASE_IDS)
def test_callers_matrix_host_and_device(ctx, family, n):
    import torch

    D = mc.FAMILIES[family](n)
    want = mc.expected(family, n)
    got = cluster.minimum_spanning_tree(D, ctx=ctx)
    assert_tree(got, want, n, "host")
    t = torch.from_numpy(D.copy()).to("cuda:0")
    before = t.clone()
    assert_tree(cluster.minimum_spanning_tree(t, ctx=ctx), want, n, "device")
    assert torch.equal(t.view(torch.int64), before.view(torch.int64)), "the device matrix was written"
    if family == "ruler" and n in mc.RULER_ROUNDS:
        assert got.n_rounds == mc.RULER_ROUNDS[n]
    if got.connected:
        assert_cuts(got, D, ctx, family)
    else:
        assert got.weights.size == n - 2  # (both forests are two trees)
        with pytest.raises(ValueError, match="forest"):
            cluster.mst_linkage(got)


# ------------------------------------------------------------------ 2. strip heights

@pytest.mark.parametrize("family,n", CASES, ids=CASE_IDS)
def test_strip_height_does_not_change_a_bit(ctx, monkeypatch, family, n):
    D = mc.FAMILIES[family](n)
    want = mc.expected(family, n)
    for strip in mc.STRIPS:
        monkeypatch.setenv("DVS_CROSS_STRIP_ROWS", str(strip))
        assert_tree(cluster.minimum_spanning_tree(D, check_symmetric=False, ctx=ctx), want, n, strip)


# ------------------------------------------------------------------ 3. poisoned blocks, other operations in between

@pytest.mark.parametrize("family,n", CASES, ids=CASE_IDS)
def test_poisoned_blocks_and_an_interleaved_workload(ctx, monkeypatch, family, n):
    """every block the call takes (the strip; the labels, core vector and candidates) full of 0xFF, with calls of other
    operations over blocks of the same sizes between two runs on one context"""
    D = mc.FAMILIES[family](n)
    want, want_core = mc.expected(family, n), mc.expected(family, n, "given")
    small = mc.euclid_points(65)
    monkeypatch.setenv("DVS_TEST_KNOBS", POISON)
    assert_tree(cluster.minimum_spanning_tree(D, check_symmetric=False, ctx=ctx), want, n, "poisoned")
    cluster.threshold_clusters(D, 1.0, ctx=ctx)
    cluster.linkage(small, "single", ctx=ctx)
    assert_tree(cluster.minimum_spanning_tree(D, core=mc.core_of(n), check_symmetric=False, ctx=ctx), want_core, n, "core")
    cluster.within(small, 0.25, ctx=ctx)
    cluster.cluster_scores(small, np.arange(65) % 3, ctx=ctx)
    assert_tree(cluster.minimum_spanning_tree(D, check_symmetric=False, ctx=ctx), want, n, "poisoned, again")


# ------------------------------------------------------------------ 4. mutual reachability

@pytest.mark.parametrize("family", ["euclid", "hamming"])
@pytest.mark.parametrize("n", [5, 65, 257, 1024, 1025])
def test_mutual_reachability(ctx, family, n):
    import torch

    D = mc.FAMILIES[family](n)
    plain = mc.expected(family, n)
    core = mc.core_of(n)
    for name, kwargs, c in (("given", {"core": core}, core), ("m1", {"min_samples": 1}, mc.kth_smallest(D, 1)),
                            ("m5", {"min_samples": 5}, mc.kth_smallest(D, 5))):
        want = mc.expected(family, n, name)
        ke, kw = mc.kruskal(mc.reachability(D, c))
        assert np.array_equal(want[0], ke) and np.array_equal(want[1], kw)
        got = cluster.minimum_spanning_tree(D, ctx=ctx, **kwargs)
        assert_tree(got, want, n, name)
        t = torch.from_numpy(D.copy()).to("cuda:0")
        assert_tree(cluster.minimum_spanning_tree(t, ctx=ctx, **kwargs), want, n, name + ", device")
        assert torch.equal(t.cpu(), torch.from_numpy(D.copy()))
        if name == "m1":
            assert np.array_equal(got.edges, plain[0]) and np.array_equal(got.weights, plain[1])
    assert_cuts(got, mc.reachability(D, mc.kth_smallest(D, 5)), ctx, "m5")


def test_an_asymmetric_matrix_still_gives_a_spanning_tree(ctx):
    D = np.random.default_rng(3).random((129, 129))
    with pytest.raises(ValueError, match="symmetric"):
        cluster.minimum_spanning_tree(D, ctx=ctx)
    got = cluster.minimum_spanning_tree(D, check_symmetric=False, ctx=ctx)
    assert got.connected and (got.edges[:, 0] < got.edges[:, 1]).all() and (np.diff(got.weights) >= 0).all()
    assert cluster.mst_linkage(got)[-1, 3] == 129  # (no cycle: dvs_linkage_from_mst would refuse one)
    cell = np.minimum(D[got.edges[:, 0], got.edges[:, 1]], D[got.edges[:, 1], got.edges[:, 0]])
    assert (got.weights >= cell).all()


# ------------------------------------------------------------------ 5. the three modes

def _mode_side(ctx, mode, seqs, canonical=False):
    args = (8, 50, 4, False) if mode == "mash" else (3, 4)
    return distance.device_side(seqs, mode, *args, ctx=ctx, canonical=canonical)


@pytest.mark.parametrize("mode", ["jsd", "euclidean", "mash"])
def test_modes_against_their_own_distances(ctx, monkeypatch, mode):
    rng = np.random.default_rng(17)
    seqs = _seqs(rng, 65)
    seqs[40] = seqs[12].copy()  # a distance of zero
    rows = rng.permutation(65)[:33]
    with _mode_side(ctx, mode, seqs) as side:
        D = side.distances()
        e, w, rounds = mc.boruvka(D)
        ke, kw = mc.kruskal(D)
        assert np.array_equal(e, ke) and np.array_equal(w, kw)
        got = side.mst()
        assert_tree(got, (e, w, rounds), 65, mode)
        heights = side.linkage("single")[:, 2]
        assert np.array_equal(got.weights.view(np.uint64), heights.view(np.uint64)), "the single-linkage heights, bit for bit"
        for h in mc.cut_heights(got.weights):
            assert np.array_equal(cluster.cut_tree(cluster.mst_linkage(got), height=h), side.threshold_clusters(h).labels), h
        assert_tree(side.mst(rows), mc.boruvka(D[np.ix_(rows, rows)]), 33, "a row list")
        for m in (1, 5):
            assert_tree(side.mst(min_samples=m), mc.boruvka(D, mc.kth_smallest(D, m)), 65, f"min_samples {m}")
        assert_tree(side.mst(core=mc.core_of(65) * np.nanmax(D)), mc.boruvka(D, mc.core_of(65) * np.nanmax(D)), 65, "core")
        monkeypatch.setenv("DVS_CROSS_STRIP_ROWS", "7")
        assert_tree(side.mst(), (e, w, rounds), 65, "strips of 7")
        monkeypatch.setenv("DVS_TEST_KNOBS", POISON)
        assert_tree(side.mst(rows, min_samples=5), mc.boruvka(D[np.ix_(rows, rows)], mc.kth_smallest(D[np.ix_(rows, rows)], 5)),
                    33, "poisoned")
    public = {"jsd": lambda: distance.jsd_mst(seqs, 3, ctx=ctx), "euclidean": lambda: distance.euclidean_mst(seqs, 3, ctx=ctx),
              "mash": lambda: distance.mash_mst(seqs, 8, 50, ctx=ctx)}[mode]()
    assert_tree(public, (e, w, rounds), 65, "the mode's function")
    general = distance.mst(seqs, mode, k=8 if mode == "mash" else 3, sketch_size=50 if mode == "mash" else None, ctx=ctx)
    assert_tree(general, (e, w, rounds), 65, "distance.mst")


@pytest.mark.parametrize("mode", ["jsd", "euclidean"])
def test_canonical_rows_and_a_row_without_a_kmer(ctx, mode):
    seqs = _seqs(np.random.default_rng(23), 33, empty=(7,))
    with _mode_side(ctx, mode, seqs, canonical=True) as side:
        D = side.distances()
        assert np.isnan(D[7, :7]).all() and np.isnan(D[7, 8:]).all()
        got = side.mst()
        assert_tree(got, mc.boruvka(D), 33, "canonical")
        assert not got.connected and got.weights.size == 31 and 7 not in got.edges  # an isolated vertex
        with pytest.raises(ValueError, match="forest"):
            cluster.mst_linkage(got)
        with pytest.raises(ValueError, match="fewer than min_samples"):
            side.mst(min_samples=2)
        assert_tree(distance.matrix_mst(side.handle, mode), mc.boruvka(D), 33, "matrix_mst")
    plain = {"jsd": distance.jsd_mst, "euclidean": distance.euclidean_mst}[mode](seqs, 3, ctx=ctx)
    folded = {"jsd": distance.jsd_mst, "euclidean": distance.euclidean_mst}[mode](seqs, 3, ctx=ctx, canonical=True)
    assert np.array_equal(folded.edges, got.edges) and not np.array_equal(folded.weights, plain.weights)


def test_an_empty_sketch_divides_by_zero(ctx):
    seqs = _seqs(np.random.default_rng(29), 20)
    seqs[4] = seqs[4][:3].copy()  # shorter than k: an empty sketch
    with _mode_side(ctx, "mash", seqs) as side:
        with pytest.raises(ZeroDivisionError):
            side.cluster_scores([0] * 20)
        with pytest.raises(ZeroDivisionError):
            side.mst()
        rows = [r for r in range(20) if r != 4]
        assert_tree(side.mst(rows), mc.boruvka(side.distances()[np.ix_(rows, rows)]), 19, "usable afterwards")


# ------------------------------------------------------------------ 6. the C entry

def test_c_entry_refuses_bad_arguments_and_writes_nothing(ctx):
    L, S = ctx._L, distance.make_source
    u32, f64 = (lambda a: _lib.ptr(a, C.c_uint32)), (lambda a: _lib.ptr(a, C.c_double))
    d = mc.euclid_points(40)
    big = 65535 * 8 + 1  # one row more than the square entries take
    edges, weights = np.full(78, 7, np.uint32), np.full(39, 7.0)
    count, rounds = C.c_uint32(99), C.c_uint32(99)

    def given(n, on_device=0, handle=d.ctypes.data, rows=None):
        return S(_lib.SRC_GIVEN, handle, n, rows, on_device=on_device)

    def call(src, core=None, e=edges, w=weights, c=count, r=rounds):
        return L.dvs_mst(ctx._h, src, None if core is None else f64(core), None if e is None else u32(e),
                         None if w is None else f64(w), None if c is None else C.byref(c), None if r is None else C.byref(r))

    def untouched():
        return (edges == 7).all() and (weights == 7.0).all() and count.value == 99 and rounds.value == 99

    assert call(given(40), e=None) == _lib.ERR_VALUE and call(given(40), w=None) == _lib.ERR_VALUE
    assert call(given(40), c=None) == _lib.ERR_VALUE and b"dvs_mst" in L.dvs_last_error(ctx._h)
    for bad in (np.nan, np.inf, -1.0):
        core = np.zeros(40)
        core[13] = bad
        assert call(given(40), core) == _lib.ERR_VALUE
        msg = L.dvs_last_error(ctx._h)
        assert b"dvs_mst" in msg and b"position 13" in msg, msg
    assert call(given(40, handle=None)) == _lib.ERR_VALUE
    assert call(given(40, 1)) == _lib.ERR_VALUE                               # a host array is not device memory
    assert call(given(40, rows=np.arange(40, dtype=np.uint32))) == _lib.ERR_VALUE  # a caller's matrix takes no row list
    assert call(given(big)) == _lib.ERR_UNSUPPORTED
    assert L.dvs_mst(None, given(40), None, u32(edges), f64(weights), C.byref(count), C.byref(rounds)) == _lib.ERR_VALUE
    assert call(given(0), e=None, w=None, c=None, r=None) == _lib.OK and call(given(0)) == _lib.OK  # n == 0: nothing written
    assert untouched()
    m = ctx.build_matrix(_seqs(np.random.default_rng(1), 10), 3, 4)
    try:
        for kind in (_lib.SRC_JSD, _lib.SRC_EUCLIDEAN):
            assert call(S(kind, m._h, 11)) == _lib.ERR_VALUE                   # more rows than the handle holds
            assert call(S(kind, m._h, 2, np.array([0, 10], np.uint32))) == _lib.ERR_VALUE
            assert call(S(kind, None, 10)) == _lib.ERR_VALUE
        assert untouched()
    finally:
        m.close()
    assert call(given(1)) == _lib.OK and (count.value, rounds.value) == (0, 0)  # n == 1: no edge, no round
    assert (edges == 7).all() and (weights == 7.0).all()
    assert call(given(40), r=None) == _lib.OK and count.value == 39            # n_rounds may be NULL
    want = mc.expected("euclid", 40)
    assert np.array_equal(edges.reshape(39, 2), want[0]) and np.array_equal(weights, want[1])
    with pytest.raises(NotImplementedError):
        distance.run_mst(ctx, given(big))


# ------------------------------------------------------------------ 7. trees and the app

def test_mst_ctree_is_the_single_linkage_ctree_of_brca1(ctx, brca1):
    names = list(brca1)
    arrays = [brca1[n] for n in names]
    newick = cluster.mst_ctree(brca1, k=8, sketch_size=400)
    assert newick.endswith(";") and newick.count("(") == len(names) - 1
    leaves = {leaf for clade in clades(newick) for leaf in clade}
    assert leaves == set(names)
    Z = distance.mash_linkage(arrays, 8, 400, method="single", ctx=ctx)
    tree = distance.mst(arrays, "mash", k=8, sketch_size=400, ctx=ctx)
    assert tree.connected and np.array_equal(tree.weights.view(np.uint64), np.ascontiguousarray(Z[:, 2]).view(np.uint64))
    assert newick == cluster.linkage_to_newick(names, cluster.mst_linkage(tree))
    single = cluster.ctree(brca1, k=8, sketch_size=400, linkage="single")
    assert {leaf for clade in clades(single) for leaf in clade} == leaves
    if np.unique(Z[:, 2]).size == Z.shape[0]:  # no two merges of one height: the same tree
        assert clades(newick) == clades(single)


def test_the_app_round_trips(ctx):
    seqs = _seqs(np.random.default_rng(31), 20)
    named = {f"s{i}": s for i, s in enumerate(seqs)}
    tree = distance.mst(seqs, "jsd", k=4, ctx=ctx)
    assert apps.dvs_mst("jsd", k=4)(named) == cluster.mst_to_edges(list(named), tree)
    assert apps.dvs_mst("jsd", k=4, tree=True)(named) == cluster.mst_ctree(named, k=4, sketch_size=None, distance_mode="jsd")
    robust = distance.mst(seqs, "mash", k=8, sketch_size=50, min_samples=3, ctx=ctx)
    got = apps.dvs_mst("mash", k=8, sketch_size=50, min_samples=3)(named)
    assert got == cluster.mst_to_edges(list(named), robust) and len(got) == 19
    assert all(a in named and b in named and isinstance(w, float) for a, b, w in got)
