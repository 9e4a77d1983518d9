"""Neighbour joining on the GPU (csrc/nj.hip) against the yardsticks of test_nj_host.py: the generating tree of dyadic
additive distances recovered exactly, the heavy-tie matrices bit for bit against the restatement, general input as the
unrooted tree of the long-double run, and the entries around the kernels (device tensors, non-finite input, the fused
distance modes, the C boundary)."""
import ctypes as C

import numpy as np
import pytest

from diverseseq_amd import _lib, apps, cluster, distance, engine
from test_gpu_linkage import family_seqs
from test_nj_host import (EPS, KINDS_GENERAL, SIZES_GENERAL, dyadic_tree, general_yardstick, length_tolerance,
                          newick_splits, restated, same_tree, split_lengths, tie_case, truth)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


# 63 .. 65: the wave; 257: more rows than a scan workgroup's waves and a join's first pass; 1025: more list positions
# than the join workgroup has threads (the second trip of its list compaction; its update loop, which covers 4096
# positions a trip, still takes one); 2049: 513 scan workgroups and a third trip of the compaction; every n > 8 repacks (first
# at r < n / 2), 2049 ten times.  The regimes beyond -- a second trip of the update loop and of the candidate reduction
# (r > 4096), a second pass of the scan over its capped grid (r > 8192) -- are in test_gpu_second_trips.py
EXACT = [(n, shape) for n in (3, 4, 5, 63, 64, 65, 257) for shape in ("random", "caterpillar", "balanced")]
EXACT += [(1025, "random"), (2049, "random")]


@pytest.mark.parametrize("n,shape", EXACT)
def test_dyadic_additive_trees_are_recovered_exactly(ctx, n, shape):
    tree, A = dyadic_tree(n, shape)
    got = cluster.neighbor_joining(A, ctx=ctx)
    assert got.children.shape == (n - 2, 3) and got.children.dtype == np.int64 and got.lengths.dtype == np.float64
    assert split_lengths(got, n) == split_lengths(tree, n)  # == on the floats
    assert np.array_equal(cluster.patristic(got), A)


@pytest.mark.parametrize("kind", ["small-integer", "constant", "zero"])
@pytest.mark.parametrize("n", [3, 4, 5, 7, 64, 300])
def test_ties_bit_for_bit(ctx, n, kind):
    d = tie_case(kind, n)
    want = restated(d)
    got = cluster.neighbor_joining(d, ctx=ctx)
    assert np.array_equal(got.children, want.children)
    assert np.array_equal(got.lengths, want.lengths)


@pytest.mark.parametrize("kind", KINDS_GENERAL)
@pytest.mark.parametrize("n", SIZES_GENERAL)
def test_general_input_is_truths_tree(ctx, n, kind):
    d, want, gap, err = general_yardstick(kind, n)
    got = split_lengths(cluster.neighbor_joining(d, ctx=ctx), n)
    assert set(got) == set(want)
    unit = n * EPS * float(np.abs(d).max())
    worst = same_tree(got, want, length_tolerance(n, d, err))
    print(f"n={n} {kind}: device worst length error {worst / unit:.3g} n eps max|D|, restated's {err / unit:.3g}, "
          f"ratio {worst / err if err else float('nan'):.3g}")


def test_only_the_upper_triangle_counts_and_the_input_is_kept(ctx):
    rng = np.random.default_rng(5)
    n = 131
    d = rng.random((n, n))
    before = d.copy()
    got = cluster.neighbor_joining(d, ctx=ctx)
    assert np.array_equal(d, before)
    up = np.triu(d, 1)
    sym = cluster.neighbor_joining(up + up.T, ctx=ctx)
    assert np.array_equal(got.children, sym.children) and np.array_equal(got.lengths, sym.lengths)
    tc, tl, _ = truth(d)
    assert set(split_lengths(got, n)) == set(split_lengths((tc, tl), n))
    lists = cluster.neighbor_joining([[0, 1, 4, 3], [9, 0, 2, 5], [9, 9, 0, 1], [9, 9, 9, 0]], ctx=ctx)
    want = restated(np.array([[0, 1, 4, 3], [1, 0, 2, 5], [4, 2, 0, 1], [3, 5, 1, 0]], dtype=np.float64))
    assert np.array_equal(lists.children, want.children) and np.array_equal(lists.lengths, want.lengths)


def test_device_tensor_is_used_in_place(ctx):
    import torch

    n = 513
    d = np.random.default_rng(7).random((n, n))
    host = cluster.neighbor_joining(d, ctx=ctx)
    t = torch.from_numpy(d).to("cuda:0")
    got = cluster.neighbor_joining(t, ctx=ctx)
    assert np.array_equal(got.children, host.children) and np.array_equal(got.lengths, host.lengths)
    assert not np.array_equal(t.cpu().numpy(), d)  # the working buffer
    with pytest.raises(ValueError):
        cluster.neighbor_joining(torch.zeros((4, 5), dtype=torch.float64, device="cuda:0"), ctx=ctx)
    with pytest.raises(ValueError):
        cluster.neighbor_joining(torch.zeros((5, 5), dtype=torch.float32, device="cuda:0"), ctx=ctx)
    with pytest.raises(ValueError):
        cluster.neighbor_joining(torch.zeros((6, 6), dtype=torch.float64, device="cuda:0")[:5, :5], ctx=ctx)
    with pytest.raises(ValueError):
        cluster.neighbor_joining(torch.zeros((2, 2), dtype=torch.float64, device="cuda:0"), ctx=ctx)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            cluster.neighbor_joining(torch.zeros((5, 5), dtype=torch.float64, device="cuda:1"), ctx=ctx)


@pytest.mark.parametrize("where", [(0, 0), (2, 7), (7, 2), (99, 98)])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_anywhere_is_a_value_error(ctx, where, bad):
    d = np.random.default_rng(8).random((100, 100))
    d[where] = bad
    with pytest.raises(ValueError, match="NaN or infinity"):
        cluster.neighbor_joining(d, ctx=ctx)
    tree, A = dyadic_tree(50, "random", seed=9)  # the context is usable afterwards
    assert split_lengths(cluster.neighbor_joining(A, ctx=ctx), 50) == split_lengths(tree, 50)


def _fused_check(seqs: dict, kw: dict, dist: np.ndarray, merge_zero: bool):
    names = list(seqs)
    n = len(names)
    newick, tree = cluster.nj_tree(seqs, **kw)
    tc, tl, _ = truth(dist)
    want = split_lengths((tc, tl), n)
    ref = split_lengths(restated(dist), n)
    err = max(abs(float(ref[k] - want[k])) for k in want if k in ref)
    tol = length_tolerance(n, dist, err)
    got = split_lengths(tree, n)
    if not merge_zero:
        assert set(got) == set(want)
    same_tree(got, want, tol, merge_zero=merge_zero)
    # the string says what the tree says
    assert newick_splits(newick, names) == got
    assert np.array_equal(np.sort(tree.children[tree.children >= 0]), np.arange(2 * n - 3))


def test_fused_entries_brca1(brca1):
    arrays = [brca1[n] for n in brca1]
    _fused_check(brca1, dict(k=16, sketch_size=400), distance.mash_distances(arrays, 16, 400), False)
    _fused_check(brca1, dict(k=5, sketch_size=None, distance_mode="euclidean"), distance.euclidean_distances(arrays, 5), False)
    _fused_check(brca1, dict(k=5, sketch_size=None, distance_mode="jsd"), distance.jsd_distances(arrays, 5), False)


def test_fused_entries_families_with_duplicates():
    """exact duplicates: zero distances and zero-length edges, compared after merging them (test_nj_host.py)"""
    seqs = family_seqs(12, 25, 4000, seed=13)
    arrays = [seqs[n] for n in seqs]
    assert len(seqs) == 300
    _fused_check(seqs, dict(), distance.mash_distances(arrays, 12, 3000), True)
    _fused_check(seqs, dict(k=5, sketch_size=None, distance_mode="jsd"), distance.jsd_distances(arrays, 5), True)


def test_fused_entries_app_and_errors(brca1):
    names = list(brca1)[:12]
    text_kw = dict(k=12, sketch_size=3000)
    seqs = {n: brca1[n] for n in names}
    assert apps.dvs_njtree(**text_kw)(seqs) == cluster.nj_tree(seqs, **text_kw)[0]
    empty = {"a": np.zeros(3, np.uint8), "b": np.ones(2, np.uint8), "c": np.arange(40, dtype=np.uint8) % 4}
    with pytest.raises(ZeroDivisionError):  # two empty sketches
        cluster.nj_tree(empty, k=8, sketch_size=10)
    no_kmers = {"a": np.full(50, 4, np.uint8), "b": np.arange(50, dtype=np.uint8) % 4, "c": np.ones(50, np.uint8)}
    for mode in ("euclidean", "jsd"):
        with pytest.raises(ValueError, match="NaN or infinity"):  # NaN distances of a row without valid k-mers
            cluster.nj_tree(no_kmers, k=3, sketch_size=None, distance_mode=mode)
    with pytest.raises(ValueError, match="three sequences"):
        cluster.nj_tree({k: empty[k] for k in "ab"}, k=8, sketch_size=10)


def test_c_boundary(ctx):
    L = ctx._L
    u32, f64 = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    _, A = dyadic_tree(9, "random")
    joins = np.zeros(21, dtype=np.uint32)
    lens = np.full(21, -1.0)
    d = np.ascontiguousarray(A)

    def given(n, on_device=0, handle=d.ctypes.data):
        return distance.make_source(_lib.SRC_GIVEN, handle, n, on_device=on_device)

    assert L.dvs_nj(ctx._h, given(9), joins.ctypes.data_as(u32), lens.ctypes.data_as(f64)) == _lib.OK
    j, l = joins.reshape(7, 3), lens.reshape(7, 3)
    assert (j[:6, 2] == 0xFFFFFFFF).all() and (l[:6, 2] == 0.0).all() and j[6, 2] != 0xFFFFFFFF
    assert sorted(j[j != 0xFFFFFFFF].tolist()) == list(range(15))
    assert L.dvs_nj(ctx._h, given(2), joins.ctypes.data_as(u32), lens.ctypes.data_as(f64)) == _lib.ERR_VALUE
    assert b"three sequences" in L.dvs_last_error(ctx._h)
    assert L.dvs_nj(ctx._h, given(9, handle=None), joins.ctypes.data_as(u32), lens.ctypes.data_as(f64)) == _lib.ERR_VALUE
    assert L.dvs_nj(ctx._h, given(9), None, lens.ctypes.data_as(f64)) == _lib.ERR_VALUE
    assert L.dvs_nj(ctx._h, given(9), joins.ctypes.data_as(u32), None) == _lib.ERR_VALUE
    null_sketches = distance.make_source(_lib.SRC_MASH, None, 9, k=8, sketch_size=10)
    assert L.dvs_nj(ctx._h, null_sketches, joins.ctypes.data_as(u32), lens.ctypes.data_as(f64)) == _lib.ERR_VALUE
    for kind in (_lib.SRC_EUCLIDEAN, _lib.SRC_JSD):
        null_matrix = distance.make_source(kind, None, 9)
        assert L.dvs_nj(ctx._h, null_matrix, joins.ctypes.data_as(u32), lens.ctypes.data_as(f64)) == _lib.ERR_VALUE
    # a host pointer said to be device memory
    assert L.dvs_nj(ctx._h, given(9, 1), joins.ctypes.data_as(u32), lens.ctypes.data_as(f64)) == _lib.ERR_VALUE
