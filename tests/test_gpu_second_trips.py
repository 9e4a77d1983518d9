"""The distance-side kernels past the sizes where their loops repeat (the cases and thresholds of
tests/test_second_trips_host.py): neighbour joining with more active rows than a join's update loop covers in one trip
(4096) and than a scan's capped grid has waves (8192), cophenet_kernel with more than one chunk of 1024 positions on a
side of the leaf order, cross_topk_kernel over rows that are not staged in LDS (more than 2048 cells), the cross
instantiation of mash_pairs_kernel with a shared row that is not staged (more than 8192 hashes), and a walk that the
driver's own arithmetic cuts into two strips.  Every comparison is against something other than the code under test,
with the yardsticks, assertions and tolerances of the older files: test_nj_host's generating trees and restatement,
test_cophenet_host's long-double sums and scipy, numpy's stable argsort, the oracle's sketches and mash distances, the
square entries."""
import time

import numpy as np
import pytest

import oracle
from diverseseq_amd import cluster, distance, engine
from test_cophenet_host import KINDS, case_matrix
from test_gpu_cophenet import assert_same_scores, assert_scores, same_bits
from test_gpu_cross import MASH_RTOL, assert_nearest
from test_nj_host import split_lengths
from test_second_trips_host import (COPH_CASES, COPH_CHUNK, COPH_DEFAULT_CUT, COPH_STRIP_SEQS, LONG_EMPTY_REF, LONG_SKETCH,
                                    MASH_NEAREST, NEAREST_K, NEAREST_KK, NEAREST_REFS, NJ_DEVICE_TENSOR, NJ_EXACT,
                                    NJ_JOIN_TRIP, NJ_SCAN_PASS, PAIR_ROW_LDS, PREFIX_CASES, PREFIX_KINDS, SPARSE_LIVE,
                                    TIE_QUERY, TOPK_LDS, chunks_per_side, copies_of_reference_2, default_strip_rows,
                                    exact_case, long_sketch_case, long_sketch_oracle, mash_nearest_case, nearest_case,
                                    prefix_yardstick, random_seqs, sparse_case, tail_joins, tail_start)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context()


# ------------------------------------------------------------------ 1. neighbour joining, r > 4096 and r > 8192
@pytest.mark.parametrize("n,shape", NJ_EXACT)
def test_nj_recovers_large_dyadic_trees_exactly(ctx, n, shape):
    """the whole tree: every join's update loop takes two trips down to r = 4096 (three above 8192), its candidate
    reduction two, and above r = 8192 the scan deals its rows out in two passes.  (Where the device-tensor case is the
    first test of a process to put a tensor on the device, most of its time is torch's initialisation.)"""
    assert n > NJ_JOIN_TRIP and (n > NJ_SCAN_PASS or (n, shape) == NJ_EXACT[0])
    want, A = exact_case(n, shape)
    t0 = time.perf_counter()
    got = cluster.neighbor_joining(A, ctx=ctx)
    print(f"n={n} {shape}: neighbor_joining of a host matrix took {time.perf_counter() - t0:.2f} s (upload included)")
    assert got.children.shape == (n - 2, 3) and got.children.dtype == np.int64 and got.lengths.dtype == np.float64
    assert split_lengths(got, n) == want  # == on the floats
    assert np.array_equal(cluster.patristic(got), A)
    if (n, shape) == NJ_DEVICE_TENSOR:
        import torch

        t = torch.from_numpy(np.array(A)).to("cuda:0")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev = cluster.neighbor_joining(t, ctx=ctx)
        print(f"n={n} {shape}: neighbor_joining of a device tensor took {time.perf_counter() - t0:.2f} s")
        assert np.array_equal(dev.children, got.children) and np.array_equal(dev.lengths, got.lengths)


@pytest.mark.parametrize("kind", PREFIX_KINDS)
@pytest.mark.parametrize("n,steps", PREFIX_CASES)
def test_nj_join_order_bit_for_bit_across_the_edge(ctx, n, steps, kind):
    """the first `steps` records against the restatement, where every decision is exact whatever the order of summation
    (test_second_trips_host.prefix_case): the all-tie kinds hold the lowest-(i, j) rule across both passes of a scan and
    across more than 1024 candidates, the third one the minimum itself, the far-tail kinds a minimum and a tie that lie
    in the rows of the second pass (the list positions of the second trip).  Of the later records only the form is known"""
    edge = NJ_JOIN_TRIP if n < NJ_SCAN_PASS else NJ_SCAN_PASS
    assert n > edge >= n - steps + 1  # the active rows of the compared steps: n .. n - steps + 1
    d, children, lengths = prefix_yardstick(kind, n, steps)
    if kind.startswith("far-tail"):  # the winners are rows beyond the edge until one node is left there
        assert tail_start(n) == edge and tail_joins(n, children) == n - edge - 1 >= 7
    got = cluster.neighbor_joining(d, ctx=ctx)
    assert np.array_equal(got.children[:steps], children)
    assert np.array_equal(got.lengths[:steps], lengths)
    assert got.children.shape == got.lengths.shape == (n - 2, 3)
    t = np.arange(n - 2)
    assert (got.children[:, :2] >= 0).all() and (got.children[:, :2] < (n + t)[:, None]).all()
    assert (got.children[:-1, 2] == -1).all() and 0 <= got.children[-1, 2] < 2 * n - 3
    assert np.array_equal(np.sort(got.children[got.children >= 0]), np.arange(2 * n - 3))  # every node joined once


# ------------------------------------------------------------------ 2. cophenetic scores, more than one chunk per side
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,method", COPH_CASES)
def test_cophenet_with_more_than_one_chunk_on_a_side(ctx, n, method, kind):
    """a caller's host matrix, the tree from the device: the cophenetic matrix against scipy's bit for bit, the row sums
    and r against the long-double yardstick and scipy (assert_scores).  The caterpillar's order is the one where the
    maximum carried from chunk to chunk is a long running one"""
    most, both = chunks_per_side(n)
    assert n - 1 > COPH_CHUNK and most >= 2 and (n < 2100 or both >= 2) and (n < 3000 or n - 1 > 2 * COPH_CHUNK)
    assert default_strip_rows(n, n) == n  # one strip: the chunks are all that is new here
    D = case_matrix(n, kind)
    Z = cluster.linkage(D, method, ctx=ctx)
    got = cluster.cophenet(Z, D, matrix=True, ctx=ctx)
    assert_scores(got, D, Z, f"n={n} {kind} {method}")
    assert (np.diag(got.cophenetic) == 0).all()


@pytest.mark.parametrize("mode", ["jsd", "euclidean"])
def test_cophenet_fused_over_count_rows_whole_and_in_strips(ctx, monkeypatch, mode):
    """the strips' sums against cluster.cophenet on the matrix the cross entry returns for the same rows, with the
    default strip (one) and in strips of 7 rows"""
    n = COPH_STRIP_SEQS
    assert chunks_per_side(n)[0] >= 2 and default_strip_rows(n, n) == n
    m = ctx.build_matrix(random_seqs(np.random.default_rng(12), n), 3, 4)
    try:
        d = distance.matrix_cross_distances(m, m, mode)
        Z = cluster.linkage(d, "average", ctx=ctx)
        want = cluster.cophenet(Z, d, matrix=True, ctx=ctx)
        whole = distance.matrix_cophenet(m, Z, mode, matrix=True)
        assert_same_scores(whole, want, f"{mode}, the default strip")
        monkeypatch.setenv("DVS_CROSS_STRIP_ROWS", "7")
        assert_same_scores(distance.matrix_cophenet(m, Z, mode, matrix=True), want, f"{mode}, strips of 7")
        assert_scores(whole, d, Z, f"{mode} fused n={n}")
    finally:
        m.close()


def test_cophenet_over_a_walk_the_default_strip_cuts_in_two(ctx):
    """no knob: 256 MiB hold 5 568 rows of 6 007 cells, so the driver cuts the walk itself (and carries the row sums
    and the cophenetic rows of the second strip to their places)"""
    n = COPH_DEFAULT_CUT
    rows = default_strip_rows(n, n)
    assert rows < n <= 2 * rows
    D = case_matrix(n, "random")
    Z = cluster.linkage(D, "average", ctx=ctx)
    got = cluster.cophenet(Z, D, matrix=True, ctx=ctx)
    assert_scores(got, D, Z, f"n={n} random average, two strips")
    assert (np.diag(got.cophenetic) == 0).all()


# ------------------------------------------------------------------ 3. nearest references, rows longer than 2048 cells
def _assert_twice(call, d, kk):
    got = call()
    assert_nearest(got, d, kk)
    again = call()
    assert np.array_equal(got[0], again[0]) and same_bits(got[1], again[1])
    return got


@pytest.mark.parametrize("mode", ["jsd", "euclidean"])
@pytest.mark.parametrize("n", NEAREST_REFS)
def test_nearest_over_rows_that_are_not_staged(ctx, mode, n):
    """2048 cells are the last row that is staged in LDS; longer ones are read from HBM on each of the kk passes"""
    assert n >= TOPK_LDS
    q, r = nearest_case(n)
    mq, mr = ctx.build_matrix(q, NEAREST_K, 4), ctx.build_matrix(r, NEAREST_K, 4)
    try:
        d = distance.matrix_cross_distances(mq, mr, mode)
        assert d.shape == (len(q), n)
        copies = copies_of_reference_2(n)
        assert (d[TIE_QUERY, copies] == 0.0).all() and not (np.delete(d[TIE_QUERY], copies) == 0.0).any()
        for kk in NEAREST_KK:
            idx, val = _assert_twice(lambda: distance.matrix_nearest(mq, mr, kk, mode), d, kk)
            assert (idx[3] == -1).all() and np.isnan(val[3]).all()  # a query without a valid k-mer: nothing listed
            assert not (idx == 2060).any() or n <= 2060             # a reference without: never listed
            head = copies[:kk]
            assert idx[TIE_QUERY, : len(head)].tolist() == head and (val[TIE_QUERY, : len(head)] == 0.0).all()
        if n == max(NEAREST_REFS):  # the same bits as the square path over the stacked rows
            ms = ctx.build_matrix(q + r, NEAREST_K, 4)
            try:
                square = {"jsd": distance.matrix_jsd_distances, "euclidean": distance.matrix_euclidean_distances}[mode]
                assert same_bits(d, square(ms)[: len(q), len(q):])
            finally:
                ms.close()
    finally:
        mq.close()
        mr.close()


@pytest.mark.parametrize("mode", ["jsd", "euclidean"])
def test_nearest_with_fewer_finite_cells_than_slots(ctx, mode):
    q, r, live = sparse_case()
    kk = max(NEAREST_KK)
    assert len(r) > TOPK_LDS and live.size == SPARSE_LIVE < kk
    mq, mr = ctx.build_matrix(q, NEAREST_K, 4), ctx.build_matrix(r, NEAREST_K, 4)
    try:
        d = distance.matrix_cross_distances(mq, mr, mode)
        assert np.array_equal(np.flatnonzero(~np.isnan(d).all(axis=0)), live)
        idx, val = _assert_twice(lambda: distance.matrix_nearest(mq, mr, kk, mode), d, kk)
        assert (idx[:, SPARSE_LIVE:] == -1).all() and np.isnan(val[:, SPARSE_LIVE:]).all()
        assert (np.sort(idx[:, :SPARSE_LIVE], axis=1) == live).all()  # the ten, in the stable order (assert_nearest)
    finally:
        mq.close()
        mr.close()


def test_mash_nearest_over_rows_that_are_not_staged(ctx):
    k, s, n = MASH_NEAREST["k"], MASH_NEAREST["sketch_size"], MASH_NEAREST["n"]
    assert n > TOPK_LDS
    q, r = mash_nearest_case()
    skq, skr = distance.Sketches(q, k, s, ctx=ctx), distance.Sketches(r, k, s, ctx=ctx)
    try:
        d = skq.cross_distances(skr)
        assert d.shape == (len(q), n) and not np.isnan(d).any()
        rng = np.random.default_rng(10)
        ii, jj = rng.integers(0, len(q), 500), rng.integers(0, n, 500)
        oq = {i: oracle.mash_sketch(q[i], k, s, 4, False) for i in set(ii.tolist())}
        orr = {j: oracle.mash_sketch(r[j], k, s, 4, False) for j in set(jj.tolist())}
        exp = np.array([oracle.mash_distance(oq[i], orr[j], k, s) for i, j in zip(ii.tolist(), jj.tolist())])
        np.testing.assert_allclose(d[ii, jj], exp, rtol=MASH_RTOL, atol=0)
        assert (d[2] == 1.0).all()  # the empty sketch: one tie over every column
        copies = [2, 2049, n - 1]
        assert (d[TIE_QUERY, copies] == 0.0).all()
        for kk in NEAREST_KK:
            idx, val = _assert_twice(lambda: skq.nearest(skr, kk), d, kk)
            assert idx[2].tolist() == list(range(kk))
            assert idx[TIE_QUERY, : min(kk, 3)].tolist() == copies[:kk]
    finally:
        skq.close()
        skr.close()


# ------------------------------------------------------------------ 4. cross mash, sketches longer than the staged row
def test_cross_mash_with_sketches_longer_than_the_staged_row(ctx):
    """the shared row of the cross instantiation read through L1 (9000 hashes against 8192 staged at most), the short
    query's row staged, in one launch; against the oracle's sketches and distances and the square entry's bits"""
    k, s = LONG_SKETCH["k"], LONG_SKETCH["sketch_size"]
    q, r = long_sketch_case()
    oq, orr, exp = long_sketch_oracle()
    assert max(x.size for x in oq) == s > PAIR_ROW_LDS and sum(x.size == s for x in oq) == len(q) - 1
    skq, skr, sks = (distance.Sketches(x, k, s, ctx=ctx) for x in (q, r, q + r))
    try:
        assert skq.stride == s and skr.stride == s
        hashes, lens = skq.to_host()
        for i, want in enumerate(oq):  # the rows the kernel reads are the oracle's sketches
            assert lens[i] == want.size and np.array_equal(hashes[i, : lens[i]], want)
        d = skq.cross_distances(skr)
        assert d.shape == (len(q), len(r))
        close = np.abs(d - exp) <= MASH_RTOL * np.abs(exp)
        assert ((d == exp) | close).all(), np.argwhere(~((d == exp) | close))[:5]
        assert (d[:, LONG_EMPTY_REF] == 1.0).all()
        assert same_bits(d, sks.distances()[: len(q), len(q):])
        assert same_bits(skr.cross_distances(skq), d.T)
    finally:
        for x in (skq, skr, sks):
            x.close()
