"""single, complete, weighted and ward linkage on the GPU (csrc/linkage.hip), and average through the same entry:
scipy's linkage matrix bit for bit and the Python restatements of tests/test_linkage_methods_host.py, ties included;
the device-tensor entry; the input errors; ctree(linkage=...) against scipy's tree of the same distances."""
import ctypes

import numpy as np
import pytest

from diverseseq_amd import _lib, cluster, distance, engine
from test_gpu_linkage import family_seqs
from test_linkage_host import tie_matrices
from test_linkage_methods_host import METHODS, restated, scipy_z

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("n", [2, 3, 5, 64, 255, 256, 257, 1000, 1025, 6007])
def test_uniform_matrices_bit_exact(ctx, n):
    """n = 6 007: 289 MB, more than the Infinity Cache"""
    d = np.random.default_rng(n).random((n, n))
    for method in METHODS:
        assert np.array_equal(cluster.linkage(d, method, ctx=ctx), scipy_z(d, method)), method


def test_tie_matrices_bit_exact(ctx):
    """heavy ties (integers 0..3), constant, all-zero, 2-decimal, negative, duplicated rows, non-symmetric; both
    oracles; ward refuses the negative ones"""
    for seed in (0, 1):
        for label, d in tie_matrices(seed):
            for method in METHODS:
                if method == "ward" and (np.triu(d, 1) < 0).any():
                    with pytest.raises(ValueError, match="non-negative"):
                        cluster.linkage(d, method, ctx=ctx)
                    continue
                got = cluster.linkage(d, method, ctx=ctx)
                assert np.array_equal(got, scipy_z(d, method)), (seed, label, method)
                assert np.array_equal(got, restated(d, method)), (seed, label, method)


@pytest.mark.parametrize("n", [300, 1000])
def test_large_tie_matrices_bit_exact(ctx, n):
    rng = np.random.default_rng(n + 2)
    for d in (rng.integers(0, 4, (n, n)).astype(np.float64), np.full((n, n), 0.5), np.zeros((n, n)),
              np.round(rng.random((n, n)), 2), rng.integers(0, 8, (n, n)) * 0.1):
        for method in METHODS:
            assert np.array_equal(cluster.linkage(d, method, ctx=ctx), scipy_z(d, method)), method


def test_negative_matrices_match_scipy_except_ward(ctx):
    rng = np.random.default_rng(21)
    for n in (2, 7, 64, 300):
        d = rng.random((n, n)) - 0.5
        for method in ("single", "complete", "average", "weighted"):
            assert np.array_equal(cluster.linkage(d, method, ctx=ctx), scipy_z(d, method)), (n, method)
        if (np.triu(d, 1) < 0).any():  # (at n = 2 the one entry that counts may be positive)
            with pytest.raises(ValueError, match="ward linkage needs non-negative distances"):
                cluster.linkage(d, "ward", ctx=ctx)
        else:
            assert np.array_equal(cluster.linkage(d, "ward", ctx=ctx), scipy_z(d, "ward"))


def test_ward_sign_rule_reads_the_upper_triangle_only(ctx):
    rng = np.random.default_rng(22)
    d = rng.random((97, 97))
    low = d.copy()
    low[np.tril_indices(97)] -= 2.0  # the diagonal and the lower triangle do not count
    assert np.array_equal(cluster.linkage(low, "ward", ctx=ctx), scipy_z(d, "ward"))
    one = d.copy()
    one[40, 96] = -1e-300
    with pytest.raises(ValueError, match="non-negative"):
        cluster.linkage(one, "ward", ctx=ctx)
    assert np.array_equal(cluster.linkage(d, "ward", ctx=ctx), scipy_z(d, "ward"))  # usable afterwards


def test_only_the_upper_triangle_counts_and_the_input_is_kept(ctx):
    rng = np.random.default_rng(5)
    d = rng.random((200, 200))
    keep = d.copy()
    sym = np.triu(d, 1) + np.triu(d, 1).T
    for method in METHODS:
        got = cluster.linkage(d, method, ctx=ctx)
        assert np.array_equal(d, keep)
        assert np.array_equal(got, scipy_z(d, method))
        assert np.array_equal(got, cluster.linkage(sym, method, ctx=ctx))


def test_average_through_the_new_entry_is_average_linkage(ctx):
    for seed in (0, 1):
        for label, d in tie_matrices(seed):
            assert np.array_equal(cluster.linkage(d, "average", ctx=ctx), cluster.average_linkage(d, ctx=ctx)), label
    d = np.random.default_rng(3).random((700, 700))
    assert np.array_equal(cluster.linkage(d, ctx=ctx), cluster.average_linkage(d, ctx=ctx))


def test_device_tensor_is_used_in_place_on_the_contexts_device_only(ctx):
    import torch

    d = np.random.default_rng(7).random((513, 513))
    for method in METHODS:
        t = torch.from_numpy(d).to("cuda:0")
        assert np.array_equal(cluster.linkage(t, method, ctx=ctx), scipy_z(d, method)), method
        assert not np.array_equal(t.cpu().numpy(), d)  # the working buffer (mirrored, at least)
    with pytest.raises(ValueError):
        cluster.linkage(torch.zeros((5, 5), dtype=torch.float32, device="cuda:0"), "single", ctx=ctx)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="on device 1"):
            cluster.linkage(torch.from_numpy(d).to("cuda:1"), "complete", ctx=ctx)


@pytest.mark.parametrize("where", [(0, 0), (2, 7), (7, 2), (99, 98)])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_anywhere_is_a_value_error(ctx, where, bad):
    d = np.random.default_rng(8).random((100, 100))
    d[where] = bad
    for method in METHODS:
        with pytest.raises(ValueError, match="NaN or infinity"):
            cluster.linkage(d, method, ctx=ctx)
    ok = np.random.default_rng(9).random((50, 50))  # the context is usable afterwards
    for method in METHODS:
        assert np.array_equal(cluster.linkage(ok, method, ctx=ctx), scipy_z(ok, method))


def test_unsupported_codes_at_the_c_boundary(ctx):
    d = np.random.default_rng(10).random((6, 6))
    pairs, heights, sizes = distance.tree_outputs(6)
    args = (_lib.ptr(pairs, ctypes.c_uint32), _lib.ptr(heights, ctypes.c_double), _lib.ptr(sizes, ctypes.c_uint32))
    src = distance.make_source(_lib.SRC_GIVEN, d.ctypes.data, 6)
    for code, rc in ((3, _lib.ERR_UNSUPPORTED), (4, _lib.ERR_UNSUPPORTED), (7, _lib.ERR_VALUE), (-1, _lib.ERR_VALUE)):
        assert ctx._L.dvs_linkage(ctx._h, src, code, *args) == rc, code
    for name, code in distance.LINKAGE_METHODS.items():
        assert ctx._L.dvs_linkage(ctx._h, src, code, *args) == _lib.OK
        assert np.array_equal(distance.linkage_matrix(pairs, heights, sizes), scipy_z(d, name)), name


# ---- ctree(linkage=...): the fused device tree against scipy's tree of the same distances, string for string ------
def scipy_newick(names, dists, method):
    return cluster.linkage_to_newick(names, scipy_z(dists, method))


@pytest.mark.parametrize("method", METHODS)
def test_ctree_brca1_methods(brca1, method):
    names = list(brca1)
    arrays = [brca1[n] for n in names]
    assert len(names) == 55
    mash = distance.mash_distances(arrays, 16, 400)
    assert cluster.ctree(brca1, k=16, sketch_size=400, linkage=method) == scipy_newick(names, mash, method)
    euc = distance.euclidean_distances(arrays, 5)
    assert (cluster.ctree(brca1, k=5, sketch_size=None, distance_mode="euclidean", tree="device", linkage=method)
            == scipy_newick(names, euc, method))
    if method != "average":
        with pytest.raises(ValueError, match="average linkage only"):
            cluster.ctree(brca1, k=16, sketch_size=400, tree="sklearn", linkage=method)


@pytest.mark.parametrize("method", METHODS)
def test_ctree_family_sequences_with_duplicates(method):
    """mutated families with exact copies: zero distances and ties through the fused entries"""
    seqs = family_seqs(12, 25, 4_000, seed=13)
    names = list(seqs)
    arrays = [seqs[n] for n in names]
    mash = distance.mash_distances(arrays, 12, 1000)
    assert cluster.ctree(seqs, k=12, sketch_size=1000, linkage=method) == scipy_newick(names, mash, method)
    euc = distance.euclidean_distances(arrays, 4)
    assert (cluster.ctree(seqs, k=4, sketch_size=None, distance_mode="euclidean", linkage=method)
            == scipy_newick(names, euc, method))


def test_fused_entries_keep_their_errors():
    empty = {"a": np.zeros(3, np.uint8), "b": np.ones(2, np.uint8), "c": np.arange(40, dtype=np.uint8) % 4}
    no_kmers = {"a": np.full(50, 4, np.uint8), "b": np.arange(50, dtype=np.uint8) % 4, "c": np.ones(50, np.uint8)}
    for method in METHODS:
        with pytest.raises(ZeroDivisionError):  # two empty sketches (distance.py:283)
            cluster.ctree(empty, k=8, sketch_size=10, linkage=method)
        with pytest.raises(ValueError):  # NaN distances of a row without valid k-mers
            cluster.ctree(no_kmers, k=3, sketch_size=None, distance_mode="euclidean", linkage=method)
