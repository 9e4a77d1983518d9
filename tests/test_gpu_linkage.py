"""The average-linkage tree on the GPU (csrc/linkage.hip): scipy's linkage matrix bit for bit, the device-pointer
entry, ctree(tree="device") against the sklearn path string for string, and the errors the host path raises."""
import numpy as np
import pytest

from conftest import GOLDEN, read_fasta
from diverseseq_amd import cluster, engine
from test_linkage_host import nn_chain_average, scipy_z, tie_matrices

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
    got = cluster.average_linkage(d, ctx=ctx)
    assert np.array_equal(got, scipy_z(d))


def test_tie_matrices_bit_exact(ctx):
    """heavy ties (integers 0..3), constant, all-zero, 2-decimal, negative, duplicated rows, non-symmetric; both
    oracles"""
    for seed in (0, 1):
        for label, d in tie_matrices(seed):
            got = cluster.average_linkage(d, ctx=ctx)
            assert np.array_equal(got, scipy_z(d)), (seed, label)
            assert np.array_equal(got, nn_chain_average(d)), (seed, label)


@pytest.mark.parametrize("n", [300, 1000])
def test_large_tie_matrices_bit_exact(ctx, n):
    rng = np.random.default_rng(n + 1)
    for d in (rng.integers(0, 4, (n, n)).astype(np.float64), np.full((n, n), 0.5), np.zeros((n, n)),
              np.round(rng.random((n, n)), 2), rng.random((n, n)) - 0.5):
        assert np.array_equal(cluster.average_linkage(d, ctx=ctx), scipy_z(d))


def test_only_the_upper_triangle_counts_and_the_input_is_kept(ctx):
    rng = np.random.default_rng(5)
    d = rng.random((200, 200))
    keep = d.copy()
    got = cluster.average_linkage(d, ctx=ctx)
    assert np.array_equal(d, keep)
    assert np.array_equal(got, scipy_z(d))
    sym = np.triu(d, 1) + np.triu(d, 1).T
    assert np.array_equal(got, cluster.average_linkage(sym, ctx=ctx))


def test_float32_and_list_input(ctx):
    d = np.random.default_rng(6).random((97, 97)).astype(np.float32)
    assert np.array_equal(cluster.average_linkage(d, ctx=ctx), scipy_z(d.astype(np.float64)))
    small = [[0, 1, 4], [1, 0, 2], [4, 2, 0]]
    assert np.array_equal(cluster.average_linkage(small, ctx=ctx), scipy_z(np.array(small, dtype=np.float64)))


def test_device_tensor_is_used_in_place(ctx):
    import torch

    d = np.random.default_rng(7).random((513, 513))
    t = torch.from_numpy(d).to("cuda:0")
    got = cluster.average_linkage(t, ctx=ctx)
    assert np.array_equal(got, scipy_z(d))
    assert not np.array_equal(t.cpu().numpy(), d)  # the working buffer


def test_device_tensor_shape_checks(ctx):
    import torch

    with pytest.raises(ValueError):
        cluster.average_linkage(torch.zeros((4, 5), dtype=torch.float64, device="cuda:0"), ctx=ctx)
    with pytest.raises(ValueError):
        cluster.average_linkage(torch.zeros((5, 5), dtype=torch.float32, device="cuda:0"), ctx=ctx)
    with pytest.raises(ValueError):
        cluster.average_linkage(torch.zeros((6, 6), dtype=torch.float64, device="cuda:0")[:5, :5], ctx=ctx)


@pytest.mark.parametrize("where", [(0, 0), (3, 3), (2, 7), (7, 2), (99, 98)])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_anywhere_is_a_value_error(ctx, where, bad):
    d = np.random.default_rng(8).random((100, 100))
    d[where] = bad
    with pytest.raises(ValueError):
        cluster.average_linkage(d, ctx=ctx)
    ok = np.random.default_rng(9).random((50, 50))  # the context is usable afterwards
    assert np.array_equal(cluster.average_linkage(ok, ctx=ctx), scipy_z(ok))


def test_fewer_than_two_is_a_value_error(ctx):
    for d in (np.zeros((1, 1)), np.zeros((0, 0)), np.zeros((3, 4))):
        with pytest.raises(ValueError):
            cluster.average_linkage(d, ctx=ctx)
    with pytest.raises(ValueError):
        cluster.ctree({"a": np.zeros(40, np.uint8)}, k=4, sketch_size=10)


# ---- ctree: the device tree against the sklearn path, string for string ----------------------------------------
SETS = [("Human", "Chimpanzee", "Rhesus", "Horse"), ("Human", "Chimpanzee", "Manatee", "Dugong"),
        ("Human", "Chimpanzee", "Manatee", "Dugong", "Rhesus"), None]
MODES = [dict(k=16, sketch_size=400), dict(k=16, sketch_size=4_000_000_000),
         dict(k=5, sketch_size=None, distance_mode="euclidean")]


@pytest.mark.parametrize("names", SETS, ids=["set1", "set2", "set3", "all"])
@pytest.mark.parametrize("kw", MODES, ids=["mash400", "mash4e9", "euclid5"])
def test_ctree_brca1_device_equals_sklearn(brca1, names, kw):
    seqs = {n: brca1[n] for n in (names or brca1)}
    if names is None:
        assert len(seqs) == 55
    assert cluster.ctree(seqs, tree="device", **kw) == cluster.ctree(seqs, tree="sklearn", **kw)
    assert cluster.ctree(seqs, **kw) == cluster.ctree(seqs, tree="sklearn", **kw)


def family_seqs(nfam: int, per: int, length: int, seed: int) -> dict:
    """mutated families (1-8 % substitutions, some gaps) with exact duplicates: structure and ties"""
    rng = np.random.default_rng(seed)
    out = {}
    for f in range(nfam):
        root = rng.integers(0, 4, length, dtype=np.uint8)
        for m in range(per):
            s = root.copy()
            if m % 7 != 3:  # every seventh member an exact copy of the root
                hit = rng.random(length) < rng.uniform(0.01, 0.08)
                s[hit] = rng.integers(0, 4, int(hit.sum()), dtype=np.uint8)
                s[rng.random(length) < 0.001] = 4
            out[f"fam{f}_m{m}"] = s
    return out


@pytest.mark.parametrize("kw", [dict(), dict(k=5, sketch_size=None, distance_mode="euclidean")], ids=["mash", "euclid5"])
def test_ctree_1000_family_sequences_device_equals_sklearn(kw):
    seqs = family_seqs(50, 20, 20_000, seed=11)
    assert len(seqs) == 1000
    assert cluster.ctree(seqs, tree="device", **kw) == cluster.ctree(seqs, tree="sklearn", **kw)


def test_dvs_ctree_app_uses_the_device_tree():
    from diverseseq_amd import apps

    raw = read_fasta(GOLDEN / "brca1.fasta")
    text = {n: s.replace("-", "").replace("?", "") for n, s in list(raw.items())[:20]}
    for kw in (dict(k=12, sketch_size=3000), dict(k=4, sketch_size=None, distance_mode="euclidean")):
        names, data, _ = apps._as_mapping(text, "dna")
        arrays = {n: np.frombuffer(data[n], dtype=np.uint8) for n in names}
        expect = cluster.ctree(arrays, tree="sklearn", **kw)
        assert apps.dvs_ctree(**kw)(text) == expect
        assert apps.dvs_par_ctree(max_workers=2, **kw)(text) == expect


def test_ctree_errors_as_the_sklearn_path():
    empty = {"a": np.zeros(3, np.uint8), "b": np.ones(2, np.uint8), "c": np.arange(40, dtype=np.uint8) % 4}
    for tree in ("device", "sklearn"):
        with pytest.raises(ZeroDivisionError):  # two empty sketches (distance.py:283)
            cluster.ctree(empty, k=8, sketch_size=10, tree=tree)
    no_kmers = {"a": np.full(50, 4, np.uint8), "b": np.arange(50, dtype=np.uint8) % 4, "c": np.ones(50, np.uint8)}
    for tree in ("device", "sklearn"):
        with pytest.raises(ValueError):  # NaN distances of a row without valid k-mers
            cluster.ctree(no_kmers, k=3, sketch_size=None, distance_mode="euclidean", tree=tree)
