"""Pairwise Jensen-Shannon distances on the GPU (csrc/rowdist.hip): every cell against the oracle's two-member total_jsd
(src/records.rs:27-68; tests/test_jsd_host.py pins that yardstick on the CPU) within tol_derived(bins), the bound a
correct f64 evaluation keeps (tests/test_distance_truth_host.py; tests/test_gpu_distance_truth.py compares with the
long-double truth itself); the exact properties of the matrix; the fused tree bit for bit against scipy over the
device's own matrix; ctree and the apps."""
import numpy as np
import pytest

import oracle
from conftest import GOLDEN, clades, read_fasta, str2arr, synth_seqs
from diverseseq_amd import apps, cluster, distance, engine
from test_cluster import EXPECT
from test_distance_truth_host import tol_derived
from test_gpu_linkage import family_seqs
from test_jsd_host import oracle_jsd_matrix
from test_linkage_methods_host import METHODS, scipy_z

pytestmark = pytest.mark.gpu

TOL = 1e-9
JSD_TILE = 32  # rows of a workgroup's tile on either side (csrc/rowdist.hip)


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context()


def _dna(rng, n):
    return rng.integers(0, 4, size=n, dtype=np.uint8)


def assert_jsd_matrix(d, seqs, k, num_states=4, empty=()):
    """the properties of "The quantity" and every cell against the oracle; -> the largest difference seen"""
    n = len(seqs)
    assert d.shape == (n, n) and d.dtype == np.float64
    assert (np.diag(d) == 0).all()
    np.testing.assert_array_equal(d, d.T)
    off = ~np.eye(n, dtype=bool)
    nan = np.zeros((n, n), dtype=bool)
    for e in empty:
        nan[e, :] = nan[:, e] = True
    np.testing.assert_array_equal(np.isnan(d), nan & off)
    ok = off & ~nan
    assert (d[ok] >= 0.0).all() and (d[ok] <= 1.0).all()
    exp = oracle_jsd_matrix(seqs, k, num_states)
    np.testing.assert_array_equal(np.isnan(exp), nan & off)
    worst = float(np.abs(d[ok] - exp[ok]).max()) if ok.any() else 0.0
    print(f"n={n} k={k} states={num_states}: largest |D - oracle| = {worst:.3g}")
    assert worst <= tol_derived(num_states ** k)
    return worst


# ------------------------------------------------------------------ 1. every cell against the oracle
@pytest.mark.parametrize("k", [1, 6, 7])
@pytest.mark.parametrize("n", [2, 7, 8, 9, 17])
@pytest.mark.parametrize("u32", [False, True])
def test_jsd_all_pairs(ctx, monkeypatch, k, n, u32):
    """the grid of test_euclidean_all_pairs (tests/test_gpu_sketch.py): 4 / 4 096 / 16 384 bins, 16- and 32-bit
    count rows, 5 % invalid symbols in row 0, from N = 7 on a last row without a valid k-mer"""
    if u32:
        monkeypatch.setenv("DVS_COUNTS_U32", "1")
    rng = np.random.default_rng(10 * k + n)
    empty_row = n > 2
    seqs = [_dna(rng, int(rng.integers(200, 3000))) for _ in range(n - 1 if empty_row else n)]
    seqs[0][rng.random(seqs[0].size) < 0.05] = 4
    if empty_row:
        seqs.append(np.full(50, 4, np.uint8) if n % 2 else _dna(rng, k - 1))
    d = distance.jsd_distances(seqs, k, 4, ctx=ctx)
    assert_jsd_matrix(d, seqs, k, empty=(n - 1,) if empty_row else ())
    assert (d[~np.isnan(d) & ~np.eye(n, dtype=bool)] > 0).all()  # (random sequences differ)


@pytest.mark.parametrize("n", [JSD_TILE - 1, JSD_TILE, JSD_TILE + 1, 2 * JSD_TILE - 1, 2 * JSD_TILE, 2 * JSD_TILE + 1])
def test_jsd_tile_edges(ctx, n):
    """N on both sides of one tile and of two (the matrix is square: the i- and the j-edge move together, and the
    second edge puts a partial tile beside full ones in either direction), an empty row in the middle"""
    rng = np.random.default_rng(n)
    seqs = [_dna(rng, int(rng.integers(100, 900))) for _ in range(n)]
    seqs[n // 2] = np.full(30, 4, np.uint8)
    assert_jsd_matrix(distance.jsd_distances(seqs, 4, 4, ctx=ctx), seqs, 4, empty=(n // 2,))


def test_jsd_protein_alphabet(ctx):
    rng = np.random.default_rng(20)
    seqs = [rng.integers(0, 20, size=int(rng.integers(150, 800)), dtype=np.uint8) for _ in range(11)]
    seqs[3][rng.random(seqs[3].size) < 0.05] = 20
    assert_jsd_matrix(distance.jsd_distances(seqs, 2, 20, ctx=ctx), seqs, 2, num_states=20)


@pytest.mark.parametrize("u32", [False, True])
def test_jsd_duplicates_are_exactly_zero(ctx, monkeypatch, u32):
    if u32:
        monkeypatch.setenv("DVS_COUNTS_U32", "1")
    rng = np.random.default_rng(3)
    for k in (1, 3, 6, 7):
        seqs = [_dna(rng, 1500) for _ in range(40)]
        seqs[37] = seqs[2].copy()  # another tile row, the same tile
        seqs[5] = seqs[2].copy()
        seqs[1] = seqs[0][::-1].copy() if k == 1 else seqs[1]  # (k = 1: the same counts in another order of bases)
        d = distance.jsd_distances(seqs, k, 4, ctx=ctx)
        assert d[37, 2] == 0.0 and d[2, 37] == 0.0 and d[5, 2] == 0.0 and d[37, 5] == 0.0
        if k == 1:
            assert d[1, 0] == 0.0
        assert (d[3, :3] > 0).all()
    # a sequence against its own copy under other names
    a = _dna(rng, 4000)
    assert distance.jsd_distances([a, a.copy()], 5, ctx=ctx)[1, 0] == 0.0
    assert distance.jsd_distances([a.copy(), _dna(rng, 50), a], 5, ctx=ctx)[2, 0] == 0.0


@pytest.mark.parametrize("k", [1, 3])
def test_jsd_disjoint_alphabets_give_one(ctx, k):
    """paper/paper.md Table 1: no k-mer in common -> 1.0, never more"""
    d = distance.jsd_distances([str2arr("A" * 40), str2arr("T" * 40), str2arr("A" * 17)], k, ctx=ctx)
    for i, j in ((1, 0), (2, 1)):
        assert abs(d[i, j] - 1.0) <= TOL and d[i, j] <= 1.0, d[i, j]
    assert d[2, 0] == 0.0  # (the same frequencies from other counts: 1.0 in one bin, whatever the total)


def test_jsd_of_frequency_rows(ctx):
    """a matrix of f64 rows (matrix_from_freqs) gives the same cells"""
    rng = np.random.default_rng(8)
    seqs = [_dna(rng, int(rng.integers(300, 2500))) for _ in range(35)]
    for k in (2, 6):
        f = np.stack([oracle.to_kfreqs(s, 4, k)[0] for s in seqs])
        m = ctx.matrix_from_freqs(f)
        try:
            d = distance.matrix_jsd_distances(m)
        finally:
            m.close()
        assert_jsd_matrix(d, seqs, k)
        assert np.abs(d - distance.jsd_distances(seqs, k, ctx=ctx)).max() <= TOL


# ------------------------------------------------------------------ 2. BASELINE-sized rows
@pytest.mark.parametrize("length,k", [(2000, 6), (5000, 7)], ids=["C2", "C4"])
def test_jsd_baseline_shapes(ctx, length, k):
    seqs = synth_seqs(40, length, 55 + k, invalid_frac=0.001, ragged=True)
    assert_jsd_matrix(distance.jsd_distances(seqs, k, 4, ctx=ctx), seqs, k)


# ------------------------------------------------------------------ 3. the tree, bit for bit
@pytest.fixture(scope="module")
def family():
    seqs = family_seqs(50, 20, 20_000, seed=11)
    assert len(seqs) == 1000
    return seqs


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("which", ["family", "brca1"])
def test_jsd_linkage_is_scipy_over_the_device_matrix(ctx, brca1, family, which, method):
    arrays = list((family if which == "family" else brca1).values())
    assert len(arrays) == (1000 if which == "family" else 55)
    d = distance.jsd_distances(arrays, 5, ctx=ctx)
    assert np.array_equal(d, distance.jsd_distances(arrays, 5, ctx=ctx))  # (deterministic)
    if which == "family":
        assert (d[np.triu_indices(len(arrays), 1)] == 0).sum() >= 50  # (exact duplicates: ties at 0)
    z = distance.jsd_linkage(arrays, 5, method=method, ctx=ctx)
    assert np.array_equal(z, scipy_z(d, method))
    assert np.array_equal(z, cluster.linkage(d, method, ctx=ctx))  # (the fused matrix is the standalone one)


# ------------------------------------------------------------------ 4. ctree
def test_ctree_jsd_reference_topologies(brca1):
    for names, newick in EXPECT.items():
        for tree in ("device", "sklearn"):
            got = cluster.ctree({n: brca1[n] for n in names}, distance_mode="jsd", k=5, sketch_size=None, tree=tree)
            assert clades(got) == clades(newick), (tree, got, newick)


@pytest.mark.parametrize("names", [*EXPECT, None], ids=["set1", "set2", "set3", "all"])
def test_ctree_jsd_device_equals_sklearn(brca1, names):
    seqs = {n: brca1[n] for n in (names or brca1)}
    kw = dict(distance_mode="jsd", k=5, sketch_size=None)
    assert cluster.ctree(seqs, tree="device", **kw) == cluster.ctree(seqs, tree="sklearn", **kw)
    assert cluster.ctree(seqs, **kw) == cluster.ctree(seqs, tree="sklearn", **kw)


def test_ctree_jsd_family_sequences_device_equals_sklearn(family):
    kw = dict(distance_mode="jsd", k=5, sketch_size=None)
    assert cluster.ctree(family, tree="device", **kw) == cluster.ctree(family, tree="sklearn", **kw)


@pytest.mark.parametrize("method", METHODS)
def test_ctree_jsd_takes_every_linkage(brca1, method):
    from scipy.cluster.hierarchy import linkage as scipy_linkage

    names, arrays = list(brca1), list(brca1.values())
    d = distance.jsd_distances(arrays, 5)
    expect = cluster.linkage_to_newick(names, scipy_linkage(d[np.triu_indices(len(names), 1)], method))
    assert cluster.ctree(brca1, distance_mode="jsd", k=5, sketch_size=None, linkage=method) == expect


def test_ctree_jsd_row_without_kmers_is_a_value_error():
    no_kmers = {"a": np.full(50, 4, np.uint8), "b": np.arange(50, dtype=np.uint8) % 4, "c": np.ones(50, np.uint8)}
    for tree in ("device", "sklearn"):
        with pytest.raises(ValueError):
            cluster.ctree(no_kmers, k=3, sketch_size=None, distance_mode="jsd", tree=tree)
    for method in METHODS:
        with pytest.raises(ValueError):
            distance.jsd_linkage(list(no_kmers.values()), 3, method=method)
    ok = {"a": np.zeros(50, np.uint8), **{n: no_kmers[n] for n in "bc"}}  # the context is usable afterwards
    assert cluster.ctree(ok, k=3, sketch_size=None, distance_mode="jsd").endswith(";")


def test_jsd_degenerate_sizes(ctx):
    a = np.arange(60, dtype=np.uint8) % 4
    assert np.array_equal(distance.jsd_distances([a], 3, ctx=ctx), np.zeros((1, 1)))
    with pytest.raises(ValueError):
        distance.jsd_linkage([a], 3, ctx=ctx)
    with pytest.raises(ValueError):
        distance.jsd_linkage([a, a], 3, method="centroid", ctx=ctx)


# ------------------------------------------------------------------ 5. apps
def _text20():
    raw = read_fasta(GOLDEN / "brca1.fasta")
    return {n: s.replace("-", "").replace("?", "") for n, s in list(raw.items())[:20]}


def test_ctree_apps_take_jsd():
    text = _text20()
    kw = dict(k=4, sketch_size=None, distance_mode="jsd")
    names, data, _ = apps._as_mapping(text, "dna")
    arrays = {n: np.frombuffer(data[n], dtype=np.uint8) for n in names}
    expect = cluster.ctree(arrays, **kw)
    assert expect == cluster.ctree(arrays, tree="sklearn", **kw)
    assert apps.dvs_ctree(**kw)(text) == expect
    assert apps.dvs_par_ctree(max_workers=2, **kw)(text) == expect


@pytest.mark.parametrize("mode", ["mash", "euclidean", "jsd"])
def test_dvs_dist_app(mode):
    text = _text20()
    names, data, _ = apps._as_mapping(text, "dna")
    arrays = [np.frombuffer(data[n], dtype=np.uint8) for n in names]
    if mode == "mash":
        app, expect = apps.dvs_dist("mash", k=12, sketch_size=400), distance.mash_distances(arrays, 12, 400)
    elif mode == "euclidean":
        app, expect = apps.dvs_dist("euclidean", k=4), distance.euclidean_distances(arrays, 4)
    else:
        app, expect = apps.dvs_dist("jsd", k=4), distance.jsd_distances(arrays, 4)
    got = app(text)
    if apps.HAVE_COGENT3:  # pragma: no cover
        got_names, got_d = list(got.names), np.asarray(got.array)
    else:
        got_names, got_d = got
    assert got_names == list(text)
    assert np.array_equal(got_d, expect)
    assert (expect[~np.eye(len(names), dtype=bool)] > 0).any()
