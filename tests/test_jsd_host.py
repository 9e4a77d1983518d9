"""The Jensen-Shannon distance mode without a GPU: the public names exist, the argument checks of `ctree` and
`apps.dvs_dist`, no CPU fall-back, and the definition itself -- the oracle's two-member total_jsd
(src/records.rs:27-68), which the GPU tests (tests/test_gpu_jsd.py) use as their yardstick -- pinned against scipy's
jensenshannon(base=2) ** 2 and against the reference's BRCA1 topologies."""
import ctypes

import numpy as np
import pytest

import oracle
from conftest import clades, str2arr
from diverseseq_amd import _lib, apps, cluster, distance
from test_cluster import EXPECT


def pair_jsd(fa, ha, fb, hb) -> float:
    """the oracle's JSD of two frequency rows: total_jsd of SummedRecords::new([a, b])"""
    return oracle.SummedRecords.new(np.stack([fa, fb]), [ha, hb]).total_jsd


def oracle_jsd_matrix(seqs, k: int, num_states: int = 4) -> np.ndarray:
    """every cell by `pair_jsd`; 0 on the diagonal; NaN off the diagonal for a sequence without a valid k-mer"""
    n = len(seqs)
    valid = [oracle.count_kmers(s, num_states, k).sum() > 0 for s in seqs]
    fh = [oracle.to_kfreqs(s, num_states, k) if v else None for s, v in zip(seqs, valid)]
    d = np.zeros((n, n))
    for i in range(n):
        for j in range(i):
            d[i, j] = d[j, i] = pair_jsd(*fh[i], *fh[j]) if valid[i] and valid[j] else np.nan
    return d


def test_public_names_exist():
    assert callable(distance.jsd_distances) and callable(distance.jsd_linkage)
    assert callable(apps.dvs_dist) and "dvs_dist" in apps.__all__
    assert {"dvs_distances", "dvs_linkage"} <= set(_lib.EXPORTS) and _lib.SRC_JSD == 2  # the mode travels in the dvs_source


def test_dvs_dist_constructor_checks():
    """diverse_seq/distance.py:67-80"""
    with pytest.raises(ValueError, match="Unexpected distance 'manhattan'"):
        apps.dvs_dist("manhattan")
    with pytest.raises(ValueError, match="Expected sketch size for mash distance measure"):
        apps.dvs_dist("mash", sketch_size=None)
    with pytest.raises(ValueError, match="Canonical kmers only supported for dna sequences"):
        apps.dvs_dist("mash", moltype="protein", mash_canonical_kmers=True)
    for mode in ("mash", "euclidean", "jsd"):
        apps.dvs_dist(mode)
    apps.dvs_dist("jsd", sketch_size=None, k=3)
    for app in (apps.dvs_ctree, apps.dvs_par_ctree):
        app(distance_mode="jsd", sketch_size=None, k=4)
        app(distance_mode="jsd")  # (the sketch size is dropped, as for euclidean)
        with pytest.raises(ValueError, match="Unexpected distance"):
            app(distance_mode="manhattan")


def test_ctree_jsd_argument_checks():
    seqs = {"a": np.zeros(30, np.uint8), "b": np.ones(30, np.uint8)}
    with pytest.raises(ValueError, match="Sketch size"):
        cluster.ctree(seqs, distance_mode="jsd", sketch_size=10)
    with pytest.raises(ValueError, match="Canonical kmers"):
        cluster.ctree(seqs, distance_mode="jsd", sketch_size=None, mash_canonical_kmers=True)
    with pytest.raises(ValueError, match="Unexpected distance"):
        cluster.ctree(seqs, distance_mode="jensen")


def _has_gpu():
    lib = _lib.load()
    h = ctypes.c_void_p()
    rc = lib.dvs_ctx_create(-1, None, ctypes.byref(h))
    if rc == 0:
        lib.dvs_ctx_destroy(h)
    return rc == 0


def test_jsd_has_no_cpu_fallback():
    if _has_gpu():
        pytest.skip("a GPU is visible")
    seqs = {"a": np.zeros(30, np.uint8), "b": np.ones(30, np.uint8), "c": np.arange(30, dtype=np.uint8) % 4}
    for tree in ("device", "sklearn"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cluster.ctree(seqs, distance_mode="jsd", sketch_size=None, k=2, tree=tree)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        distance.jsd_distances(list(seqs.values()), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        apps.dvs_dist("jsd", k=2)({"a": "ACGTACGT", "b": "AACCGGTT"})


@pytest.mark.parametrize("k", [1, 2, 6, 7])
@pytest.mark.parametrize("length", [50, 300, 5000])
def test_oracle_pair_jsd_is_the_squared_jensen_shannon_distance(k, length):
    """the yardstick of the GPU tests: order-independent, within 1e-11 of scipy's jensenshannon(base=2) ** 2 (two
    independent f64 evaluations; 8.3e-13 at most on these inputs), exactly 0 for a duplicate"""
    from scipy.spatial.distance import jensenshannon

    rng = np.random.default_rng(100 * k + length)
    seqs = [rng.integers(0, 4, length, dtype=np.uint8) for _ in range(5)]
    seqs.append(seqs[2].copy())
    fh = [oracle.to_kfreqs(s, 4, k) for s in seqs]
    worst = 0.0
    for i in range(len(seqs)):
        for j in range(i):
            d = pair_jsd(*fh[i], *fh[j])
            assert d == pair_jsd(*fh[j], *fh[i])
            diff = abs(d - jensenshannon(fh[i][0], fh[j][0], base=2) ** 2)
            worst = max(worst, diff)
            assert diff <= 1e-11, (i, j, d, diff)
    print(f"k={k} L={length}: largest |oracle - scipy| = {worst:.3g}")
    assert pair_jsd(*fh[5], *fh[2]) == 0.0


def test_oracle_pair_jsd_of_disjoint_sequences_is_one():
    """paper/paper.md Table 1"""
    a, b = oracle.to_kfreqs(str2arr("AAAA"), 4, 1), oracle.to_kfreqs(str2arr("TTTT"), 4, 1)
    assert pair_jsd(*a, *b) == 1.0
    assert pair_jsd(*a, *a) == 0.0


@pytest.mark.parametrize("k", [3, 4, 5, 6, 7])
def test_average_linkage_over_oracle_jsd_gives_the_reference_topologies(brca1, k):
    for names, newick in EXPECT.items():
        d = oracle_jsd_matrix([brca1[n] for n in names], k)
        got = cluster.make_cluster_tree(list(names), d)
        assert clades(got) == clades(newick), (k, got, newick)
