"""The host half of the device tree (no GPU): `cluster.linkage_to_newick` against `make_cluster_tree`, and a
plain-Python restatement of scipy's nearest-neighbour chain -- the second oracle of the GPU linkage tests
(tests/test_gpu_linkage.py) -- against scipy itself."""
import numpy as np
import pytest
from scipy.cluster.hierarchy import linkage

from diverseseq_amd import cluster


def scipy_z(d: np.ndarray) -> np.ndarray:
    """what sklearn's AgglomerativeClustering(metric="precomputed", linkage="average") runs"""
    d = np.asarray(d, dtype=np.float64)
    return linkage(d[np.triu_indices(d.shape[0], 1)], "average")


def nn_chain_average(d) -> np.ndarray:
    """scipy's _hierarchy.nn_chain (average linkage) and `label`, restated over the upper triangle of d"""
    n = len(d)
    D = np.array(d, dtype=np.float64)
    D = np.triu(D, 1) + np.triu(D, 1).T
    D = [[float(v) for v in row] for row in D]
    size = [1] * n
    chain: list[int] = []
    rec = []
    for _ in range(n - 1):
        if not chain:
            chain.append(next(i for i in range(n) if size[i] > 0))
        while True:
            x = chain[-1]
            if len(chain) > 1:
                y = chain[-2]
                cur = D[x][y]  # the previous element wins ties
            else:
                y, cur = -1, float("inf")
            for i in range(n):
                if size[i] > 0 and i != x and D[x][i] < cur:  # strict <: the lowest index wins ties
                    cur, y = D[x][i], i
            if len(chain) > 1 and y == chain[-2]:
                break
            chain.append(y)
        chain.pop()
        chain.pop()
        a, b = min(x, y), max(x, y)
        na, nb = size[a], size[b]
        rec.append((a, b, cur, na + nb))
        size[a], size[b] = 0, na + nb
        for i in range(n):
            if size[i] > 0 and i != b:
                D[i][b] = D[b][i] = (float(na) * D[i][a] + float(nb) * D[i][b]) / float(na + nb)
    order = np.argsort(np.array([r[2] for r in rec]), kind="mergesort")
    parent = list(range(2 * n - 1))
    usize = [1] * (2 * n - 1)

    def find(v):
        while parent[v] != v:
            v = parent[v]
        return v

    z = np.zeros((n - 1, 4))
    for j, q in enumerate(order):
        xr, yr = find(rec[q][0]), find(rec[q][1])
        parent[xr] = parent[yr] = n + j
        usize[n + j] = usize[xr] + usize[yr]
        z[j] = (min(xr, yr), max(xr, yr), rec[q][2], usize[n + j])
    return z


def tie_matrices(seed: int):
    """(label, matrix) pairs: uniform, heavy ties, constant, zero, rounded, negative, duplicated rows, non-symmetric"""
    rng = np.random.default_rng(seed)
    for n in (2, 3, 4, 5, 8, 17, 40, 120):
        u = rng.random((n, n))
        yield f"uniform{n}", u
        yield f"int{n}", rng.integers(0, 4, (n, n)).astype(np.float64)
        yield f"rounded{n}", np.round(u, 2)
        yield f"negative{n}", u - 0.5
    yield "constant", np.full((30, 30), 0.25)
    yield "zero", np.zeros((30, 30))
    base = rng.random((10, 40))
    rows = base[rng.integers(0, 10, 60)]
    dup = np.sqrt(((rows[:, None, :] - rows[None, :, :]) ** 2).sum(-1))
    yield "duplicated_rows", dup
    yield "nonsymmetric", rng.random((33, 33))


def test_restatement_matches_scipy():
    """the second oracle is scipy's Z bit for bit, ties included (72 matrices)"""
    count = 0
    for seed in (0, 1):
        for label, d in tie_matrices(seed):
            exp = scipy_z(d)
            got = nn_chain_average(d)
            assert np.array_equal(got, exp), (seed, label)
            count += 1
    assert count == 72


@pytest.mark.parametrize("n", [2, 3, 4, 5, 7, 10, 31, 64, 100, 300])
def test_newick_matches_make_cluster_tree(n):
    rng = np.random.default_rng(n)
    d = rng.random((n, n))
    d = d + d.T
    np.fill_diagonal(d, 0.0)
    names = [f"s{i}" for i in range(n)]
    assert cluster.linkage_to_newick(names, scipy_z(d)) == cluster.make_cluster_tree(names, d)
    ties = rng.integers(0, 3, (n, n)).astype(np.float64)
    assert cluster.linkage_to_newick(names, scipy_z(ties)) == cluster.make_cluster_tree(names, ties)


@pytest.mark.parametrize("names", [
    ["it's", 'say "hi"', "two words", "naïve", "日本", "plain", "'quoted'", "a\\b"],
    [3, 1, 4, 15, 9, 2, 6, 5],
    ["x", 7, "y's", 2.5, "z", "w", ("t", 1), None],
])
def test_newick_names_as_make_cluster_tree_prints_them(names):
    rng = np.random.default_rng(len(str(names)))
    d = rng.random((len(names), len(names)))
    assert cluster.linkage_to_newick(names, scipy_z(d)) == cluster.make_cluster_tree(names, d)


def caterpillar(n: int) -> np.ndarray:
    i = np.arange(n, dtype=np.float64)
    return np.maximum(i[:, None], i[None, :]) + 1.0


def caterpillar_newick(n: int) -> str:
    return "".join(f"(s{i}, " for i in range(n - 1, 1, -1)) + "(s0, s1)" + ")" * (n - 2) + ";"


def test_caterpillar_closed_form_is_make_cluster_tree():
    names = [f"s{i}" for i in range(6)]
    assert cluster.make_cluster_tree(names, caterpillar(6)) == caterpillar_newick(6)
    assert caterpillar_newick(6) == "(s5, (s4, (s3, (s2, (s0, s1)))));"


def test_caterpillar_5000_deeper_than_the_recursion_limit():
    n = 5000
    names = [f"s{i}" for i in range(n)]
    _, j = np.triu_indices(n, 1)  # condensed: D[i][j] = j + 1 for i < j
    z = linkage((j + 1).astype(np.float64), "average")
    assert cluster.linkage_to_newick(names, z) == caterpillar_newick(n)


def test_linkage_to_newick_rejects_bad_shapes():
    with pytest.raises(ValueError):
        cluster.linkage_to_newick(["a"], np.zeros((0, 4)))
    with pytest.raises(ValueError):
        cluster.linkage_to_newick(["a", "b", "c"], np.zeros((1, 4)))


def test_ctree_rejects_an_unknown_tree():
    seqs = {"a": np.zeros(30, np.uint8), "b": np.ones(30, np.uint8)}
    with pytest.raises(ValueError, match="Unexpected tree"):
        cluster.ctree(seqs, tree="upgma")
