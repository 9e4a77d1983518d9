"""The host half of the other linkage methods (no GPU): plain-Python restatements of scipy's nn_chain for complete,
weighted and ward linkage and of its mst_single_linkage, both followed by `label` -- the second oracle of
tests/test_gpu_linkage_methods.py -- against scipy itself, bit for bit; and the argument errors `cluster.linkage`
and `ctree` raise before any device work."""
import math

import numpy as np
import pytest
from scipy.cluster.hierarchy import linkage as scipy_linkage

from diverseseq_amd import cluster, distance

METHODS = ("single", "complete", "average", "weighted", "ward")


def scipy_z(d: np.ndarray, method: str) -> np.ndarray:
    d = np.asarray(d, dtype=np.float64)
    return scipy_linkage(d[np.triu_indices(d.shape[0], 1)], method)


def upper_mirrored(d) -> list:
    """the upper triangle of d copied over the lower one, as Python floats"""
    D = np.array(d, dtype=np.float64)
    D = np.triu(D, 1) + np.triu(D, 1).T
    return [[float(v) for v in row] for row in D]


def merged_distance(method: str, d_xi: float, d_yi: float, d_xy: float, nx: int, ny: int, ni: int) -> float:
    """scipy's _hierarchy_distance_update.pxi, same operands in the same order"""
    if method == "complete":
        return d_yi if d_yi > d_xi else d_xi  # Cython's max(d_xi, d_yi)
    if method == "average":
        return (nx * d_xi + ny * d_yi) / (nx + ny)
    if method == "weighted":
        return 0.5 * (d_xi + d_yi)
    assert method == "ward"
    t = 1.0 / (nx + ny + ni)
    return math.sqrt((ni + nx) * t * d_xi * d_xi + (ni + ny) * t * d_yi * d_yi - ni * t * d_xy * d_xy)


def label(n: int, rec) -> np.ndarray:
    """scipy's stable sort of the records (x, y, height) by height and its union-find relabelling"""
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


def nn_chain(d, method: str) -> np.ndarray:
    """scipy's _hierarchy.nn_chain and `label`, restated over the upper triangle of d"""
    n = len(d)
    D = upper_mirrored(d)
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
        x, y = min(x, y), max(x, y)
        nx, ny = size[x], size[y]
        rec.append((x, y, cur))
        size[x], size[y] = 0, nx + ny
        for i in range(n):
            if size[i] > 0 and i != y:
                D[i][y] = D[y][i] = merged_distance(method, D[i][x], D[i][y], cur, nx, ny, size[i])
    return label(n, rec)


def mst_single(d) -> np.ndarray:
    """scipy's _hierarchy.mst_single_linkage and `label`, restated over the upper triangle of d"""
    n = len(d)
    D = upper_mirrored(d)
    merged = [False] * n
    dm = [float("inf")] * n
    rec = []
    x = y = 0
    for _ in range(n - 1):
        cur = float("inf")
        merged[x] = True
        for i in range(n):
            if merged[i]:
                continue
            if dm[i] > D[x][i]:
                dm[i] = D[x][i]
            if dm[i] < cur:  # strict <, ascending: the lowest index wins ties
                cur, y = dm[i], i
        rec.append((x, y, cur))
        x = y
    return label(n, rec)


def restated(d, method: str) -> np.ndarray:
    return mst_single(d) if method == "single" else nn_chain(d, method)


def method_matrices(seed: int, negative: bool = True):
    """(label, matrix): random, integers 0..3 (heavy ties), constant, 2 decimals, multiples of 0.1, negative"""
    rng = np.random.default_rng(seed)
    for n in (2, 3, 5, 9, 17, 33, 60):
        u = rng.random((n, n))
        yield f"uniform{n}", u
        yield f"int{n}", rng.integers(0, 4, (n, n)).astype(np.float64)
        yield f"rounded{n}", np.round(u, 2)
        yield f"tenths{n}", rng.integers(0, 8, (n, n)) * 0.1
        if negative:
            yield f"negative{n}", u - 0.5
    yield "constant", np.full((25, 25), 0.75)
    yield "zero", np.zeros((12, 12))


@pytest.mark.parametrize("method", METHODS)
def test_restatement_matches_scipy(method):
    """the second oracle is scipy's Z bit for bit, ties included; ward on non-negative matrices only"""
    count = 0
    for seed in (0, 1):
        for name, d in method_matrices(seed, negative=method != "ward"):
            assert np.array_equal(restated(d, method), scipy_z(d, method)), (method, seed, name)
            count += 1
    assert count == (74 if method != "ward" else 60)


def test_single_linkage_ties_take_the_lowest_index():
    """mst_single_linkage's records before relabelling: from 0 along equal distances in ascending index order"""
    d = np.ones((5, 5))
    assert mst_single(d).tolist() == scipy_z(d, "single").tolist() == [
        [0, 1, 1, 2], [2, 5, 1, 3], [3, 6, 1, 4], [4, 7, 1, 5]]


@pytest.mark.parametrize("bad", ["centroid", "median"])
def test_fast_linkage_methods_are_refused_without_a_gpu(bad):
    with pytest.raises(ValueError, match="not built on the device"):
        cluster.linkage(np.ones((4, 4)), bad)
    with pytest.raises(ValueError, match="not built on the device"):
        cluster.ctree({"a": np.zeros(30, np.uint8), "b": np.ones(30, np.uint8)}, linkage=bad)


@pytest.mark.parametrize("bad", ["upgma", "Average", "", None, 2])
def test_unknown_methods_list_the_supported_ones(bad):
    with pytest.raises(ValueError, match="single, complete, average, weighted, ward"):
        cluster.linkage(np.ones((4, 4)), bad)
    with pytest.raises(ValueError, match="single, complete, average, weighted, ward"):
        distance.linkage_method_code(bad)


@pytest.mark.parametrize("method", METHODS)
def test_shape_errors_without_a_gpu(method):
    for d in (np.zeros((3, 4)), np.zeros(5), np.zeros((2, 2, 2)), np.zeros((1, 1)), np.zeros((0, 0)), [[0.0]]):
        with pytest.raises(ValueError):
            cluster.linkage(d, method)


def test_the_sklearn_tree_is_average_only():
    seqs = {"a": np.zeros(30, np.uint8), "b": np.ones(30, np.uint8)}
    for method in ("single", "complete", "weighted", "ward"):
        with pytest.raises(ValueError, match="average linkage only"):
            cluster.ctree(seqs, tree="sklearn", linkage=method)
