"""The minimum spanning tree's cases and yardsticks (tests/test_mst_host.py pins the yardsticks on the CPU,
tests/test_gpu_mst.py holds the device to them).  numpy only.

Edges are ordered by (weight, lower position, higher position); under that order the minimum spanning tree is unique,
so every comparison is "equal as arrays": `kruskal` is the definition, `boruvka` restates the device's algorithm round
by round (and counts the rounds), `linkage_from_mst` restates dvs_linkage_from_mst."""
import functools

import numpy as np

# the bounds of csrc/mst.hip, each with a size on either side of it among SIZES
MST_WAVE_ROW = 1024   # rows of up to that many cells take a wave each, longer rows a workgroup each
MST_THREADS = 256     # a workgroup's threads, its stride along a long row: 1 025 and 2 049 = k x 256 + 1 give one thread a step more
WAVE = 64             # a wave's lanes: a row with fewer cells leaves lanes without one
SIZES = (2, 3, 64, 65, 257, 1024, 1025, 2049)
STRIPS = (1, 7, 64)   # strip heights (DVS_CROSS_STRIP_ROWS) beside the default


def kruskal(W):
    """the minimum spanning forest of the symmetric weights W (NaN: no edge) by Kruskal's algorithm over the upper
    triangle in ascending (w, i, j) -> (edges int64 [m, 2] with i < j, weights float64 [m]), in that order"""
    W = np.asarray(W, dtype=np.float64)
    n = W.shape[0]
    iu, ju = np.triu_indices(n, 1)
    w = W[iu, ju]
    keep = ~np.isnan(w)
    iu, ju, w = iu[keep], ju[keep], w[keep]
    order = np.lexsort((ju, iu, w))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    edges, weights = [], []
    for e in order.tolist():
        a, b = find(int(iu[e])), find(int(ju[e]))
        if a != b:
            parent[max(a, b)] = min(a, b)
            edges.append((int(iu[e]), int(ju[e])))
            weights.append(w[e])
            if len(edges) == n - 1:
                break
    return np.array(edges, dtype=np.int64).reshape(-1, 2), np.array(weights, dtype=np.float64)


def reachability(D, core=None):
    """max(D[i, j], core[i], core[j]): the weights the device takes with a core vector"""
    D = np.asarray(D, dtype=np.float64)
    if core is None:
        return D
    c = np.asarray(core, dtype=np.float64)
    W = np.maximum(np.maximum(D, c[:, None]), c[None, :])
    W[np.isnan(D)] = np.nan
    return W


def boruvka(D, core=None):
    """the device's algorithm restated: labels the identity; a round gives every row its least (w, j) over the columns
    of another label whose cell is not NaN (a tie to the lower j), every label the least (w, lo, hi) of its rows, and
    applies the sorted picks through a union-find that drops a pick whose ends already share a root; every row is
    relabelled with the lowest position of its component.  It ends with one component or a round without a pick, which
    counts.  -> (edges, weights, rounds), the edges sorted by (w, lo, hi)"""
    W = reachability(D, core)
    n = W.shape[0]
    labels = np.arange(n)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    tree, rounds, components = [], 0, n
    while components > 1:
        rounds += 1
        masked = np.where(np.isnan(W) | (labels[:, None] == labels[None, :]), np.inf, W)  # (the cases hold no inf)
        j = masked.argmin(axis=1)  # (the first least: the lower column)
        w = masked[np.arange(n), j]
        best = {}
        for i in np.flatnonzero(np.isfinite(w)).tolist():
            pick = (w[i], min(i, int(j[i])), max(i, int(j[i])))
            if labels[i] not in best or pick < best[labels[i]]:
                best[labels[i]] = pick
        if not best:
            break
        for pick in sorted(best.values()):
            a, b = find(pick[1]), find(pick[2])
            if a != b:
                parent[max(a, b)] = min(a, b)
                tree.append(pick)
                components -= 1
        labels = np.array([find(i) for i in range(n)])
    tree.sort()
    return (np.array([(lo, hi) for _, lo, hi in tree], dtype=np.int64).reshape(-1, 2),
            np.array([w for w, _, _ in tree], dtype=np.float64), rounds)


def linkage_from_mst(n, edges, weights):
    """dvs_linkage_from_mst restated: the sorted edges of a spanning tree -> scipy's Z of the single-linkage tree"""
    root = list(range(n))
    ident = list(range(n))
    size = [1] * n

    def find(x):
        while root[x] != x:
            root[x] = root[root[x]]
            x = root[x]
        return x

    Z = np.zeros((n - 1, 4))
    for e, ((x, y), w) in enumerate(zip(np.asarray(edges).tolist(), np.asarray(weights).tolist())):
        a, b = find(x), find(y)
        assert a != b
        Z[e] = min(ident[a], ident[b]), max(ident[a], ident[b]), w, size[a] + size[b]
        root[b] = a
        size[a] += size[b]
        ident[a] = n + e
    return Z


def partition(labels) -> np.ndarray:
    """a labelling numbered by first appearance in row order"""
    first = {}
    return np.array([first.setdefault(int(x), len(first)) for x in labels], dtype=np.int64)


def cut_heights(weights):
    """the heights a tree is cut at: a few of its merge heights, one ulp below each, and between two of them"""
    u = np.unique(np.asarray(weights, dtype=np.float64))
    picks = u[np.unique(np.linspace(0, u.size - 1, 4).astype(int))]
    between = [(u[i] + u[i + 1]) / 2 for i in (0, u.size // 2 - 1) if 0 <= i < u.size - 1]
    return sorted({float(h) for h in picks} | {float(np.nextafter(h, -np.inf)) for h in picks} | {float(h) for h in between})


# ------------------------------------------------------------------ the families of matrices (seeded, read-only)

def _frozen(d):
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def euclid_points(n: int) -> np.ndarray:
    """(a) the distances of n random points in the plane: no two equal off the diagonal"""
    p = np.random.default_rng(n).random((n, 2))
    d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))
    iu = np.triu_indices(n, 1)
    assert np.unique(d[iu]).size == iu[0].size and np.array_equal(d, d.T)
    return _frozen(d)


@functools.lru_cache(maxsize=None)
def hamming10(n: int) -> np.ndarray:
    """(b) the Hamming distances of n 10-bit strings with duplicates: integers 0 .. 10, heavy ties, zeros"""
    codes = np.random.default_rng(n + 1).integers(0, 1 << 10, n)
    if n > 2:
        codes[n // 2] = codes[0]
    x = codes[:, None] ^ codes[None, :]
    d = np.zeros((n, n))
    for b in range(10):
        d += (x >> b) & 1
    return _frozen(d)


@functools.lru_cache(maxsize=None)
def ruler(n: int) -> np.ndarray:
    """(c) points on a line, the gap in front of point i bit_length(i & -i): the most rounds a Boruvka takes"""
    gaps = np.array([0] + [int(i & -i).bit_length() for i in range(1, n)], dtype=np.float64)
    x = np.cumsum(gaps)
    return _frozen(np.abs(x[:, None] - x[None, :]))


@functools.lru_cache(maxsize=None)
def nan_row(n: int) -> np.ndarray:
    """(d) tie-free distances with row and column n // 3 NaN: that position is a tree of its own"""
    d = euclid_points(n).copy()
    d[n // 3, :] = d[:, n // 3] = np.nan
    return _frozen(d)


@functools.lru_cache(maxsize=None)
def nan_blocks(n: int) -> np.ndarray:
    """(d) Hamming distances with every cell between the first n // 2 positions and the rest NaN: two trees"""
    d = hamming10(n).copy()
    h = n // 2
    d[:h, h:] = d[h:, :h] = np.nan
    return _frozen(d)


@functools.lru_cache(maxsize=None)
def core_of(n: int) -> np.ndarray:
    """(e) a core vector given by the caller: a quarter of the largest distance at most, so that most weights tie"""
    return _frozen(np.random.default_rng(n + 2).random(n) * euclid_points(n).max() / 4)


def kth_smallest(D, m: int) -> np.ndarray:
    """the m-th smallest cell of every row, the row's own cell included"""
    return np.sort(np.asarray(D), axis=1)[:, m - 1]


FAMILIES = {"euclid": euclid_points, "hamming": hamming10, "ruler": ruler, "nan_row": nan_row, "nan_blocks": nan_blocks}
RULER_ROUNDS = {257: 8, 1025: 10}


def matrix_cases():
    """(family, n) of every GIVEN case: every size for the two dense families, the sizes the round count is known at
    for the ruler, and sizes on both sides of the kernel's bound for the forests"""
    cases = [(f, n) for f in ("euclid", "hamming") for n in SIZES]
    cases += [("ruler", n) for n in (65, 257, 1025)]
    cases += [(f, n) for f in ("nan_row", "nan_blocks") for n in (3, 65, 1024, 1025)]
    return cases


@functools.lru_cache(maxsize=None)
def expected(family: str, n: int, core: str = "none"):
    """the yardstick of a GIVEN case, computed once: (edges, weights, rounds) of `boruvka`; core: "none", "given"
    (`core_of`) or "m<k>" (the k-th smallest cell)"""
    D = FAMILIES[family](n)
    c = None if core == "none" else core_of(n) if core == "given" else kth_smallest(D, int(core[1:]))
    e, w, r = boruvka(D, c)
    for a in (e, w):
        a.setflags(write=False)
    return e, w, r
