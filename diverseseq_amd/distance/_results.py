"""What the operations over distances return and what they take, host side only: the result types, the limits of
include/dvs_hip.h, the argument checks (each before any device work, each returning its arguments as the C entry takes
them) and the buffers and conversions around a call.  numpy alone: no ctypes, no context."""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

# the public names of this layer, which the package re-exports
__all__ = [
    "CANONICAL_MASH", "LINKAGE_METHODS", "linkage_method_code", "tree_outputs", "linkage_matrix", "NJTree",
    "nj_outputs", "nj_tree_of", "nj_inputs", "N_NEAREST_MAX", "check_n_nearest", "ClusterScores", "check_labels",
    "CopheneticScores", "check_linkage_matrix", "MaxMin", "check_maxmin_args", "Neighbours", "ThresholdClusters",
    "check_radius", "check_max_pairs", "MIN_SAMPLES_MAX", "MST", "check_core", "check_min_samples", "PCOA_MAX_AXES",
    "PCoA", "check_pcoa_args", "check_pcoa_fit", "KMEDOIDS_MAX_K", "KMEDOIDS_MAX_SWAPS", "KMedoids",
    "check_kmedoids_args", "PERMANOVA_MAX_GROUPS", "PERMANOVA", "encode_grouping", "permuted_labels",
    "check_permanova_args", "permanova_statistics",
]

_U32_MAX = 0xFFFFFFFF

CANONICAL_MASH = "Canonical count rows should only be specified for the jsd and euclidean distances (mash: mash_canonical)."


def _row_list(rows, limit: int):
    """a side's row list as the C entries take it: (None, limit) for every row, else (uint32 array, its length);
    ValueError for an entry outside 0 .. limit - 1"""
    if rows is None:
        return None, int(limit)
    a = np.asarray(rows)
    if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
        raise ValueError("a row list is a one-dimensional sequence of integers")
    if a.size and (int(a.min()) < 0 or int(a.max()) >= limit):
        raise ValueError(f"row list entry outside 0 .. {limit - 1}")
    return np.ascontiguousarray(a, dtype=np.uint32), int(a.size)


def _dist_out(out, n: int) -> np.ndarray:
    """the n x n matrix a distance call writes into: `out` when it is given (and fits), else zeros"""
    if out is None:
        return np.zeros((n, n), dtype=np.float64)
    if (not isinstance(out, np.ndarray) or out.shape != (n, n) or out.dtype != np.float64
            or not out.flags["C_CONTIGUOUS"]):
        raise ValueError(f"out must be a C-contiguous float64 array of shape ({n}, {n})")
    return out


def _sketch_stride(offsets: np.ndarray, k: int, sketch_size: int) -> int:
    """words per sketch row: min(sketch_size, longest possible sketch of the batch), at least 1"""
    lens_in = np.diff(offsets.astype(np.int64))
    longest = int(max(0, (lens_in.max() if lens_in.size else 0) - k + 1))
    if sketch_size < 0 or sketch_size > _U32_MAX:
        raise OverflowError("sketch_size out of range for u32")  # pyo3 usize/u32 extraction
    return max(1, min(int(sketch_size), longest))


# ---- linkage trees

# scipy's _LINKAGE_METHODS codes of the methods the device builds (include/dvs_hip.h DVS_LINKAGE_*)
LINKAGE_METHODS = {"single": 0, "complete": 1, "average": 2, "weighted": 6, "ward": 5}


def linkage_method_code(method) -> int:
    """a linkage method's name -> its code; ValueError for centroid and median (scipy's fast_linkage, not built on
    the device) and for any other name"""
    if method in ("centroid", "median"):
        raise ValueError(f"{method!r} linkage is not built on the device (scipy builds it by fast_linkage); "
                         f"supported: {', '.join(LINKAGE_METHODS)}")
    if not isinstance(method, str) or method not in LINKAGE_METHODS:
        raise ValueError(f"Unexpected linkage method {method!r}: one of {', '.join(LINKAGE_METHODS)}")
    return LINKAGE_METHODS[method]


def tree_outputs(n: int):
    """host buffers of a dvs_linkage call for n leaves: pairs uint32 [2 (n - 1)], heights f64 [n - 1],
    sizes uint32 [n - 1]"""
    return (np.zeros(2 * (n - 1), dtype=np.uint32), np.zeros(n - 1, dtype=np.float64),
            np.zeros(n - 1, dtype=np.uint32))


def linkage_matrix(pairs: np.ndarray, heights: np.ndarray, sizes: np.ndarray) -> np.ndarray:
    """the outputs of a dvs_linkage call -> scipy's linkage matrix Z, float64 [n - 1, 4]"""
    z = np.empty((heights.size, 4), dtype=np.float64)
    z[:, 0] = pairs[0::2]
    z[:, 1] = pairs[1::2]
    z[:, 2] = heights
    z[:, 3] = sizes
    return z


# ---- neighbour-joining trees

class NJTree(NamedTuple):
    """A neighbour-joining tree of n leaves (include/dvs_hip.h "neighbour-joining tree"): unrooted, n - 2 records.
    children int64 [n - 2, 3]: record t joins these node ids (leaves 0 .. n - 1, record t makes node n + t); the third
    slot is -1 except in the last record, which joins the three nodes left.  lengths float64 [n - 2, 3]: the branch
    above each child, 0.0 in an unused slot; negative where the distances are not additive."""
    children: np.ndarray
    lengths: np.ndarray


def nj_outputs(n: int):
    """host buffers of a dvs_nj call for n leaves: joins uint32 [3 (n - 2)], lengths f64 [3 (n - 2)]"""
    return np.zeros(3 * (n - 2), dtype=np.uint32), np.zeros(3 * (n - 2), dtype=np.float64)


def nj_tree_of(joins: np.ndarray, lengths: np.ndarray) -> NJTree:
    """the outputs of a dvs_nj call -> NJTree"""
    children = joins.reshape(-1, 3).astype(np.int64)
    children[children == _U32_MAX] = -1
    return NJTree(children, lengths.reshape(-1, 3).copy())


def nj_inputs(tree) -> tuple[int, np.ndarray, np.ndarray]:
    """an NJTree (or any (children, lengths) pair) as dvs_nj_patristic takes it -> (n, joins uint32, lengths f64);
    ValueError unless both have shape (n - 2, 3) for n >= 3 leaves and the children are node ids or -1"""
    children, lengths = np.asarray(tree[0]), np.asarray(tree[1], dtype=np.float64)
    if children.ndim != 2 or children.shape[1] != 3 or children.shape[0] < 1 or children.dtype.kind not in "iu":
        raise ValueError(f"the children of a neighbour-joining tree of n >= 3 leaves have shape (n - 2, 3), not {children.shape}")
    if lengths.shape != children.shape:
        raise ValueError(f"the lengths of a neighbour-joining tree have its children's shape {children.shape}, not {lengths.shape}")
    n = children.shape[0] + 2
    c = children.astype(np.int64)
    if ((c < -1) | (c >= 2 * n - 2)).any():
        raise ValueError("the children of a neighbour-joining tree are node ids in 0 .. 2 n - 3, or -1 in an unused slot")
    c[c == -1] = _U32_MAX
    return n, np.ascontiguousarray(c, dtype=np.uint32).reshape(-1), np.ascontiguousarray(lengths).reshape(-1)


# ---- distances between two collections, and the nearest references of every query

N_NEAREST_MAX = 64  # include/dvs_hip.h: a caller who wants a full ranking takes the matrix


def check_n_nearest(n_nearest, n_refs: int) -> int:
    """n_nearest as dvs_nearest takes it, checked before any device work: ValueError unless it is an
    integer in 1 .. n_refs, NotImplementedError beyond N_NEAREST_MAX"""
    if isinstance(n_nearest, bool) or not isinstance(n_nearest, (int, np.integer)):
        raise ValueError(f"n_nearest must be an integer, not {n_nearest!r}")
    if n_nearest < 1 or n_nearest > n_refs:
        raise ValueError(f"n_nearest = {n_nearest}: between 1 and the number of references ({n_refs})")
    if n_nearest > N_NEAREST_MAX:
        raise NotImplementedError(f"n_nearest = {n_nearest}: {N_NEAREST_MAX} at most (a full ranking takes the matrix "
                                  "of cross_distances)")
    return int(n_nearest)


# ---- the scores of a labelling: sums within a cluster, the nearest other cluster, silhouettes, medoids

class ClusterScores(NamedTuple):
    """The scores of a labelling of n rows into K = labels.max() + 1 clusters (include/dvs_hip.h "flat clusters").
    Per row: labels int64; within float64, the sum of the distances to the other members of the row's cluster; a =
    within / (size - 1), 0 for a row alone in its cluster; b, the least mean distance to the members of another
    cluster, and neighbour int64, that cluster (a tie to the lower one, -1 and NaN where there is none); silhouette,
    0 for a row alone in its cluster or with a = b = 0, else (b - a) / max(a, b).  Per cluster: sizes int64; medoids
    int64, the member with the least within (a tie to the lowest row, -1 where there is none); cluster_silhouette,
    the mean silhouette of its members (NaN for an empty cluster).  mean_silhouette: the mean over all rows."""
    labels: np.ndarray
    within: np.ndarray
    a: np.ndarray
    b: np.ndarray
    neighbour: np.ndarray
    silhouette: np.ndarray
    sizes: np.ndarray
    medoids: np.ndarray
    cluster_silhouette: np.ndarray
    mean_silhouette: float


def check_labels(labels, n: int) -> np.ndarray:
    """a labelling of n rows as dvs_cluster_scores takes it (uint32 [n]), checked before any device work:
    ValueError unless it is a one-dimensional sequence of n integers in 0 .. 2^32 - 2"""
    a = np.asarray(labels)
    if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
        raise ValueError("labels: a one-dimensional sequence of integers")
    if a.size != n:
        raise ValueError(f"{a.size} labels for {n} rows")
    if a.size and (int(a.min()) < 0 or int(a.max()) >= _U32_MAX):
        raise ValueError("label out of range: a cluster label is an integer of 0 or more")
    return np.ascontiguousarray(a, dtype=np.uint32)


# ---- the cophenetic correlation of a tree with the distances it was built from

class CopheneticScores(NamedTuple):
    """How well a tree represents the distances D of its n leaves (include/dvs_hip.h "cophenetic distances").
    correlation: Pearson's r between D(i, j) and the cophenetic distance coph(i, j), the height at which i and j first
    join, over every pair i != j: scipy's cophenet(Z, Y)[0]; NaN when either has no variance (n = 2, a constant matrix).
    row_sums float64 [5, n]: per leaf i the sums over j != i of x, y, x x, y y and x y with x = D(i, j) - c_bar, y =
    coph(i, j) - c_bar, c_bar the mean cophenetic distance; the same bits on every run.  cophenetic: float64 [n, n],
    squareform(scipy's cophenet(Z)) bit for bit, when it was asked for (matrix=True: n^2 doubles come back from the
    device), else None."""
    correlation: float
    row_sums: np.ndarray
    cophenetic: np.ndarray | None


def check_linkage_matrix(Z, n: int | None = None):
    """a linkage matrix in scipy's layout as dvs_cophenet takes it, checked before any device work ->
    (pairs uint32 [2 (n - 1)], heights float64 [n - 1]); ValueError unless its shape is (n - 1, 4) for n >= 2 leaves (n:
    the number of rows it must describe, None: taken from Z) and its first two columns are cluster ids.  (Which ids may
    meet in which merge is the C entry's check.)"""
    z = np.asarray(Z, dtype=np.float64)
    if z.ndim != 2 or z.shape[1] != 4 or z.shape[0] < 1:
        raise ValueError(f"a linkage matrix of n >= 2 leaves has shape (n - 1, 4), not {z.shape}")
    if n is not None and z.shape[0] != n - 1:
        raise ValueError(f"a linkage matrix of {n} leaves has shape ({n - 1}, 4), not {z.shape}")
    leaves = z.shape[0] + 1
    kids = z[:, :2]
    if not (np.isfinite(kids).all() and (kids >= 0).all() and (kids < 2 * leaves - 1).all() and (kids == np.floor(kids)).all()):
        raise ValueError("a linkage matrix's first two columns are cluster ids in 0 .. 2 n - 2")
    return np.ascontiguousarray(kids, dtype=np.uint32).reshape(-1), np.ascontiguousarray(z[:, 2])


# ---- farthest-first (max-min) selection of representatives

class MaxMin(NamedTuple):
    """A farthest-first traversal of n items (include/dvs_hip.h "farthest-first selection").  picks int64 [m]: the rows
    in pick order, the seeds first; radius float64 [m]: a pick's distance to the nearest earlier pick when it was taken
    (NaN for a seed; non-increasing behind the seeds); owner int64 [n]: the position in `picks` of every item's nearest
    pick, a tie to the earlier pick, -1 for an item that is out (NaN distance to a pick) or at +inf from every pick;
    dist float64 [n]: the distance to that pick (0.0 for a pick, NaN where out); cover: the largest dist over the items
    that are neither picks nor out -- the covering radius of the picks -- 0.0 when there are none."""
    picks: np.ndarray
    radius: np.ndarray
    owner: np.ndarray
    dist: np.ndarray
    cover: float


def check_maxmin_args(n: int, n_select, seeds, min_distance):
    """the arguments of a farthest-first selection over n items as dvs_maxmin takes them, checked before
    any device work -> (n_select, seeds uint32, use_min_distance, min_distance).  n_select None: n.  ValueError unless
    at least one of n_select and min_distance is given, the seeds are one or more distinct rows, n_seeds <= n_select <=
    n and min_distance is not NaN."""
    if n_select is None and min_distance is None:
        raise ValueError("farthest-first selection takes n_select, min_distance or both")
    sd = np.asarray(list(seeds) if not isinstance(seeds, np.ndarray) else seeds)
    if sd.ndim != 1 or sd.size == 0 or sd.dtype.kind not in "iu":
        raise ValueError("seeds: one or more row indices")
    if int(sd.min()) < 0 or int(sd.max()) >= n:
        raise ValueError(f"seed outside 0 .. {n - 1}")
    if np.unique(sd).size != sd.size:
        raise ValueError("a row is a seed more than once")
    if n_select is None:
        n_select = n
    if isinstance(n_select, bool) or not isinstance(n_select, (int, np.integer)):
        raise ValueError(f"n_select must be an integer, not {n_select!r}")
    if n_select < sd.size or n_select > n:
        raise ValueError(f"n_select = {n_select}: between the number of seeds ({sd.size}) and the number of rows ({n})")
    md = 0.0
    if min_distance is not None:
        md = float(min_distance)
        if md != md:
            raise ValueError("min_distance cannot be NaN")
    return int(n_select), np.ascontiguousarray(sd, dtype=np.uint32), int(min_distance is not None), md


# ---- the neighbours within a radius, and the groups they make (threshold clusters)

class Neighbours(NamedTuple):
    """For each of M queries the references within a radius (include/dvs_hip.h "neighbours within a radius"), as a CSR
    list: row_start int64 [M + 1]; index int64, the positions in the reference list, ascending within a query; distance
    float64, the cells of the mode's matrix bit for bit.  Query i owns the slots row_start[i] .. row_start[i + 1] - 1:
    `of(i)`.  A cell equal to the radius is listed, a NaN cell never."""
    row_start: np.ndarray
    index: np.ndarray
    distance: np.ndarray

    def of(self, i: int):
        """(the positions, the distances) of query i"""
        lo, hi = int(self.row_start[i]), int(self.row_start[i + 1])
        return self.index[lo:hi], self.distance[lo:hi]


class ThresholdClusters(NamedTuple):
    """The connected components of "distance <= radius" over n rows (include/dvs_hip.h "threshold clusters"): the flat
    clusters of the single-linkage tree cut at that height.  labels int64 [n], numbered by first appearance in row
    order (row 0 is in cluster 0), as cluster.cut_tree numbers them; n_clusters; sizes int64 [n_clusters]."""
    labels: np.ndarray
    n_clusters: int
    sizes: np.ndarray


def check_radius(radius) -> float:
    """a radius as dvs_within and dvs_threshold_clusters take it, checked before any handle is touched:
    ValueError unless it is a real number that is not NaN (inclusive; negative: nothing lies within it; inf: all does)"""
    if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)):
        raise ValueError(f"radius must be a real number, not {radius!r}")
    r = float(radius)
    if r != r:
        raise ValueError("radius cannot be NaN")
    return r


def check_max_pairs(max_pairs) -> int:
    """max_pairs as dvs_within takes it (0: no limit): ValueError unless None or an integer of 1 or more"""
    if max_pairs is None:
        return 0
    if isinstance(max_pairs, bool) or not isinstance(max_pairs, (int, np.integer)) or max_pairs < 1 or max_pairs >= 1 << 64:
        raise ValueError(f"max_pairs must be None or an integer of 1 or more, not {max_pairs!r}")
    return int(max_pairs)


def _no_neighbours(m: int) -> Neighbours:
    return Neighbours(np.zeros(m + 1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float64))


# ---- the minimum spanning tree: single linkage without the matrix

MIN_SAMPLES_MAX = 64  # N_NEAREST_MAX: the core distances come from `DeviceSide.nearest`


class MST(NamedTuple):
    """The minimum spanning tree of the distances of n rows (include/dvs_hip.h "minimum spanning tree"): edges int64
    [n_edges, 2], edge e joining positions edges[e, 0] < edges[e, 1] at weights[e] (float64), in ascending (weight,
    lower position, higher position) -- the order under which the tree is unique; n; n_rounds, the passes over the
    distances that were made.  Where NaN distances disconnect the rows it is a spanning forest of n - n_edges trees:
    `connected` tells.  The sorted weights are the heights of the single-linkage tree: `cluster.mst_linkage`."""
    edges: np.ndarray
    weights: np.ndarray
    n: int
    n_rounds: int

    @property
    def connected(self) -> bool:
        return self.n > 0 and self.weights.size == self.n - 1


def check_core(core, n: int) -> np.ndarray | None:
    """a core vector as dvs_mst takes it (float64 [n], or None), checked before any device work: ValueError unless it
    has one finite, non-negative entry per row"""
    if core is None:
        return None
    c = np.ascontiguousarray(np.asarray(core, dtype=np.float64))
    if c.shape != (n,):
        raise ValueError(f"core must hold one distance per row ({n}), got shape {c.shape}")
    bad = ~(np.isfinite(c) & (c >= 0))
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError(f"core distance {c[i]} of position {i}: finite and not negative")
    return c


def check_min_samples(min_samples, n: int) -> int:
    """min_samples as `DeviceSide.mst` takes it: ValueError unless an integer in 1 .. min(MIN_SAMPLES_MAX, n)"""
    if isinstance(min_samples, bool) or not isinstance(min_samples, (int, np.integer)):
        raise ValueError(f"min_samples must be an integer, not {min_samples!r}")
    if min_samples < 1 or min_samples > MIN_SAMPLES_MAX:
        raise ValueError(f"min_samples = {min_samples}: between 1 and {MIN_SAMPLES_MAX}")
    if min_samples > n:
        raise ValueError(f"min_samples = {min_samples} of {n} rows: no row has that many cells")
    return int(min_samples)


# ---- principal coordinates (PCoA, classical MDS) and the projection of further rows

PCOA_MAX_AXES = 64  # include/dvs_hip.h: a full spectrum takes a dense solver


class PCoA(NamedTuple):
    """The principal coordinates of n rows (include/dvs_hip.h "principal coordinates"): the n_axes algebraically largest
    eigenpairs of Gower's double-centred matrix B = J (-1/2 D o D) J, in descending order.
    values float64 [n_axes]; vectors float64 [n, n_axes], unit columns orthogonal to 1, the component of largest
    magnitude positive; coordinates float64 [n, n_axes] = vectors * sqrt(values), a zero column where values <= 0 (a
    non-Euclidean matrix has such axes; they come last); proportion = values / trace; residuals float64 [n_axes], the
    true ||B v - lambda v||_2 of each returned pair; row_means float64 [n], the row means of the squared distances (what
    a projection needs beside values and vectors); trace, the total inertia (1 / 2n) sum d^2; converged: every residual
    <= tol * values[0]; basis, steps: the columns of the Krylov basis at the end and the passes over the matrix."""
    values: np.ndarray
    vectors: np.ndarray
    coordinates: np.ndarray
    proportion: np.ndarray
    residuals: np.ndarray
    row_means: np.ndarray
    trace: float
    converged: bool
    basis: int
    steps: int


def check_pcoa_args(n: int, n_axes, tol, max_basis) -> tuple[int, float, int]:
    """the arguments of a principal-coordinates run over n rows as dvs_pcoa takes them -> (n_axes, tol, max_basis with
    0 for None), checked before any device work: ValueError unless n >= 2, n_axes is an integer in 1 .. n - 1, tol a
    number >= 0 and max_basis None or an integer >= n_axes; NotImplementedError for n_axes > PCOA_MAX_AXES"""
    if n < 2:
        raise ValueError(f"need at least two rows for principal coordinates, not {n}")
    if isinstance(n_axes, bool) or not isinstance(n_axes, (int, np.integer)):
        raise ValueError(f"n_axes must be an integer, not {n_axes!r}")
    if n_axes < 1 or n_axes > n - 1:
        raise ValueError(f"n_axes = {n_axes}: between 1 and n - 1 = {n - 1}")
    if n_axes > PCOA_MAX_AXES:
        raise NotImplementedError(f"n_axes = {n_axes}: {PCOA_MAX_AXES} at most (a full spectrum takes a dense solver)")
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or not float(tol) >= 0.0:
        raise ValueError(f"tol must be a number >= 0, not {tol!r}")
    if max_basis is None:
        max_basis = 0
    elif isinstance(max_basis, bool) or not isinstance(max_basis, (int, np.integer)) or max_basis < n_axes:
        raise ValueError(f"max_basis must be None or an integer >= n_axes = {n_axes}, not {max_basis!r}")
    return int(n_axes), float(tol), int(max_basis)


def check_pcoa_fit(fit, n_fitted: int):
    """the tables of a fit as dvs_pcoa_project takes them -> (values [m], vectors [n_fitted, m], row_means [n_fitted]),
    contiguous float64; ValueError unless `fit` is a `PCoA` (or has its values, vectors and row_means) of n_fitted rows"""
    try:
        values = np.ascontiguousarray(fit.values, dtype=np.float64)
        vectors = np.ascontiguousarray(fit.vectors, dtype=np.float64)
        mu = np.ascontiguousarray(fit.row_means, dtype=np.float64)
    except AttributeError:
        raise ValueError("a projection takes the PCoA of the fitted rows") from None
    if values.ndim != 1 or values.size < 1 or vectors.shape != (mu.size, values.size):
        raise ValueError(f"a fit of shapes {values.shape}, {vectors.shape}, {mu.shape}: values [m], vectors [n, m], row_means [n]")
    if values.size > PCOA_MAX_AXES:
        raise NotImplementedError(f"{values.size} axes: {PCOA_MAX_AXES} at most")
    if mu.size != n_fitted or n_fitted == 0:
        raise ValueError(f"the fit holds {mu.size} rows, the references {n_fitted}: they must be the fitted rows")
    return values, vectors, mu


# ---- k-medoids (PAM): the representatives that minimise the total distance

KMEDOIDS_MAX_K = 1024        # include/dvs_hip.h: the accumulators of a candidate live in LDS
KMEDOIDS_MAX_SWAPS = 65_535


class KMedoids(NamedTuple):
    """A k-medoids clustering of n items (include/dvs_hip.h "k-medoids").  medoids int64 [k]: the representatives, slot
    order part of the result; labels int64 [n]: the slot of every item's nearest medoid, equal distances to the lowest
    slot, a medoid in its own; dist float64 [n]: the distance to that medoid (0.0 for a medoid); second float64 [n]:
    the least distance to a medoid of any other slot (+inf when k = 1); swaps int64 [m, 2]: the exchanges in order, (the
    row that came in, the slot it took); td float64 [m + 1]: the total distance after the initialisation and after
    every exchange, td[-1] the final one; stop: 1 when no exchange lowers td any more, 0 when max_swaps exchanges were
    made; passes: the reads of the whole matrix."""
    medoids: np.ndarray
    labels: np.ndarray
    dist: np.ndarray
    second: np.ndarray
    swaps: np.ndarray
    td: np.ndarray
    stop: int
    passes: int


def check_kmedoids_args(n: int, n_medoids, init, max_swaps):
    """the arguments of a k-medoids run over n items, checked before any device work -> (k, kind, rows, max_swaps):
    kind "build", "maxmin" or "given", rows the initial medoids as uint32 [k] for "given", else None.  ValueError unless
    n >= 1, n_medoids is an integer in 1 .. n, max_swaps an integer >= 0 and init is "build", "maxmin" or n_medoids
    distinct rows; NotImplementedError for n_medoids > KMEDOIDS_MAX_K or max_swaps > KMEDOIDS_MAX_SWAPS"""
    if n < 1:
        raise ValueError("need at least one row for k-medoids")
    if isinstance(n_medoids, bool) or not isinstance(n_medoids, (int, np.integer)):
        raise ValueError(f"n_medoids must be an integer, not {n_medoids!r}")
    if n_medoids < 1 or n_medoids > n:
        raise ValueError(f"n_medoids = {n_medoids}: between 1 and the number of rows ({n})")
    if n_medoids > KMEDOIDS_MAX_K:
        raise NotImplementedError(f"n_medoids = {n_medoids}: {KMEDOIDS_MAX_K} at most")
    if isinstance(max_swaps, bool) or not isinstance(max_swaps, (int, np.integer)) or max_swaps < 0:
        raise ValueError(f"max_swaps must be an integer >= 0, not {max_swaps!r}")
    if max_swaps > KMEDOIDS_MAX_SWAPS:
        raise NotImplementedError(f"max_swaps = {max_swaps}: {KMEDOIDS_MAX_SWAPS} at most")
    if isinstance(init, str):
        if init not in ("build", "maxmin"):
            raise ValueError(f"init must be 'build', 'maxmin' or the initial medoids, not {init!r}")
        return int(n_medoids), init, None, int(max_swaps)
    try:
        rows = np.asarray(list(init) if not isinstance(init, np.ndarray) else init)
    except TypeError:
        raise ValueError(f"init must be 'build', 'maxmin' or the initial medoids, not {init!r}") from None
    if rows.ndim != 1 or rows.size == 0 or rows.dtype.kind not in "iu":
        raise ValueError("init: the initial medoids as row indices")
    if rows.size != n_medoids:
        raise ValueError(f"init names {rows.size} initial medoids, n_medoids is {n_medoids}")
    if int(rows.min()) < 0 or int(rows.max()) >= n:
        raise ValueError(f"initial medoid outside 0 .. {n - 1}")
    if np.unique(rows).size != rows.size:
        raise ValueError("a row is an initial medoid more than once")
    return int(n_medoids), "given", np.ascontiguousarray(rows, dtype=np.uint32), int(max_swaps)


# ---- PERMANOVA: do the groups explain the distances?

PERMANOVA_MAX_GROUPS = 65_535  # include/dvs_hip.h: a label travels in 8 or 16 bits


class PERMANOVA(NamedTuple):
    """A permutational multivariate analysis of variance (Anderson 2001; include/dvs_hip.h "PERMANOVA") of n items in a
    groups.  f: the pseudo-F statistic (SS_A / (a - 1)) / (SS_W / (n - a)), inf where SS_W == 0 < SS_A, nan where
    SS_T == 0; p_value: (1 + the permutations whose SS_W is <= the observed one, i.e. whose F is >= the observed F) /
    (1 + permutations), nan for permutations = 0; r2: SS_A / SS_T; ss_total, ss_within, ss_among = ss_total -
    ss_within; group_ss float64 [a]: each group's own term of ss_within, in the order of the groups' first appearance
    in the grouping; group_sizes int64 [a]; perm_f float64 [permutations]: F under each permutation, in the order they
    were drawn; permutations."""
    f: float
    p_value: float
    r2: float
    ss_total: float
    ss_within: float
    ss_among: float
    group_ss: np.ndarray
    group_sizes: np.ndarray
    perm_f: np.ndarray
    permutations: int


def encode_grouping(grouping, n: int, what: str = "grouping") -> tuple:
    """any sequence of n hashables -> (uint32 [n] codes 0 .. a - 1 in the order of first appearance, the a distinct
    values in that order); ValueError unless it holds one value per row"""
    if isinstance(grouping, (str, bytes)) or not hasattr(grouping, "__len__") or not hasattr(grouping, "__iter__"):
        raise ValueError(f"{what}: a sequence with one value per row")
    if len(grouping) != n:
        raise ValueError(f"{len(grouping)} values of {what} for {n} rows")
    codes, names = {}, []
    out = np.zeros(n, dtype=np.uint32)
    for i, g in enumerate(grouping.tolist() if isinstance(grouping, np.ndarray) else grouping):
        try:
            c = codes.get(g)
        except TypeError:
            raise ValueError(f"{what}: value {g!r} of row {i} is not hashable") from None
        if c is None:
            c = codes[g] = len(names)
            names.append(g)
        out[i] = c
    return out, names


def permuted_labels(labels: np.ndarray, permutations: int, seed=None, strata: np.ndarray | None = None) -> np.ndarray:
    """the label vectors of a PERMANOVA run: uint32 [permutations, n].  THE RULE, which the tests restate: rng =
    numpy.random.default_rng(seed); for each row, in order, ONE perm = rng.permutation(n); without strata the row is
    labels[perm]; with strata (codes, one per item) the positions of every block, in ascending order, receive the
    labels of that block's positions taken in ascending order of perm -- labels move inside their block only."""
    n = labels.size
    rng = np.random.default_rng(seed)
    out = np.zeros((permutations, n), dtype=np.uint32)
    blocks = None if strata is None else [np.flatnonzero(strata == s) for s in range(int(strata.max()) + 1)]
    for p in range(permutations):
        perm = rng.permutation(n)
        if blocks is None:
            out[p] = labels[perm]
        else:
            for idx in blocks:
                out[p, idx] = labels[idx[np.argsort(perm[idx], kind="stable")]]
    return out


def check_permanova_args(n: int, grouping, permutations, seed, strata) -> tuple:
    """the arguments of a PERMANOVA over n items, checked before any device work -> (labels uint32 [n], n_groups,
    perm_labels uint32 [permutations, n]).  ValueError unless n >= 3, grouping (and strata, if given) holds one
    hashable per row, there are between 2 and n - 1 groups and permutations is an integer >= 0; NotImplementedError
    beyond PERMANOVA_MAX_GROUPS groups.  The permutations are drawn here: `permuted_labels`."""
    if n < 3:
        raise ValueError("need at least three rows for PERMANOVA")
    labels, names = encode_grouping(grouping, n)
    a = len(names)
    if a < 2 or a >= n:
        raise ValueError(f"{a} groups of {n} rows: between 2 and {n - 1} (a group of its own for every row leaves no "
                         "distance within a group)")
    if a > PERMANOVA_MAX_GROUPS:
        raise NotImplementedError(f"{a} groups: {PERMANOVA_MAX_GROUPS} at most")
    if isinstance(permutations, bool) or not isinstance(permutations, (int, np.integer)) or permutations < 0:
        raise ValueError(f"permutations must be an integer >= 0, not {permutations!r}")
    if permutations >= _U32_MAX:
        raise ValueError(f"permutations = {permutations}: fewer than 2^32 - 1")
    blocks = None if strata is None else encode_grouping(strata, n, "strata")[0]
    return labels, a, permuted_labels(labels, int(permutations), seed, blocks)


def permanova_statistics(n: int, n_groups: int, ss_total: float, ss_within: np.ndarray) -> tuple:
    """(SS_A, F, R^2) from SS_T and SS_W (a scalar or one per label vector) in float64, as `PERMANOVA` states them:
    SS_A = SS_T - SS_W; F = (SS_A / (a - 1)) / (SS_W / (n - a)), x / 0 = inf and 0 / 0 = nan as IEEE has them, nan
    wherever SS_T == 0; R^2 = SS_A / SS_T"""
    ssw = np.asarray(ss_within, dtype=np.float64)
    sst = np.float64(ss_total)
    with np.errstate(divide="ignore", invalid="ignore"):
        ssa = sst - ssw
        f = (ssa / np.float64(n_groups - 1)) / (ssw / np.float64(n - n_groups))
        f = np.where(sst == 0, np.nan, f)
        r2 = ssa / sst
    return ssa, f, r2
