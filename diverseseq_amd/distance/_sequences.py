"""The public functions over sequences and over count matrices already in HBM: per operation the functions of each mode
(mash_*, euclidean_*, jsd_*) with the table that names them, the general function that takes `distance_mode`, and the
matrix_* function over an engine.CountMatrix.  Each checks its arguments, makes a `DeviceSide` and calls its method."""

from __future__ import annotations

import numpy as np

from .. import engine
from ._calls import (_NO_ROWS, distances_from_sketches, run_cluster_scores, run_mst, run_permanova, run_threshold_clusters,
                     sketch_batch)
from ._results import (CANONICAL_MASH, ClusterScores, CopheneticScores, KMedoids, MaxMin, MST, Neighbours, NJTree, PCoA,
                       PERMANOVA, ThresholdClusters, _no_neighbours, check_core, check_kmedoids_args, check_labels,
                       check_linkage_matrix, check_max_pairs, check_maxmin_args, check_min_samples, check_n_nearest,
                       check_pcoa_args, check_pcoa_fit, check_permanova_args, check_radius, linkage_method_code)
from ._sides import DeviceSide, device_side

# the public names of this layer, which the package re-exports
__all__ = [
    "mash_sketches", "mash_distance", "mode_args", "check_mode_args", "mash_distances", "euclidean_distances",
    "matrix_euclidean_distances", "jsd_distances", "matrix_jsd_distances", "mash_linkage", "euclidean_linkage",
    "jsd_linkage", "MODES", "mash_nj", "euclidean_nj", "jsd_nj", "NJ_MODES", "matrix_cross_distances",
    "matrix_nearest", "mash_cross_distances", "mash_nearest", "euclidean_cross_distances", "euclidean_nearest",
    "jsd_cross_distances", "jsd_nearest", "CROSS_MODES", "cross_distances", "nearest", "matrix_cluster_scores",
    "cluster_scores", "matrix_cophenet", "cophenet", "matrix_maxmin", "mash_maxmin", "euclidean_maxmin",
    "jsd_maxmin", "MAXMIN_MODES", "maxmin", "matrix_within", "matrix_threshold_clusters", "within", "neighbours",
    "threshold_clusters", "matrix_mst", "mash_mst", "euclidean_mst", "jsd_mst", "MST_MODES", "mst", "matrix_pcoa",
    "matrix_pcoa_project", "mash_pcoa", "euclidean_pcoa", "jsd_pcoa", "PCOA_MODES", "pcoa", "pcoa_project",
    "matrix_kmedoids", "mash_kmedoids", "euclidean_kmedoids", "jsd_kmedoids", "KMEDOIDS_MODES", "kmedoids",
    "matrix_permanova", "mash_permanova", "euclidean_permanova", "jsd_permanova", "PERMANOVA_MODES", "permanova",
]


def mash_sketches(seqs, k: int, sketch_size: int, num_states: int = 4,
                  mash_canonical: bool = False) -> list[list[int]]:
    sk, lens = sketch_batch(seqs, k, sketch_size, num_states, mash_canonical)
    return [sk[i, : int(lens[i])].tolist() for i in range(len(seqs))]


def mash_distance(left_sketch, right_sketch, k: int, sketch_size: int) -> float:
    """diverse_seq/distance.py:230-291 for one pair"""
    l = np.asarray(left_sketch, dtype=np.uint32)
    r = np.asarray(right_sketch, dtype=np.uint32)
    stride = max(1, l.size, r.size)
    sk = np.zeros((2, stride), dtype=np.uint32)
    sk[1, : l.size] = l  # pair (i=1, j=0): left is row i
    sk[0, : r.size] = r
    d = distances_from_sketches(sk, np.array([r.size, l.size], dtype=np.uint32), k, sketch_size)
    return float(d[1, 0])


def _count_side(m: "engine.CountMatrix", mode: str) -> DeviceSide:
    """a count matrix of the caller's as a `DeviceSide` that does not own it"""
    if mode not in ("jsd", "euclidean"):
        raise ValueError(f"Unexpected distance {mode!r} between the rows of count matrices: 'jsd' or 'euclidean'.")
    return DeviceSide(m, mode)


def mode_args(distance_mode: str, k: int, sketch_size, num_states: int, mash_canonical: bool) -> tuple:
    """what either function of MODES[distance_mode] takes behind the sequences"""
    if distance_mode == "mash":
        return k, int(sketch_size), num_states, mash_canonical
    return k, num_states


def check_mode_args(distance_mode: str, sketch_size, mash_canonical: bool, canonical: bool = False) -> None:
    """the argument checks of cluster.ctree for a distance mode, with its messages; canonical: the count rows of the jsd
    and euclidean modes folded onto the canonical k-mer bins (`device_side`)"""
    if distance_mode not in DeviceSide.MODE_NAMES:
        raise ValueError(f"Unexpected distance {distance_mode!r}.")
    if distance_mode == "mash" and sketch_size is None:
        raise ValueError("Expected sketch size for mash distance measure.")
    if distance_mode != "mash" and sketch_size is not None:
        raise ValueError("Sketch size should only be specified for the mash distance.")
    if distance_mode != "mash" and mash_canonical:
        raise ValueError("Canonical kmers should only be specified for the mash distance.")
    if distance_mode == "mash" and canonical:
        raise ValueError(CANONICAL_MASH)


# ---- the N x N distances and the linkage tree

def mash_distances(seqs, k: int, sketch_size: int, num_states: int = 4,
                   mash_canonical: bool = False, ctx: engine.Context | None = None) -> np.ndarray:
    """diverse_seq/distance.py:119-175: sketches, then the symmetric N x N matrix; the sketches stay in
    HBM between the two stages"""
    with device_side(seqs, "mash", k, sketch_size, num_states, mash_canonical, ctx=ctx) as dev:
        return dev.distances()


def euclidean_distances(seqs, k: int, num_states: int = 4,
                        ctx: engine.Context | None = None, canonical: bool = False) -> np.ndarray:
    """diverse_seq/distance.py:294-332: ||kfreqs_i - kfreqs_j||_2; canonical (here and in every jsd / euclidean function
    over sequences below): over count rows folded onto the canonical k-mer bins, as `device_side` takes it"""
    with device_side(seqs, "euclidean", k, num_states, ctx=ctx, canonical=canonical) as dev:
        return dev.distances()


def matrix_euclidean_distances(m: "engine.CountMatrix") -> np.ndarray:
    """`euclidean_distances` over the rows of a matrix already in HBM (count rows of either width, or the frequency
    rows of Context.matrix_from_freqs)"""
    return DeviceSide(m, "euclidean").distances()


def jsd_distances(seqs, k: int, num_states: int = 4, ctx: engine.Context | None = None,
                  canonical: bool = False) -> np.ndarray:
    """the Jensen-Shannon divergence (bits, not its square root) of the k-mer frequencies of every pair,
    H((f_i + f_j) / 2) - (H(f_i) + H(f_j)) / 2: total_jsd of the two-member set (src/records.rs:27-68; paper Table 1).
    float64 [n, n], symmetric, in [0, 1], exactly 0 on the diagonal and between sequences of equal counts; NaN off
    the diagonal for a sequence without a valid k-mer"""
    with device_side(seqs, "jsd", k, num_states, ctx=ctx, canonical=canonical) as dev:
        return dev.distances()


def matrix_jsd_distances(m: "engine.CountMatrix") -> np.ndarray:
    """`jsd_distances` over the rows of a matrix already in HBM (count rows of either width, or the frequency rows
    of Context.matrix_from_freqs)"""
    return DeviceSide(m, "jsd").distances()


def mash_linkage(seqs, k: int, sketch_size: int, num_states: int = 4, mash_canonical: bool = False, *,
                 method: str = "average", ctx: engine.Context | None = None) -> np.ndarray:
    """`dvs ctree`'s mash tree on the device for any of LINKAGE_METHODS: sketches, the N x N distances and scipy's
    linkage matrix Z of `method`, every stage in HBM; only Z (n - 1 rows) comes back"""
    linkage_method_code(method)
    with device_side(seqs, "mash", k, sketch_size, num_states, mash_canonical, ctx=ctx) as dev:
        return dev.linkage(method)


def euclidean_linkage(seqs, k: int, num_states: int = 4, *, method: str = "average",
                      ctx: engine.Context | None = None, canonical: bool = False) -> np.ndarray:
    """the same for the euclidean distances (a sequence without valid k-mers: NaN distances, ValueError)"""
    linkage_method_code(method)
    with device_side(seqs, "euclidean", k, num_states, ctx=ctx, canonical=canonical) as dev:
        return dev.linkage(method)


def jsd_linkage(seqs, k: int, num_states: int = 4, *, method: str = "average",
                ctx: engine.Context | None = None, canonical: bool = False) -> np.ndarray:
    """the same for the Jensen-Shannon divergences of `jsd_distances`, the same matrix bit for bit (a sequence
    without valid k-mers: NaN distances, ValueError)"""
    linkage_method_code(method)
    with device_side(seqs, "jsd", k, num_states, ctx=ctx, canonical=canonical) as dev:
        return dev.linkage(method)


# a ctree distance mode -> (its N x N distances, its tree): both take (seqs, *mode_args(...)), the tree also method=
MODES = {"mash": (mash_distances, mash_linkage), "euclidean": (euclidean_distances, euclidean_linkage),
         "jsd": (jsd_distances, jsd_linkage)}


# ---- neighbour-joining trees

def mash_nj(seqs, k: int, sketch_size: int, num_states: int = 4, mash_canonical: bool = False, *,
            ctx: engine.Context | None = None) -> NJTree:
    """the neighbour-joining tree of the mash distances on the device: sketches, the N x N distances and the tree,
    every stage in HBM; only the n - 2 records come back.  ZeroDivisionError as `mash_distances`."""
    return _nj(seqs, "mash", k, sketch_size, num_states, mash_canonical, ctx=ctx)


def euclidean_nj(seqs, k: int, num_states: int = 4, *, ctx: engine.Context | None = None,
                 canonical: bool = False) -> NJTree:
    """the same for the euclidean distances (a sequence without valid k-mers: NaN distances, ValueError)"""
    return _nj(seqs, "euclidean", k, num_states, ctx=ctx, canonical=canonical)


def jsd_nj(seqs, k: int, num_states: int = 4, *, ctx: engine.Context | None = None, canonical: bool = False) -> NJTree:
    """the same for the Jensen-Shannon divergences of `jsd_distances` (a sequence without valid k-mers: ValueError)"""
    return _nj(seqs, "jsd", k, num_states, ctx=ctx, canonical=canonical)


def _nj(seqs, distance_mode: str, *args, ctx, canonical: bool = False) -> NJTree:
    if len(seqs) < 3:
        raise ValueError("need at least three sequences for a neighbour-joining tree")
    with device_side(seqs, distance_mode, *args, ctx=ctx, canonical=canonical) as dev:
        return dev.nj()


# a ctree distance mode -> its neighbour-joining tree: takes (seqs, *mode_args(...)), and ctx=
NJ_MODES = {"mash": mash_nj, "euclidean": euclidean_nj, "jsd": jsd_nj}


# ---- distances between two collections, and the nearest references of every query

def matrix_cross_distances(q: "engine.CountMatrix", r: "engine.CountMatrix", mode: str = "jsd", q_rows=None,
                           r_rows=None) -> np.ndarray:
    """the `mode` ("jsd", "euclidean") distances of rows q_rows of q (None: all) against rows r_rows of r: float64
    [M, N], every cell the bits the square function of the mode gives the same two rows.  q and r may be one matrix
    (rows against selected rows of the same matrix copy nothing) and may differ in element type, not in nbins."""
    return _count_side(q, mode).cross_distances(_count_side(r, mode), q_rows, r_rows)


def matrix_nearest(q: "engine.CountMatrix", r: "engine.CountMatrix", n_nearest: int = 1, mode: str = "jsd", q_rows=None,
                   r_rows=None):
    """the n_nearest rows of r (positions into r_rows, or rows) nearest to each row of q by `mode`, nearest first, a
    tie to the lower position: (int64 [M, n_nearest], -1 in a slot without a reference -- NaN cells are never
    listed; float64 distances, NaN there)"""
    return _count_side(q, mode).nearest(_count_side(r, mode), n_nearest, q_rows, r_rows)


def _two_sides(queries, refs, distance_mode: str, args, ctx, run, canonical: bool = False):
    """run(the queries' side, the references' side), both made for the call; the first is closed also where making
    the second fails"""
    with device_side(queries, distance_mode, *args, ctx=ctx, canonical=canonical) as q, \
            device_side(refs, distance_mode, *args, ctx=ctx, canonical=canonical) as r:
        return run(q, r)


def mash_cross_distances(queries, refs, k: int, sketch_size: int, num_states: int = 4, mash_canonical: bool = False,
                         ctx: engine.Context | None = None) -> np.ndarray:
    return _two_sides(queries, refs, "mash", (k, sketch_size, num_states, mash_canonical), ctx, DeviceSide.cross_distances)


def mash_nearest(queries, refs, n_nearest: int, k: int, sketch_size: int, num_states: int = 4,
                 mash_canonical: bool = False, ctx: engine.Context | None = None):
    return _two_sides(queries, refs, "mash", (k, sketch_size, num_states, mash_canonical), ctx,
                      lambda q, r: q.nearest(r, n_nearest))


def euclidean_cross_distances(queries, refs, k: int, num_states: int = 4, ctx: engine.Context | None = None,
                              canonical: bool = False) -> np.ndarray:
    return _two_sides(queries, refs, "euclidean", (k, num_states), ctx, DeviceSide.cross_distances, canonical)


def euclidean_nearest(queries, refs, n_nearest: int, k: int, num_states: int = 4, ctx: engine.Context | None = None,
                      canonical: bool = False):
    return _two_sides(queries, refs, "euclidean", (k, num_states), ctx, lambda q, r: q.nearest(r, n_nearest), canonical)


def jsd_cross_distances(queries, refs, k: int, num_states: int = 4, ctx: engine.Context | None = None,
                        canonical: bool = False) -> np.ndarray:
    return _two_sides(queries, refs, "jsd", (k, num_states), ctx, DeviceSide.cross_distances, canonical)


def jsd_nearest(queries, refs, n_nearest: int, k: int, num_states: int = 4, ctx: engine.Context | None = None,
                canonical: bool = False):
    return _two_sides(queries, refs, "jsd", (k, num_states), ctx, lambda q, r: q.nearest(r, n_nearest), canonical)


# a distance mode -> (its M x N distances, its nearest references): the first takes (queries, refs, *mode_args(...)),
# the second (queries, refs, n_nearest, *mode_args(...)); both ctx=
CROSS_MODES = {"mash": (mash_cross_distances, mash_nearest), "euclidean": (euclidean_cross_distances, euclidean_nearest),
               "jsd": (jsd_cross_distances, jsd_nearest)}


def cross_distances(queries, refs, distance_mode: str = "mash", *, k: int, sketch_size: int | None = None,
                    num_states: int = 4, mash_canonical: bool = False, ctx: engine.Context | None = None,
                    canonical: bool = False) -> np.ndarray:
    """the `distance_mode` distance of every query sequence to every reference sequence: float64 [M, N], cell (i, j) the
    bits MODES[distance_mode] gives the pair (queries[i], refs[j]) inside one collection.  Only the M x N pairs are
    computed.  Argument checks as cluster.ctree; ZeroDivisionError (mash) when a query and a reference both have an empty
    sketch; NaN (jsd, euclidean) for a sequence without a valid k-mer."""
    check_mode_args(distance_mode, sketch_size, mash_canonical, canonical)
    queries, refs = list(queries), list(refs)
    if not queries or not refs:
        return np.zeros((len(queries), len(refs)), dtype=np.float64)
    return _two_sides(queries, refs, distance_mode, mode_args(distance_mode, k, sketch_size, num_states, mash_canonical),
                      ctx, DeviceSide.cross_distances, canonical)


def nearest(queries, refs, n_nearest: int = 1, distance_mode: str = "mash", *, k: int, sketch_size: int | None = None,
            num_states: int = 4, mash_canonical: bool = False, ctx: engine.Context | None = None, canonical: bool = False):
    """the n_nearest references of every query by `distance_mode`, nearest first, a tie to the reference that comes first in
    `refs`: (idx int64 [M, n_nearest], positions in `refs`, -1 in a slot without one; dist float64 [M, n_nearest], NaN
    there).  A reference at NaN distance is never listed.  1 <= n_nearest <= min(len(refs), N_NEAREST_MAX), checked -- like
    the arguments cluster.ctree checks -- before any device work."""
    check_mode_args(distance_mode, sketch_size, mash_canonical, canonical)
    queries, refs = list(queries), list(refs)
    kk = check_n_nearest(n_nearest, len(refs))
    if not queries:
        return np.zeros((0, kk), dtype=np.int64), np.zeros((0, kk), dtype=np.float64)
    return _two_sides(queries, refs, distance_mode, mode_args(distance_mode, k, sketch_size, num_states, mash_canonical),
                      ctx, lambda q, r: q.nearest(r, kk), canonical)


# ---- the scores of a labelling: sums within a cluster, the nearest other cluster, silhouettes, medoids

def matrix_cluster_scores(m: "engine.CountMatrix", labels, mode: str = "jsd", rows=None) -> ClusterScores:
    """the scores of a labelling of rows `rows` of m (None: all; labels[i] belongs to rows[i]) over their `mode` ("jsd",
    "euclidean") distances, the cells of `matrix_cross_distances(m, m, mode, rows, rows)` computed strip by strip and
    reduced on the device: the n x n matrix never exists whole"""
    return _count_side(m, mode).cluster_scores(labels, rows)


def cluster_scores(seqs, labels, distance_mode: str = "mash", *, k: int, sketch_size: int | None = None,
                   num_states: int = 4, mash_canonical: bool = False, ctx: engine.Context | None = None,
                   canonical: bool = False) -> ClusterScores:
    """the scores of a labelling of the sequences (`ClusterScores`) over their `distance_mode` distances: the cells
    MODES[distance_mode] gives the collection (off the diagonal, which is never read), computed strip by strip and never
    held whole.  Argument checks as cluster.ctree, before any device work; ZeroDivisionError (mash) when two sequences
    have an empty sketch; NaN (jsd, euclidean) for a sequence without a valid k-mer."""
    check_mode_args(distance_mode, sketch_size, mash_canonical, canonical)
    seqs = list(seqs)
    lab = check_labels(labels, len(seqs))
    if not seqs:
        return run_cluster_scores(ctx, _NO_ROWS, lab)
    with device_side(seqs, distance_mode, *mode_args(distance_mode, k, sketch_size, num_states, mash_canonical), ctx=ctx,
                     canonical=canonical) as dev:
        return dev.cluster_scores(lab)


# ---- the cophenetic correlation of a tree with the distances it was built from

def matrix_cophenet(m: "engine.CountMatrix", Z, mode: str = "jsd", rows=None, matrix: bool = False) -> CopheneticScores:
    """the cophenetic correlation of the linkage matrix Z with the `mode` ("jsd", "euclidean") distances of rows `rows`
    of m (None: all; leaf i of Z is rows[i]): the cells of `matrix_cross_distances(m, m, mode, rows, rows)` computed
    strip by strip and reduced on the device, the n x n matrix never existing whole"""
    return _count_side(m, mode).cophenet(Z, rows, matrix)


def cophenet(seqs, Z, distance_mode: str = "mash", *, k: int, sketch_size: int | None = None, num_states: int = 4,
             mash_canonical: bool = False, matrix: bool = False, ctx: engine.Context | None = None,
             canonical: bool = False) -> CopheneticScores:
    """the cophenetic correlation (`CopheneticScores`) of the linkage matrix Z over the sequences with their
    `distance_mode` distances: scipy's cophenet(Z, Y)[0] for the condensed form Y of what MODES[distance_mode] gives the
    collection, computed strip by strip and never held whole.  Argument checks as cluster.ctree, and the shape of Z,
    before any device work; ZeroDivisionError (mash) for a sequence with an empty sketch."""
    check_mode_args(distance_mode, sketch_size, mash_canonical, canonical)
    seqs = list(seqs)
    check_linkage_matrix(Z, len(seqs))
    with device_side(seqs, distance_mode, *mode_args(distance_mode, k, sketch_size, num_states, mash_canonical), ctx=ctx,
                     canonical=canonical) as dev:
        return dev.cophenet(Z, matrix=matrix)


# ---- farthest-first (max-min) selection of representatives

def matrix_maxmin(m: "engine.CountMatrix", n_select: int | None = None, *, mode: str = "jsd", seeds=(0,),
                  min_distance: float | None = None) -> MaxMin:
    """farthest-first selection (`MaxMin`) among the rows of m by their `mode` ("jsd", "euclidean") distances: from the
    seeds on, the row farthest from the rows already taken (a tie to the lowest row), until n_select rows are taken or
    every row lies within min_distance of one.  The cells are those of the mode's square function bit for bit, one row
    of them per pick: the n x n matrix never exists.  A row without a valid k-mer is at NaN from every other: never
    picked, owner -1."""
    return _count_side(m, mode).maxmin(n_select, seeds=seeds, min_distance=min_distance)


def mash_maxmin(seqs, k: int, sketch_size: int, num_states: int = 4, mash_canonical: bool = False, *,
                n_select: int | None = None, seeds=(0,), min_distance: float | None = None,
                ctx: engine.Context | None = None) -> MaxMin:
    """farthest-first selection among the sequences by their mash distances: sketches, then a row of distances per
    pick, everything in HBM.  ZeroDivisionError where a pair the traversal visits has two empty sketches."""
    return _maxmin(seqs, "mash", k, sketch_size, num_states, mash_canonical, n_select=n_select, seeds=seeds,
                   min_distance=min_distance, ctx=ctx)


def euclidean_maxmin(seqs, k: int, num_states: int = 4, *, n_select: int | None = None, seeds=(0,),
                     min_distance: float | None = None, ctx: engine.Context | None = None, canonical: bool = False) -> MaxMin:
    """the same by the euclidean distances of the k-mer frequencies"""
    return _maxmin(seqs, "euclidean", k, num_states, n_select=n_select, seeds=seeds, min_distance=min_distance, ctx=ctx,
                   canonical=canonical)


def jsd_maxmin(seqs, k: int, num_states: int = 4, *, n_select: int | None = None, seeds=(0,),
               min_distance: float | None = None, ctx: engine.Context | None = None, canonical: bool = False) -> MaxMin:
    """the same by the Jensen-Shannon divergences of `jsd_distances`"""
    return _maxmin(seqs, "jsd", k, num_states, n_select=n_select, seeds=seeds, min_distance=min_distance, ctx=ctx,
                   canonical=canonical)


def _maxmin(seqs, distance_mode: str, *args, n_select, seeds, min_distance, ctx, canonical: bool = False) -> MaxMin:
    check_maxmin_args(len(seqs), n_select, seeds, min_distance)
    with device_side(seqs, distance_mode, *args, ctx=ctx, canonical=canonical) as dev:
        return dev.maxmin(n_select, seeds=seeds, min_distance=min_distance)


# a distance mode -> its farthest-first selection: takes (seqs, *mode_args(...)), and n_select=, seeds=, min_distance=, ctx=
MAXMIN_MODES = {"mash": mash_maxmin, "euclidean": euclidean_maxmin, "jsd": jsd_maxmin}


def maxmin(seqs, n_select: int | None = None, distance_mode: str = "mash", *, k: int, sketch_size: int | None = None,
           num_states: int = 4, mash_canonical: bool = False, seeds=(0,), min_distance: float | None = None,
           ctx: engine.Context | None = None, canonical: bool = False) -> MaxMin:
    """farthest-first (max-min) selection of representatives among the sequences by `distance_mode`: the seeds, then
    again and again the sequence farthest from those already taken, until n_select are taken (None: all) or every
    sequence lies within min_distance of one (dereplication: one representative per group within min_distance).  One
    of the two must be given.  `MaxMin` also names every sequence's nearest representative and the covering radius.
    Only n_select rows of distances are computed, never the N x N matrix.  Argument checks as cluster.ctree, and those
    of `check_maxmin_args`, before any device work."""
    check_mode_args(distance_mode, sketch_size, mash_canonical, canonical)
    seqs = list(seqs)
    return _maxmin(seqs, distance_mode, *mode_args(distance_mode, k, sketch_size, num_states, mash_canonical),
                   n_select=n_select, seeds=seeds, min_distance=min_distance, ctx=ctx, canonical=canonical)


# ---- the neighbours within a radius, and the groups they make (threshold clusters)

def matrix_within(q: "engine.CountMatrix", r: "engine.CountMatrix", radius, mode: str = "jsd", q_rows=None, r_rows=None, *,
                  skip_self: bool = False, max_pairs: int | None = None) -> Neighbours:
    """for every row q_rows of q (None: all) the rows r_rows of r at a `mode` ("jsd", "euclidean") distance <= radius
    (`Neighbours`): the cells of `matrix_cross_distances(q, r, mode, q_rows, r_rows)`, compacted on the device strip by
    strip -- only the pairs listed cross to the host.  skip_self: row i against position i is left out (q_rows and
    r_rows name the same rows of one matrix)."""
    check_radius(radius)  # (here, so that a wrong radius is reported before a wrong mode)
    return _count_side(q, mode).within(_count_side(r, mode), radius, q_rows, r_rows, skip_self=skip_self, max_pairs=max_pairs)


def matrix_threshold_clusters(m: "engine.CountMatrix", radius, mode: str = "jsd", rows=None) -> ThresholdClusters:
    """the groups that "`mode` distance <= radius" makes of rows `rows` of m (None: all): `ThresholdClusters`, the flat
    clusters of their single-linkage tree cut at height radius, without the n x n matrix and without the tree"""
    check_radius(radius)  # (as in `matrix_within`)
    return _count_side(m, mode).threshold_clusters(radius, rows)


def within(queries, refs, radius, distance_mode: str = "mash", *, k: int, sketch_size: int | None = None,
           num_states: int = 4, mash_canonical: bool = False, canonical: bool = False, max_pairs: int | None = None,
           ctx: engine.Context | None = None) -> Neighbours:
    """for every query sequence the reference sequences at a `distance_mode` distance <= radius (`Neighbours`: positions
    in `refs`, ascending, and the cells `cross_distances` gives the same pairs, bit for bit).  The M x N matrix is never
    held whole and never crosses to the host.  The radius, max_pairs and the arguments cluster.ctree checks are checked
    before any device work; ZeroDivisionError and NaN cells as `cross_distances`; NotImplementedError once more than
    max_pairs pairs are found."""
    radius = check_radius(radius)
    check_max_pairs(max_pairs)
    check_mode_args(distance_mode, sketch_size, mash_canonical, canonical)
    queries, refs = list(queries), list(refs)
    if not queries or not refs:
        return _no_neighbours(len(queries))
    return _two_sides(queries, refs, distance_mode, mode_args(distance_mode, k, sketch_size, num_states, mash_canonical),
                      ctx, lambda q, r: q.within(r, radius, max_pairs=max_pairs), canonical)


def neighbours(seqs, radius, distance_mode: str = "mash", *, k: int, sketch_size: int | None = None, num_states: int = 4,
               mash_canonical: bool = False, canonical: bool = False, max_pairs: int | None = None,
               ctx: engine.Context | None = None) -> Neighbours:
    """`within` of a collection against itself, a sequence not listed as its own neighbour: every pair (i, j), i != j,
    at a distance <= radius, from both of its ends"""
    radius = check_radius(radius)
    check_max_pairs(max_pairs)
    check_mode_args(distance_mode, sketch_size, mash_canonical, canonical)
    seqs = list(seqs)
    if not seqs:
        return _no_neighbours(0)
    with device_side(seqs, distance_mode, *mode_args(distance_mode, k, sketch_size, num_states, mash_canonical), ctx=ctx,
                     canonical=canonical) as dev:
        return dev.within(dev, radius, skip_self=True, max_pairs=max_pairs)


def threshold_clusters(seqs, radius, distance_mode: str = "mash", *, k: int, sketch_size: int | None = None,
                       num_states: int = 4, mash_canonical: bool = False, canonical: bool = False,
                       ctx: engine.Context | None = None) -> ThresholdClusters:
    """the groups that "`distance_mode` distance <= radius" makes of the sequences (`ThresholdClusters`): connected
    components, i.e. the flat clusters of the single-linkage tree cut at height radius (dereplication: "cluster at mash
    distance 0.05"), without the N x N matrix and without the tree.  Argument checks as `within`; ZeroDivisionError (mash)
    as `cluster_scores`; a sequence without a valid k-mer (jsd, euclidean: NaN distances) is a cluster of its own."""
    radius = check_radius(radius)
    check_mode_args(distance_mode, sketch_size, mash_canonical, canonical)
    seqs = list(seqs)
    if not seqs:
        return run_threshold_clusters(ctx, _NO_ROWS, radius)
    with device_side(seqs, distance_mode, *mode_args(distance_mode, k, sketch_size, num_states, mash_canonical), ctx=ctx,
                     canonical=canonical) as dev:
        return dev.threshold_clusters(radius)


# ---- the minimum spanning tree: single linkage without the matrix

def matrix_mst(m: "engine.CountMatrix", mode: str = "jsd", rows=None, *, min_samples: int | None = None, core=None) -> MST:
    """the minimum spanning tree (`MST`) of the `mode` ("jsd", "euclidean") distances of rows `rows` of m (None: all),
    a Boruvka round per pass over the strips: the n x n matrix never exists.  A row without a valid k-mer (NaN distances)
    is a tree of its own.  min_samples, core: as `DeviceSide.mst` takes them (mutual reachability)."""
    return _count_side(m, mode).mst(rows, min_samples=min_samples, core=core)


def mash_mst(seqs, k: int, sketch_size: int, num_states: int = 4, mash_canonical: bool = False, *,
             min_samples: int | None = None, core=None, ctx: engine.Context | None = None) -> MST:
    """the minimum spanning tree of the sequences by their mash distances: sketches, then a pass over the strips per
    round, everything in HBM.  ZeroDivisionError as `cluster_scores`."""
    return _mst(seqs, "mash", k, sketch_size, num_states, mash_canonical, min_samples=min_samples, core=core, ctx=ctx)


def euclidean_mst(seqs, k: int, num_states: int = 4, *, min_samples: int | None = None, core=None,
                  ctx: engine.Context | None = None, canonical: bool = False) -> MST:
    """the same by the euclidean distances of the k-mer frequencies"""
    return _mst(seqs, "euclidean", k, num_states, min_samples=min_samples, core=core, ctx=ctx, canonical=canonical)


def jsd_mst(seqs, k: int, num_states: int = 4, *, min_samples: int | None = None, core=None,
            ctx: engine.Context | None = None, canonical: bool = False) -> MST:
    """the same by the Jensen-Shannon divergences of `jsd_distances`"""
    return _mst(seqs, "jsd", k, num_states, min_samples=min_samples, core=core, ctx=ctx, canonical=canonical)


def _mst(seqs, distance_mode: str, *args, min_samples, core, ctx, canonical: bool = False) -> MST:
    if min_samples is not None and core is not None:
        raise ValueError("mst takes at most one of min_samples and core")
    if min_samples is not None:
        check_min_samples(min_samples, len(seqs))
    check_core(core, len(seqs))
    if not len(seqs):
        return run_mst(ctx, _NO_ROWS)
    with device_side(seqs, distance_mode, *args, ctx=ctx, canonical=canonical) as dev:
        return dev.mst(min_samples=min_samples, core=core)


# a distance mode -> its minimum spanning tree: takes (seqs, *mode_args(...)), and min_samples=, core=, ctx=
MST_MODES = {"mash": mash_mst, "euclidean": euclidean_mst, "jsd": jsd_mst}


def mst(seqs, distance_mode: str = "mash", *, k: int, sketch_size: int | None = None, num_states: int = 4,
        mash_canonical: bool = False, canonical: bool = False, min_samples: int | None = None, core=None,
        ctx: engine.Context | None = None) -> MST:
    """the minimum spanning tree (`MST`) of the sequences by `distance_mode`: single linkage -- and, with min_samples or
    core, robust single linkage over the mutual-reachability distance -- for collections whose N x N matrix could never
    exist.  Every round recomputes all N x N cells strip by strip and there are at most ceil(log2 N) rounds; where the
    matrix fits, `MODES[distance_mode]`'s linkage with method "single" is the faster route to the same heights.  Argument
    checks as cluster.ctree, and those of `check_min_samples` and `check_core`, before any device work."""
    check_mode_args(distance_mode, sketch_size, mash_canonical, canonical)
    seqs = list(seqs)
    return _mst(seqs, distance_mode, *mode_args(distance_mode, k, sketch_size, num_states, mash_canonical),
                min_samples=min_samples, core=core, ctx=ctx, canonical=canonical)


# ---- principal coordinates (PCoA, classical MDS) and the projection of further rows

def matrix_pcoa(m: "engine.CountMatrix", mode: str = "jsd", n_axes: int = 3, *, tol: float = 1e-8,
                max_basis: int | None = None, strict: bool = True) -> PCoA:
    """`pcoa` over the rows of a matrix already in HBM, by `mode` ("jsd" or "euclidean")"""
    return _count_side(m, mode).pcoa(n_axes, tol=tol, max_basis=max_basis, strict=strict)


def matrix_pcoa_project(fit: PCoA, q: "engine.CountMatrix", r: "engine.CountMatrix", mode: str = "jsd", q_rows=None,
                        r_rows=None) -> np.ndarray:
    """the coordinates of rows q_rows of q (None: all) in the ordination `fit` of rows r_rows of r, by `mode`: float64
    [M, n_axes]; q and r as `matrix_cross_distances` takes them"""
    return _count_side(q, mode).pcoa_project(fit, _count_side(r, mode), q_rows, r_rows)


def mash_pcoa(seqs, k: int, sketch_size: int, num_states: int = 4, mash_canonical: bool = False, *, n_axes: int = 3,
              tol: float = 1e-8, max_basis: int | None = None, strict: bool = True,
              ctx: engine.Context | None = None) -> PCoA:
    """the principal coordinates of the mash distances on the device: sketches, the N x N distances and the iteration,
    every stage in HBM; only the n_axes eigenpairs come back.  ZeroDivisionError as `mash_distances`."""
    return _pcoa(seqs, "mash", k, sketch_size, num_states, mash_canonical, n_axes=n_axes, tol=tol, max_basis=max_basis,
                 strict=strict, ctx=ctx)


def euclidean_pcoa(seqs, k: int, num_states: int = 4, *, n_axes: int = 3, tol: float = 1e-8, max_basis: int | None = None,
                   strict: bool = True, ctx: engine.Context | None = None, canonical: bool = False) -> PCoA:
    """the same for the euclidean distances (a sequence without valid k-mers: NaN distances, ValueError)"""
    return _pcoa(seqs, "euclidean", k, num_states, n_axes=n_axes, tol=tol, max_basis=max_basis, strict=strict, ctx=ctx,
                 canonical=canonical)


def jsd_pcoa(seqs, k: int, num_states: int = 4, *, n_axes: int = 3, tol: float = 1e-8, max_basis: int | None = None,
             strict: bool = True, ctx: engine.Context | None = None, canonical: bool = False) -> PCoA:
    """the same for the Jensen-Shannon divergences of `jsd_distances` (a sequence without valid k-mers: ValueError)"""
    return _pcoa(seqs, "jsd", k, num_states, n_axes=n_axes, tol=tol, max_basis=max_basis, strict=strict, ctx=ctx,
                 canonical=canonical)


def _pcoa(seqs, distance_mode: str, *args, n_axes, tol, max_basis, strict, ctx, canonical: bool = False) -> PCoA:
    check_pcoa_args(len(seqs), n_axes, tol, max_basis)
    with device_side(seqs, distance_mode, *args, ctx=ctx, canonical=canonical) as dev:
        return dev.pcoa(n_axes, tol=tol, max_basis=max_basis, strict=strict)


# a distance mode -> its principal coordinates: takes (seqs, *mode_args(...)), and n_axes=, tol=, max_basis=, strict=, ctx=
PCOA_MODES = {"mash": mash_pcoa, "euclidean": euclidean_pcoa, "jsd": jsd_pcoa}


def pcoa(seqs, n_axes: int = 3, distance_mode: str = "mash", *, k: int, sketch_size: int | None = None, num_states: int = 4,
         mash_canonical: bool = False, tol: float = 1e-8, max_basis: int | None = None, strict: bool = True,
         ctx: engine.Context | None = None, canonical: bool = False) -> PCoA:
    """the principal coordinates (`PCoA`) of the `distance_mode` distances of a collection of sequences: the distances
    are written into HBM and stay there, only the n_axes eigenpairs come back.  Argument checks as cluster.ctree and
    those of `check_pcoa_args`, before any device work."""
    check_mode_args(distance_mode, sketch_size, mash_canonical, canonical)
    seqs = list(seqs)
    return _pcoa(seqs, distance_mode, *mode_args(distance_mode, k, sketch_size, num_states, mash_canonical), n_axes=n_axes,
                 tol=tol, max_basis=max_basis, strict=strict, ctx=ctx, canonical=canonical)


def pcoa_project(fit: PCoA, queries, refs, distance_mode: str = "mash", *, k: int, sketch_size: int | None = None,
                 num_states: int = 4, mash_canonical: bool = False, ctx: engine.Context | None = None,
                 canonical: bool = False) -> np.ndarray:
    """the coordinates of every query sequence in the ordination `fit` of the sequences `refs` (the fitted ones, in the
    fit's order) by Gower's formula over the `distance_mode` distances: float64 [M, n_axes].  Only the M x N distances
    are computed, strip by strip, and none leaves the device.  A query without a valid k-mer (jsd, euclidean) gets NaN
    coordinates.  Argument checks as `cross_distances` and the fit's shapes, before any device work."""
    check_mode_args(distance_mode, sketch_size, mash_canonical, canonical)
    queries, refs = list(queries), list(refs)
    values, _, _ = check_pcoa_fit(fit, len(refs))
    if not queries:
        return np.zeros((0, values.size), dtype=np.float64)
    return _two_sides(queries, refs, distance_mode, mode_args(distance_mode, k, sketch_size, num_states, mash_canonical),
                      ctx, lambda q, r: q.pcoa_project(fit, r), canonical)


# ---- k-medoids (PAM): the representatives that minimise the total distance

def matrix_kmedoids(m: "engine.CountMatrix", n_medoids: int, *, mode: str = "jsd", init="build",
                    max_swaps: int = 300) -> KMedoids:
    """`kmedoids` over the rows of a matrix already in HBM, by `mode` ("jsd" or "euclidean")"""
    return _count_side(m, mode).kmedoids(n_medoids, init=init, max_swaps=max_swaps)


def mash_kmedoids(seqs, k: int, sketch_size: int, num_states: int = 4, mash_canonical: bool = False, *, n_medoids: int,
                  init="build", max_swaps: int = 300, ctx: engine.Context | None = None) -> KMedoids:
    """k-medoids of the mash distances on the device: sketches, the N x N distances and the search, every stage in HBM.
    ZeroDivisionError as `mash_distances`."""
    return _kmedoids(seqs, "mash", k, sketch_size, num_states, mash_canonical, n_medoids=n_medoids, init=init,
                     max_swaps=max_swaps, ctx=ctx)


def euclidean_kmedoids(seqs, k: int, num_states: int = 4, *, n_medoids: int, init="build", max_swaps: int = 300,
                       ctx: engine.Context | None = None, canonical: bool = False) -> KMedoids:
    """the same for the euclidean distances (a sequence without valid k-mers: NaN distances, ValueError)"""
    return _kmedoids(seqs, "euclidean", k, num_states, n_medoids=n_medoids, init=init, max_swaps=max_swaps, ctx=ctx,
                     canonical=canonical)


def jsd_kmedoids(seqs, k: int, num_states: int = 4, *, n_medoids: int, init="build", max_swaps: int = 300,
                 ctx: engine.Context | None = None, canonical: bool = False) -> KMedoids:
    """the same for the Jensen-Shannon divergences of `jsd_distances` (a sequence without valid k-mers: ValueError)"""
    return _kmedoids(seqs, "jsd", k, num_states, n_medoids=n_medoids, init=init, max_swaps=max_swaps, ctx=ctx,
                     canonical=canonical)


def _kmedoids(seqs, distance_mode: str, *args, n_medoids, init, max_swaps, ctx, canonical: bool = False) -> KMedoids:
    check_kmedoids_args(len(seqs), n_medoids, init, max_swaps)
    with device_side(seqs, distance_mode, *args, ctx=ctx, canonical=canonical) as dev:
        return dev.kmedoids(n_medoids, init=init, max_swaps=max_swaps)


# a distance mode -> its k-medoids: takes (seqs, *mode_args(...)), and n_medoids=, init=, max_swaps=, ctx=
KMEDOIDS_MODES = {"mash": mash_kmedoids, "euclidean": euclidean_kmedoids, "jsd": jsd_kmedoids}


def kmedoids(seqs, n_medoids: int, distance_mode: str = "mash", *, k: int, sketch_size: int | None = None,
             num_states: int = 4, mash_canonical: bool = False, init="build", max_swaps: int = 300,
             ctx: engine.Context | None = None, canonical: bool = False) -> KMedoids:
    """k-medoids (`KMedoids`) of a collection of sequences by `distance_mode`: the n_medoids sequences that lie closest,
    in total, to everything else, with the partition they make -- representation, where `maxmin` gives coverage of the
    worst case and `nmost` diversity.  The distances are written into HBM and stay there.  init: "build" (PAM's BUILD),
    "maxmin" (the farthest-first picks as the start: cheaper, usually a higher td) or the initial medoids as rows;
    max_swaps = 0 scores a set as it is.  Argument checks as cluster.ctree and those of `check_kmedoids_args`, before
    any device work."""
    check_mode_args(distance_mode, sketch_size, mash_canonical, canonical)
    seqs = list(seqs)
    return _kmedoids(seqs, distance_mode, *mode_args(distance_mode, k, sketch_size, num_states, mash_canonical),
                     n_medoids=n_medoids, init=init, max_swaps=max_swaps, ctx=ctx, canonical=canonical)


# ---- PERMANOVA: do the groups explain the distances?

def matrix_permanova(m: "engine.CountMatrix", grouping, *, mode: str = "jsd", permutations: int = 999, seed=None,
                     strata=None) -> PERMANOVA:
    """`permanova` over the rows of a matrix already in HBM, by `mode` ("jsd" or "euclidean")"""
    return _count_side(m, mode).permanova(grouping, permutations=permutations, seed=seed, strata=strata)


def mash_permanova(seqs, k: int, sketch_size: int, num_states: int = 4, mash_canonical: bool = False, *, grouping,
                   permutations: int = 999, seed=None, strata=None, ctx: engine.Context | None = None) -> PERMANOVA:
    """PERMANOVA of the mash distances on the device: sketches, the N x N distances and the sums under every
    permutation, every stage in HBM.  ZeroDivisionError as `mash_distances`."""
    return _permanova(seqs, "mash", k, sketch_size, num_states, mash_canonical, grouping=grouping, permutations=permutations,
                      seed=seed, strata=strata, ctx=ctx)


def euclidean_permanova(seqs, k: int, num_states: int = 4, *, grouping, permutations: int = 999, seed=None, strata=None,
                        ctx: engine.Context | None = None, canonical: bool = False) -> PERMANOVA:
    """the same for the euclidean distances (a sequence without valid k-mers: NaN distances, ValueError)"""
    return _permanova(seqs, "euclidean", k, num_states, grouping=grouping, permutations=permutations, seed=seed,
                      strata=strata, ctx=ctx, canonical=canonical)


def jsd_permanova(seqs, k: int, num_states: int = 4, *, grouping, permutations: int = 999, seed=None, strata=None,
                  ctx: engine.Context | None = None, canonical: bool = False) -> PERMANOVA:
    """the same for the Jensen-Shannon divergences of `jsd_distances` (a sequence without valid k-mers: ValueError)"""
    return _permanova(seqs, "jsd", k, num_states, grouping=grouping, permutations=permutations, seed=seed, strata=strata,
                      ctx=ctx, canonical=canonical)


def _permanova(seqs, distance_mode: str, *args, grouping, permutations, seed, strata, ctx, canonical: bool = False) -> PERMANOVA:
    checked = check_permanova_args(len(seqs), grouping, permutations, seed, strata)
    with device_side(seqs, distance_mode, *args, ctx=ctx, canonical=canonical) as dev:
        return run_permanova(dev.ctx, dev._source(), *checked)  # (the label vectors are drawn once)


# a distance mode -> its PERMANOVA: takes (seqs, *mode_args(...)), and grouping=, permutations=, seed=, strata=, ctx=
PERMANOVA_MODES = {"mash": mash_permanova, "euclidean": euclidean_permanova, "jsd": jsd_permanova}


def permanova(seqs, grouping, distance_mode: str = "mash", *, k: int, sketch_size: int | None = None, num_states: int = 4,
              mash_canonical: bool = False, permutations: int = 999, seed=None, strata=None,
              ctx: engine.Context | None = None, canonical: bool = False) -> PERMANOVA:
    """PERMANOVA (`PERMANOVA`) of a grouping of a collection of sequences by `distance_mode`: are the distances between
    the groups larger than within them, beyond chance?  The test that goes with `pcoa`.  The distances are written into
    HBM and stay there; one pass over them serves a batch of permutations.

    grouping: any sequence of hashables, one per sequence (host species, sampling site, the labels of `cut_tree`,
    `kmedoids` or `threshold_clusters`), encoded 0 .. a - 1 in the order of first appearance.  permutations: how many
    label vectors are drawn (0: the statistic alone, p_value nan); seed: of numpy.random.default_rng, from which one
    rng.permutation(n) is drawn per label vector, in order (`permuted_labels` has the rule); strata: a second sequence
    of hashables, labels are then permuted inside its blocks only.  Argument checks as cluster.ctree and those of
    `check_permanova_args`, before any device work."""
    check_mode_args(distance_mode, sketch_size, mash_canonical, canonical)
    seqs = list(seqs)
    return _permanova(seqs, distance_mode, *mode_args(distance_mode, k, sketch_size, num_states, mash_canonical),
                      grouping=grouping, permutations=permutations, seed=seed, strata=strata, ctx=ctx, canonical=canonical)
