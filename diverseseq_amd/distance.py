"""Host side of the distance path: mirrors diverse_seq/distance.py's functions
(mash_sketches :178-227, mash_distances :119-175, mash_distance :230-291,
euclidean_distances :294-332) and the strided chunks of
diverse_seq/cluster.py:607-644, with the arithmetic in libdvs_hip.so; the pairwise Jensen-Shannon
divergence of k-mer frequencies (jsd_distances: total_jsd of a two-member set, src/records.rs:27-68);
and the fused ctree stages
(distances and the linkage tree with the N x N matrix left in HBM); and the distances between two collections
(cross_distances: M queries against N references, no counterpart in the reference) with the k nearest references
of every query (nearest), the M x N matrix computed strip by strip and never leaving the device; and the scores of a
labelling of one collection over the same strips (cluster_scores: sums within a cluster, the nearest other cluster,
silhouettes, medoids; no counterpart in the reference); and, over the same strips again, the correlation of the distances
with the cophenetic distances of a tree (cophenet: scipy's cophenet(Z, Y)[0]; no counterpart in the reference); and
the neighbour-joining tree of each distance mode (mash_nj, euclidean_nj, jsd_nj: csrc/nj.hip, an unrooted tree with
branch lengths, the matrix left in HBM as for the linkage trees; no counterpart in the reference); and farthest-first
(max-min) selection of representatives by any of these distances (maxmin, matrix_maxmin, Sketches.maxmin:
csrc/maxmin.hip, one row of distances per pick and never the matrix; no counterpart in the reference); and the sparse
product over the same strips: the pairs within a radius (within, neighbours, matrix_within -> `Neighbours`) and the
groups they make (threshold_clusters, matrix_threshold_clusters -> `ThresholdClusters`: connected components, the
single-linkage clusters at that height), each strip compacted on the device (csrc/within.hip) so that only the listed
pairs cross to the host; no counterpart in the reference; and the ordination of a collection's distances, principal
coordinates (pcoa, matrix_pcoa, mash_pcoa / euclidean_pcoa / jsd_pcoa -> `PCoA`: csrc/pcoa.hip, the few largest eigenpairs
of the double-centred matrix by an iteration that only reads the N x N matrix in HBM) with the projection of further
rows into a fitted ordination (pcoa_project, matrix_pcoa_project: Gower's formula beside each strip of
cross_distances, csrc/pcoa.hip behind the strip driver of csrc/crossdist.hip); no counterpart in the reference; and
the representatives that lie closest, in total, to everything else, k-medoids (kmedoids, matrix_kmedoids,
mash_kmedoids / euclidean_kmedoids / jsd_kmedoids ->
`KMedoids`: csrc/kmedoids.hip, PAM's BUILD and FastPAM1's swaps over the N x N matrix in HBM); no counterpart in the
reference; and the tree without the matrix, the minimum spanning tree (mst, matrix_mst, mash_mst / euclidean_mst /
jsd_mst -> `MST`: csrc/mst.hip, a Boruvka round per pass over the strips of cross_distances; single linkage, and with a
core vector the mutual-reachability tree of HDBSCAN); no counterpart in the reference; and the test that goes with
the ordination, PERMANOVA (permanova, matrix_permanova, mash_permanova / euclidean_permanova / jsd_permanova ->
`PERMANOVA`: csrc/permanova.hip, whether a grouping of the sequences explains their distances -- a pseudo-F statistic
and its p-value under permutations of the labels, a batch of permutations per pass over the N x N matrix in HBM); no
counterpart in the reference.  `DeviceSide`
is what a mode keeps in HBM of one batch, with every one of these operations as a method; the per-mode functions, the
matrix_* functions and the Sketches methods are a few lines over it.  Every operation has one C entry, which takes a
`_lib.Source` (dvs_source: the mode and its handle, or a caller's matrix): `make_source` fills one per call."""

from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _lib, engine

_U32_MAX = 0xFFFFFFFF


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


def make_source(kind: int, handle, n: int, rows: np.ndarray | None = None, *, k: int = 0, sketch_size: int = 0,
                on_device: int = 0, keep=None) -> _lib.Source:
    """the dvs_source of one call: `kind` (_lib.SRC_*), the handle or matrix pointer, the `n` rows taken and their
    optional uint32 row list.  What its pointers refer to -- the row array, and `keep`, the owner of a caller's
    matrix -- lives as long as the structure does"""
    src = _lib.Source(kind, handle, _lib.ptr(rows, C.c_uint32), n, k, sketch_size, on_device)
    src._keep = (handle, rows, keep)
    return src


def run_linkage(ctx: engine.Context | None, n: int, src: _lib.Source, code: int,
                too_few: str = "need at least two sequences to build a tree") -> np.ndarray:
    """dvs_linkage over `src` with the method `code` for n leaves -> Z; ValueError(too_few) before any device work
    when n < 2"""
    if n < 2:
        raise ValueError(too_few)
    ctx = ctx or engine.default_context()
    pairs, heights, sizes = tree_outputs(n)
    ctx.check(ctx._L.dvs_linkage(ctx._h, src, code, _lib.ptr(pairs, C.c_uint32), _lib.ptr(heights, C.c_double),
                                 _lib.ptr(sizes, C.c_uint32)))
    return linkage_matrix(pairs, heights, sizes)


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


def sketch_batch(seqs, k: int, sketch_size: int, num_states: int = 4,
                 mash_canonical: bool = False, ctx: engine.Context | None = None):
    """bottom-`sketch_size` sketches of a batch -> (uint32 [n, stride], lens uint32 [n]);
    stride = min(sketch_size, longest possible sketch)"""
    ctx = ctx or engine.default_context()
    data, offsets = engine.concat(seqs)
    n = len(seqs)
    stride = _sketch_stride(offsets, k, sketch_size)
    sk = np.zeros((n, stride), dtype=np.uint32)
    lens = np.zeros(n, dtype=np.uint32)
    if n and sketch_size:
        ctx.check(ctx._L.dvs_mash_sketch(ctx._h, data.ctypes.data_as(C.c_void_p), 0,
                                         _lib.ptr(offsets, C.c_uint64), n, k, stride, num_states,
                                         int(bool(mash_canonical)), _lib.ptr(sk, C.c_uint32),
                                         _lib.ptr(lens, C.c_uint32)))
    return sk, lens


def mash_sketches(seqs, k: int, sketch_size: int, num_states: int = 4,
                  mash_canonical: bool = False) -> list[list[int]]:
    sk, lens = sketch_batch(seqs, k, sketch_size, num_states, mash_canonical)
    return [sk[i, : int(lens[i])].tolist() for i in range(len(seqs))]


def distances_from_sketches(sk: np.ndarray, lens: np.ndarray, k: int, sketch_size: int, *,
                            row_start: int = 0, row_stride: int = 1, symmetric: bool = True,
                            out: np.ndarray | None = None,
                            ctx: engine.Context | None = None) -> np.ndarray:
    """lower-triangle mash distances for rows row_start, row_start+row_stride, ...
    (compute_mash_chunk_distances, diverse_seq/cluster.py:640-644)"""
    ctx = ctx or engine.default_context()
    sk = np.ascontiguousarray(sk, dtype=np.uint32)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    n = sk.shape[0]
    dist = _dist_out(out, n)
    ctx.check(ctx._L.dvs_mash_distances(ctx._h, _lib.ptr(sk, C.c_uint32), sk.shape[1],
                                        _lib.ptr(lens, C.c_uint32), n, k,
                                        min(int(sketch_size), _U32_MAX), row_start, row_stride,
                                        int(symmetric), _lib.ptr(dist, C.c_double)))
    return dist


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


class Sketches:
    """bottom-s sketches of a batch resident in HBM (dvs_sketches): the hand-over between the two
    stages of ctree (diverse_seq/cluster.py:241-297) without a trip through the host"""

    def __init__(self, seqs, k: int, sketch_size: int, num_states: int = 4, mash_canonical: bool = False,
                 ctx: engine.Context | None = None, dev_ptr: int | None = None, offsets=None,
                 packed: "engine.Packed | None" = None, batch: "engine.SeqBatch | None" = None):
        """seqs: host sequences; or dev_ptr + offsets: bytes already in HBM; or packed + offsets: a packed batch
        (engine.Packed); or batch: an ingested engine.SeqBatch (packed or not)"""
        self.ctx = ctx or (batch.ctx if batch is not None else packed.ctx if packed is not None else engine.default_context())
        if batch is not None:
            offsets, seqs = batch.offsets, _lib.make_seqs(_lib.SEQ_BATCH, batch._h)
        elif packed is not None:
            seqs = _lib.make_seqs(_lib.SEQ_PACKED, packed._h, offsets)
        elif dev_ptr is not None:  # sequences already in HBM
            seqs = _lib.make_seqs(_lib.SEQ_DEVICE, dev_ptr, offsets)
        else:
            data, offsets = engine.concat(seqs)
            seqs = _lib.make_seqs(_lib.SEQ_HOST, data.ctypes.data, offsets, keep=data)
        offsets = np.asarray(offsets)
        self.n = offsets.size - 1
        self.stride = _sketch_stride(offsets, k, sketch_size) if sketch_size else 0
        self.k, self.sketch_size = k, int(sketch_size)
        h = C.c_void_p()
        self.ctx.check(self.ctx._L.dvs_sketches_build(self.ctx._h, seqs, k, self.stride, num_states,
                                                      int(bool(mash_canonical)), C.byref(h)))
        self._h = h
        self._source = batch if batch is not None else packed  # (its planes must outlive the sketch kernels)

    def close(self):
        if getattr(self, "_h", None):
            self.ctx._L.dvs_sketches_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def to_host(self):
        """(uint32 [n, stride], lens uint32 [n])"""
        sk = np.zeros((self.n, max(self.stride, 1)), dtype=np.uint32)
        lens = np.zeros(self.n, dtype=np.uint32)
        self.ctx.check(self.ctx._L.dvs_sketches_get(self.ctx._h, self._h, _lib.ptr(sk, C.c_uint32), _lib.ptr(lens, C.c_uint32)))
        return sk, lens

    @classmethod
    def from_device(cls, ctx: engine.Context, sk_ptr: int, lens_ptr: int, n: int, stride: int, k: int,
                    sketch_size: int, keep=None) -> "Sketches":
        """sketches that already sit in HBM (uint32 [n, stride] ascending, uint32 [n] lengths) -- e.g. an
        all_gather's output -- wrapped without a copy; `keep`: whatever owns the two buffers, kept alive beside the
        handle"""
        self = cls.__new__(cls)
        self.ctx, self.n, self.k, self.sketch_size, self.stride = ctx, int(n), k, int(sketch_size), int(stride)
        h = C.c_void_p()
        ctx.check(ctx._L.dvs_sketches_from_device(ctx._h, C.c_void_p(sk_ptr), C.c_void_p(lens_ptr), self.n, self.stride,
                                                  C.byref(h)))
        self._h, self._source = h, keep
        return self

    def copy_to_device(self, dst_ptr: int, dst_stride: int, dst_lens_ptr: int):
        """this batch's sketches into a caller's device buffer whose rows are dst_stride words apart (a collective's
        send buffer); enqueued on the context's stream"""
        self.ctx.check(self.ctx._L.dvs_sketches_copy_to_device(self.ctx._h, self._h, C.c_void_p(dst_ptr), int(dst_stride),
                                                               C.c_void_p(dst_lens_ptr)))

    @property
    def sketch_size_u32(self) -> int:
        """the sketch size as the C entries take it"""
        return min(self.sketch_size, _U32_MAX)

    def distances_device(self, dist_ptr: int, zerodiv_ptr: int, *, row_start: int = 0, row_stride: int = 1,
                         symmetric: bool = True):
        """the visited cells into a device matrix (float64 [n, n]) of the caller's; enqueued, not waited for;
        the uint32 at zerodiv_ptr is set where `distances` would raise ZeroDivisionError"""
        self.ctx.check(self.ctx._L.dvs_sketches_distances_device(self.ctx._h, self._h, self.k, self.sketch_size_u32,
                                                                 row_start, row_stride, int(symmetric), C.c_void_p(dist_ptr),
                                                                 C.c_void_p(zerodiv_ptr)))

    def distances(self, *, row_start: int = 0, row_stride: int = 1, symmetric: bool = True,
                  out: np.ndarray | None = None) -> np.ndarray:
        dist = _dist_out(out, self.n)
        self.ctx.check(self.ctx._L.dvs_sketches_distances(self.ctx._h, self._h, self.k, self.sketch_size_u32,
                                                          row_start, row_stride, int(symmetric), _lib.ptr(dist, C.c_double)))
        return dist

    # every other operation over the mash distances of these sketches: `DeviceSide`'s, for the mode "mash"

    def linkage(self, method: str = "average") -> np.ndarray:
        """scipy's linkage matrix Z of `method` (LINKAGE_METHODS) over the mash distances of every pair: the N x N
        matrix is written and read in HBM (dvs_linkage); ZeroDivisionError as `distances`"""
        return DeviceSide(self, "mash").linkage(method)

    def cross_distances(self, other: "Sketches", rows=None, other_rows=None) -> np.ndarray:
        """the mash distances of this set's sketches `rows` (None: all) against `other`'s `other_rows`: float64 [M, N],
        every cell the bits `distances` gives the same two sketches (dvs_cross_distances);
        ZeroDivisionError as `distances`"""
        return DeviceSide(self, "mash").cross_distances(DeviceSide(other, "mash"), rows, other_rows)

    def nearest(self, other: "Sketches", n_nearest: int = 1, rows=None, other_rows=None):
        """the n_nearest sketches of `other` (positions into other_rows, or rows) nearest to each of this set's, nearest
        first, a tie to the lower position: (int64 [M, n_nearest], -1 in a slot without a reference; float64 distances,
        NaN there) (dvs_nearest)"""
        return DeviceSide(self, "mash").nearest(DeviceSide(other, "mash"), n_nearest, rows, other_rows)

    def cluster_scores(self, labels, rows=None) -> "ClusterScores":
        """the scores of a labelling (`ClusterScores`) of this set's sketches `rows` (None: all; labels[i] belongs to
        rows[i]) over their mash distances, computed strip by strip (dvs_cluster_scores); ZeroDivisionError
        as `distances`"""
        return DeviceSide(self, "mash").cluster_scores(labels, rows)

    def cophenet(self, Z, rows=None, matrix: bool = False) -> "CopheneticScores":
        """the cophenetic correlation (`CopheneticScores`) of the linkage matrix Z with the mash distances of this set's
        sketches `rows` (None: all; leaf i of Z is rows[i]), computed strip by strip (dvs_cophenet);
        ZeroDivisionError as `cluster_scores`"""
        return DeviceSide(self, "mash").cophenet(Z, rows, matrix)

    def maxmin(self, n_select: int | None = None, *, seeds=(0,), min_distance: float | None = None) -> "MaxMin":
        """farthest-first selection (`MaxMin`) among this set's sketches by their mash distances, a row of distances
        per pick (dvs_maxmin); ZeroDivisionError where a pair the traversal visits has two empty sketches"""
        return DeviceSide(self, "mash").maxmin(n_select, seeds=seeds, min_distance=min_distance)

    def kmedoids(self, n_medoids: int, *, init="build", max_swaps: int = 300) -> "KMedoids":
        """k-medoids (`KMedoids`) of this set's sketches over their mash distances, the N x N matrix written and only
        read in HBM (dvs_kmedoids); ZeroDivisionError as `distances`"""
        return DeviceSide(self, "mash").kmedoids(n_medoids, init=init, max_swaps=max_swaps)

    def permanova(self, grouping, *, permutations: int = 999, seed=None, strata=None) -> "PERMANOVA":
        """PERMANOVA (`PERMANOVA`) of a grouping of this set's sketches over their mash distances, the N x N matrix
        written and only read in HBM (dvs_permanova); ZeroDivisionError as `distances`"""
        return DeviceSide(self, "mash").permanova(grouping, permutations=permutations, seed=seed, strata=strata)

    def within(self, other: "Sketches", radius, rows=None, other_rows=None, *, skip_self: bool = False,
               max_pairs: int | None = None) -> "Neighbours":
        """for each of this set's sketches `rows` the sketches of `other` at a mash distance <= radius (`Neighbours`:
        the cells of `cross_distances`, compacted on the device; dvs_within); ZeroDivisionError as
        `cross_distances`"""
        check_radius(radius)
        return DeviceSide(self, "mash").within(DeviceSide(other, "mash"), radius, rows, other_rows, skip_self=skip_self,
                                               max_pairs=max_pairs)

    def threshold_clusters(self, radius, rows=None) -> "ThresholdClusters":
        """the groups that "mash distance <= radius" makes of this set's sketches `rows` (`ThresholdClusters`;
        dvs_threshold_clusters); ZeroDivisionError as `cluster_scores`"""
        check_radius(radius)
        return DeviceSide(self, "mash").threshold_clusters(radius, rows)


class OrdinationOps:
    """The ordination operations of a `DeviceSide` -- principal coordinates and the projection into a fitted ordination
    -- which it inherits: `DeviceSide.pcoa`, `DeviceSide.pcoa_project`.  They stand in a base class of their own, as
    every operation added after the first ten does; tests/test_blocks_host.py collects the operations of `DeviceSide`
    through its base classes and demands a case of its table for each in every mode (more cases: tests/test_gpu_pcoa.py)."""

    def pcoa(self, n_axes: int = 3, *, tol: float = 1e-8, max_basis: int | None = None, strict: bool = True) -> "PCoA":
        """the principal coordinates of the distances (`PCoA`), the N x N matrix written and only read in HBM"""
        args = check_pcoa_args(self.n, n_axes, tol, max_basis)
        return run_pcoa(self.ctx, self.n, self._source(), *args, strict)

    def pcoa_project(self, fit: "PCoA", other: "DeviceSide", rows=None, other_rows=None) -> np.ndarray:
        """the coordinates of this side's `rows` (None: all) in the ordination `fit` of `other`'s `other_rows` (None:
        all; they are the fitted rows, in the fit's order): float64 [M, n_axes]"""
        self._against(other)
        q, r = _row_list(rows, self.n), _row_list(other_rows, other.n)
        values, vectors, mu = check_pcoa_fit(fit, r[1])
        coords = np.zeros((q[1], values.size), dtype=np.float64)
        q, r = self._source(q), other._source(r)
        self.ctx.check(self.ctx._L.dvs_pcoa_project(self.ctx._h, q, r, values.size, _lib.ptr(values, C.c_double),
                                                    _lib.ptr(vectors, C.c_double), _lib.ptr(mu, C.c_double),
                                                    _lib.ptr(coords, C.c_double)))
        return coords


class MedoidOps:
    """k-medoids as an operation of a `DeviceSide`, which inherits it: `DeviceSide.kmedoids`.  In a base class of its
    own as `OrdinationOps` is; more poisoned-block cases are in tests/test_gpu_kmedoids.py."""

    def kmedoids(self, n_medoids: int, *, init="build", max_swaps: int = 300) -> "KMedoids":
        """k-medoids of the distances (`KMedoids`), the N x N matrix written and only read in HBM.  init: "build"
        (PAM's BUILD), "maxmin" (the first n_medoids farthest-first picks from row 0, `maxmin`, as the initial
        medoids) or the initial medoids themselves, n_medoids distinct rows"""
        k, kind, rows, max_swaps = check_kmedoids_args(self.n, n_medoids, init, max_swaps)
        if kind == "maxmin":
            rows = self.maxmin(k, seeds=(0,)).picks.astype(np.uint32)
            if rows.size != k:
                raise ValueError(f"farthest-first selection found only {rows.size} of {k} initial medoids")
        return run_kmedoids(self.ctx, self.n, self._source(), k, rows, max_swaps)


class GroupOps:
    """PERMANOVA as an operation of a `DeviceSide`, which inherits it: `DeviceSide.permanova`.  In a base class of its
    own as `OrdinationOps` is; more poisoned-block cases are in tests/test_gpu_permanova.py."""

    def permanova(self, grouping, *, permutations: int = 999, seed=None, strata=None) -> "PERMANOVA":
        """PERMANOVA of `grouping` over the distances (`PERMANOVA`), the N x N matrix written and only read in HBM; the
        arguments as `permanova`"""
        labels, n_groups, perms = check_permanova_args(self.n, grouping, permutations, seed, strata)
        return run_permanova(self.ctx, self.n, self._source(), labels, n_groups, perms)


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
    """min_samples as `SpanningOps.mst` takes it: ValueError unless an integer in 1 .. min(MIN_SAMPLES_MAX, n)"""
    if isinstance(min_samples, bool) or not isinstance(min_samples, (int, np.integer)):
        raise ValueError(f"min_samples must be an integer, not {min_samples!r}")
    if min_samples < 1 or min_samples > MIN_SAMPLES_MAX:
        raise ValueError(f"min_samples = {min_samples}: between 1 and {MIN_SAMPLES_MAX}")
    if min_samples > n:
        raise ValueError(f"min_samples = {min_samples} of {n} rows: no row has that many cells")
    return int(min_samples)


def run_mst(ctx: engine.Context | None, n: int, src: _lib.Source | None, core: np.ndarray | None = None) -> MST:
    """dvs_mst over the n rows of `src` (not looked at for n == 0) with the checked core vector -> MST"""
    edges = np.zeros(2 * max(n - 1, 0), dtype=np.uint32)
    weights = np.zeros(max(n - 1, 0), dtype=np.float64)
    count, rounds = C.c_uint32(0), C.c_uint32(0)
    if n:
        ctx = ctx or engine.default_context()
        ctx.check(ctx._L.dvs_mst(ctx._h, src, _lib.ptr(core, C.c_double), _lib.ptr(edges, C.c_uint32),
                                 _lib.ptr(weights, C.c_double), C.byref(count), C.byref(rounds)))
    m = int(count.value)
    return MST(edges[:2 * m].astype(np.int64).reshape(m, 2), weights[:m].copy(), int(n), int(rounds.value))


class SpanningOps:
    """The minimum spanning tree as an operation of a `DeviceSide`, which inherits it: `DeviceSide.mst`.  In a base
    class of its own as `OrdinationOps` is; more poisoned-block cases are in tests/test_gpu_mst.py."""

    def mst(self, rows=None, *, min_samples: int | None = None, core=None) -> "MST":
        """the minimum spanning tree (`MST`) of the distances of this side's `rows` (None: all), strip by strip: the
        N x N matrix never exists.  core: one distance per row, the weights become max(d(i, j), core[i], core[j]) (mutual
        reachability); or min_samples = m (1 .. MIN_SAMPLES_MAX): core[i] the m-th smallest cell of row i, its own cell
        included (sklearn's HDBSCAN convention; `nearest` over the same rows) -- ValueError for a row with fewer
        than m cells that are not NaN"""
        if min_samples is not None and core is not None:
            raise ValueError("mst takes at most one of min_samples and core")
        listed = _row_list(rows, self.n)
        if min_samples is not None:
            m = check_min_samples(min_samples, listed[1])
            idx, dist = self.nearest(self, m, rows, rows)
            short = idx[:, m - 1] < 0
            if short.any():
                raise ValueError(f"row {int(np.argmax(short))} has fewer than min_samples = {m} distances that are not NaN")
            core = dist[:, m - 1]
        return run_mst(self.ctx, listed[1], self._source(listed), check_core(core, listed[1]))


class DeviceSide(OrdinationOps, MedoidOps, SpanningOps, GroupOps):
    """What a distance mode keeps in HBM of one batch -- its `Sketches` (mash) or its count matrix (euclidean, jsd) --
    together with the mode: every operation over "the distances of a collection", whatever the mode.  `device_side`
    makes one that owns its handle; DeviceSide(handle, mode) wraps a handle of the caller's, which close() then leaves
    alone.  Every method checks its arguments before it touches the handle; what the results hold is told where the
    public functions of each operation are.  A new operation over distances is one C entry and one method."""

    MODE_NAMES = ("mash", "euclidean", "jsd")  # in the order of _lib.SRC_MASH, SRC_EUCLIDEAN, SRC_JSD

    def __init__(self, handle, mode: str, *, owns: bool = False):
        if mode not in self.MODE_NAMES:
            raise ValueError(f"Unexpected distance {mode!r}.")
        self.handle, self.mode, self._owns = handle, mode, owns

    @property
    def ctx(self):
        return self.handle.ctx

    @property
    def n(self) -> int:
        return self.handle.n if self.mode == "mash" else self.handle.nrows

    def close(self):
        """frees the handle if this side owns it; once, however often it is called"""
        if self._owns:
            self._owns = False
            self.handle.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _source(self, listed=None) -> _lib.Source:
        """this side as the C entries take it: the rows `listed` -- what `_row_list` made of a caller's list -- or all"""
        rr, n = listed or (None, self.n)
        mash = {"k": self.handle.k, "sketch_size": self.handle.sketch_size_u32} if self.mode == "mash" else {}
        return make_source(self.MODE_NAMES.index(self.mode), self.handle._h, n, rr, **mash)

    def _against(self, other: "DeviceSide"):
        if other.mode != self.mode:
            raise ValueError(f"a side of mode {self.mode!r} against one of mode {other.mode!r}")
        if self.mode == "mash" and (other.handle.k != self.handle.k or other.handle.sketch_size != self.handle.sketch_size):
            raise ValueError(f"sketches of k = {self.handle.k}, sketch size {self.handle.sketch_size} against "
                             f"k = {other.handle.k}, sketch size {other.handle.sketch_size}")

    def distances(self) -> np.ndarray:
        """the symmetric n x n matrix of the distances, float64"""
        dist = np.zeros((self.n, self.n), dtype=np.float64)
        self.ctx.check(self.ctx._L.dvs_distances(self.ctx._h, self._source(), _lib.ptr(dist, C.c_double)))
        return dist

    def linkage(self, method: str = "average") -> np.ndarray:
        """scipy's linkage matrix Z of `method` (LINKAGE_METHODS), the N x N matrix written and read in HBM"""
        code = linkage_method_code(method)
        return run_linkage(self.ctx, self.n, self._source(), code)

    def nj(self) -> "NJTree":
        """the neighbour-joining tree, the N x N matrix left in HBM"""
        return run_nj(self.ctx, self.n, self._source())

    def cross_distances(self, other: "DeviceSide", rows=None, other_rows=None) -> np.ndarray:
        """this side's `rows` (None: all) against `other`'s `other_rows`: float64 [M, N], the cells of `distances`"""
        self._against(other)
        q, r = _row_list(rows, self.n), _row_list(other_rows, other.n)
        dist = np.zeros((q[1], r[1]), dtype=np.float64)
        q, r = self._source(q), other._source(r)
        self.ctx.check(self.ctx._L.dvs_cross_distances(self.ctx._h, q, r, _lib.ptr(dist, C.c_double)))
        return dist

    def nearest(self, other: "DeviceSide", n_nearest: int = 1, rows=None, other_rows=None):
        """the n_nearest rows of `other` nearest to each of this side's -> (int64 [M, n_nearest] positions into
        other_rows with -1 for an empty slot, float64 [M, n_nearest])"""
        self._against(other)
        q, r = _row_list(rows, self.n), _row_list(other_rows, other.n)
        kk = check_n_nearest(n_nearest, r[1])
        idx = np.zeros((q[1], kk), dtype=np.uint32)
        dist = np.zeros((q[1], kk), dtype=np.float64)
        q, r = self._source(q), other._source(r)
        self.ctx.check(self.ctx._L.dvs_nearest(self.ctx._h, q, r, kk, _lib.ptr(idx, C.c_uint32), _lib.ptr(dist, C.c_double)))
        out = idx.astype(np.int64)
        out[idx == _U32_MAX] = -1
        return out, dist

    def cluster_scores(self, labels, rows=None) -> "ClusterScores":
        """the scores of a labelling of this side's `rows` (None: all; labels[i] belongs to rows[i])"""
        listed = _row_list(rows, self.n)
        return _run_cluster_scores(self.ctx, check_labels(labels, listed[1]), self._source(listed))

    def cophenet(self, Z, rows=None, matrix: bool = False) -> "CopheneticScores":
        """the cophenetic correlation of Z with the distances of this side's `rows` (None: all; leaf i is rows[i])"""
        listed = _row_list(rows, self.n)
        pairs, heights = check_linkage_matrix(Z, listed[1])
        return _run_cophenet(self.ctx, listed[1], pairs, heights, matrix, self._source(listed))

    def maxmin(self, n_select: int | None = None, *, seeds=(0,), min_distance: float | None = None) -> "MaxMin":
        """farthest-first selection among this side's rows, a row of distances per pick"""
        args = check_maxmin_args(self.n, n_select, seeds, min_distance)
        return _run_maxmin(self.ctx, self.n, *args, self._source())

    def within(self, other: "DeviceSide", radius, rows=None, other_rows=None, *, skip_self: bool = False,
               max_pairs: int | None = None) -> "Neighbours":
        """for each of this side's `rows` (None: all) the rows of `other` (positions into other_rows, or rows) at a
        distance <= radius, in ascending position; skip_self: row i against position i is left out (both sides list
        the same rows); max_pairs: NotImplementedError once more pairs than that are found"""
        radius = check_radius(radius)
        limit = check_max_pairs(max_pairs)
        self._against(other)
        q, r = _row_list(rows, self.n), _row_list(other_rows, other.n)
        return _run_within(self.ctx, self._source(q), other._source(r), radius, _lib.WITHIN_SKIP_SELF if skip_self else 0, limit)

    def threshold_clusters(self, radius, rows=None) -> "ThresholdClusters":
        """the groups that "distance <= radius" makes of this side's `rows` (None: all): connected components"""
        radius = check_radius(radius)
        listed = _row_list(rows, self.n)
        return _run_threshold_clusters(self.ctx, listed[1], self._source(listed), radius)


CANONICAL_MASH = "Canonical count rows should only be specified for the jsd and euclidean distances (mash: mash_canonical)."


def device_side(seqs, distance_mode: str, *args, ctx: engine.Context | None = None, canonical: bool = False) -> DeviceSide:
    """what a distance mode keeps in HBM of a batch, made once: a `DeviceSide` that owns its Sketches (mash) or its
    count matrix (euclidean, jsd); args: mode_args(...).  canonical (euclidean, jsd; four states): the count rows folded
    onto the canonical k-mer bins (`engine.CountMatrix.canonical`), so that the distances do not tell a sequence from its
    reverse complement; ValueError for mash, whose sketches have mash_canonical"""
    if distance_mode not in DeviceSide.MODE_NAMES:
        raise ValueError(f"Unexpected distance {distance_mode!r}.")
    if distance_mode == "mash":
        if canonical:
            raise ValueError(CANONICAL_MASH)
        return DeviceSide(Sketches(seqs, *args, ctx=ctx), distance_mode, owns=True)
    fold = {"canonical": True} if canonical else {}
    return DeviceSide((ctx or engine.default_context()).build_matrix(seqs, *args, **fold), distance_mode, owns=True)


def _count_side(m: "engine.CountMatrix", mode: str) -> DeviceSide:
    """a count matrix of the caller's as a `DeviceSide` that does not own it"""
    if mode not in ("jsd", "euclidean"):
        raise ValueError(f"Unexpected distance {mode!r} between the rows of count matrices: 'jsd' or 'euclidean'.")
    return DeviceSide(m, mode)


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


def run_nj(ctx: engine.Context | None, n: int, src: _lib.Source) -> NJTree:
    """dvs_nj over `src` for n leaves -> NJTree; ValueError before any device work when n < 3"""
    if n < 3:
        raise ValueError("need at least three sequences for a neighbour-joining tree")
    ctx = ctx or engine.default_context()
    joins, lengths = nj_outputs(n)
    ctx.check(ctx._L.dvs_nj(ctx._h, src, _lib.ptr(joins, C.c_uint32), _lib.ptr(lengths, C.c_double)))
    return nj_tree_of(joins, lengths)


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


# a ctree distance mode -> (its N x N distances, its tree): both take (seqs, *mode_args(...)), the tree also method=
MODES = {"mash": (mash_distances, mash_linkage), "euclidean": (euclidean_distances, euclidean_linkage),
         "jsd": (jsd_distances, jsd_linkage)}


def mode_args(distance_mode: str, k: int, sketch_size, num_states: int, mash_canonical: bool) -> tuple:
    """what either function of MODES[distance_mode] takes behind the sequences"""
    if distance_mode == "mash":
        return k, int(sketch_size), num_states, mash_canonical
    return k, num_states


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


def check_mode_args(distance_mode: str, sketch_size, mash_canonical: bool, canonical: bool = False) -> None:
    """the argument checks of cluster.ctree for a distance mode, with its messages; canonical: the count rows of the jsd
    and euclidean modes folded onto the canonical k-mer bins (`device_side`)"""
    if distance_mode not in CROSS_MODES:
        raise ValueError(f"Unexpected distance {distance_mode!r}.")
    if distance_mode == "mash" and sketch_size is None:
        raise ValueError("Expected sketch size for mash distance measure.")
    if distance_mode != "mash" and sketch_size is not None:
        raise ValueError("Sketch size should only be specified for the mash distance.")
    if distance_mode != "mash" and mash_canonical:
        raise ValueError("Canonical kmers should only be specified for the mash distance.")
    if distance_mode == "mash" and canonical:
        raise ValueError(CANONICAL_MASH)


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


def _run_cluster_scores(ctx, lab: np.ndarray, src: _lib.Source | None) -> ClusterScores:
    """dvs_cluster_scores over `src` (not looked at for an empty labelling) -> ClusterScores; the means per cluster and
    overall from the n silhouettes here"""
    n = lab.size
    k = int(lab.max()) + 1 if n else 0
    within, a, b, sil = (np.zeros(n, dtype=np.float64) for _ in range(4))
    nb = np.zeros(n, dtype=np.uint32)
    med = np.zeros(k, dtype=np.uint32)
    if n:
        ctx.check(ctx._L.dvs_cluster_scores(ctx._h, src, _lib.ptr(lab, C.c_uint32), k, _lib.ptr(within, C.c_double),
                                            _lib.ptr(a, C.c_double), _lib.ptr(b, C.c_double), _lib.ptr(nb, C.c_uint32),
                                            _lib.ptr(sil, C.c_double), _lib.ptr(med, C.c_uint32)))
    neighbour, medoids = nb.astype(np.int64), med.astype(np.int64)
    neighbour[nb == _U32_MAX] = -1
    medoids[med == _U32_MAX] = -1
    sizes = np.bincount(lab, minlength=k).astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        per_cluster = np.bincount(lab, weights=sil, minlength=k) / sizes
    return ClusterScores(lab.astype(np.int64), within, a, b, neighbour, sil, sizes, medoids, per_cluster,
                         float(sil.mean()) if n else float("nan"))


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
        return _run_cluster_scores(ctx, lab, None)
    with device_side(seqs, distance_mode, *mode_args(distance_mode, k, sketch_size, num_states, mash_canonical), ctx=ctx,
                     canonical=canonical) as dev:
        return dev.cluster_scores(lab)


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


def _run_cophenet(ctx, n: int, pairs, heights, matrix: bool, src: _lib.Source) -> CopheneticScores:
    """dvs_cophenet over the n rows of `src` -> CopheneticScores"""
    corr = C.c_double(float("nan"))
    sums = np.zeros((5, n), dtype=np.float64)
    coph = np.zeros((n, n), dtype=np.float64) if matrix else None
    ctx.check(ctx._L.dvs_cophenet(ctx._h, src, _lib.ptr(pairs, C.c_uint32), _lib.ptr(heights, C.c_double),
                                  C.byref(corr), _lib.ptr(sums, C.c_double), _lib.ptr(coph, C.c_double)))
    return CopheneticScores(float(corr.value), sums, coph)


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


def _run_maxmin(ctx, n: int, n_select: int, seeds: np.ndarray, use_min: int, min_distance: float, src: _lib.Source) -> MaxMin:
    """dvs_maxmin over rows 0 .. n - 1 of `src` -> MaxMin"""
    ctx = ctx or engine.default_context()
    picks = np.zeros(n_select, dtype=np.uint32)
    radius = np.zeros(n_select, dtype=np.float64)
    owner = np.zeros(n, dtype=np.uint32)
    dist = np.zeros(n, dtype=np.float64)
    count, cover = C.c_uint32(0), C.c_double(0.0)
    ctx.check(ctx._L.dvs_maxmin(ctx._h, src, _lib.ptr(seeds, C.c_uint32), seeds.size, n_select, use_min, min_distance,
                                _lib.ptr(picks, C.c_uint32), _lib.ptr(radius, C.c_double), C.byref(count),
                                _lib.ptr(owner, C.c_uint32), _lib.ptr(dist, C.c_double), C.byref(cover)))
    own = owner.astype(np.int64)
    own[owner == _U32_MAX] = -1
    m = int(count.value)
    return MaxMin(picks[:m].astype(np.int64), radius[:m].copy(), own, dist, float(cover.value))


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


def _run_within(ctx, q: _lib.Source, r: _lib.Source | None, radius: float, flags: int, max_pairs: int) -> Neighbours:
    """dvs_within of `q` against `r` (None: a caller's matrix against itself) -> Neighbours; the dvs_pairs is copied out
    and freed"""
    ctx = ctx or engine.default_context()
    L = ctx._L
    h = C.c_void_p()
    ctx.check(L.dvs_within(ctx._h, q, r, radius, flags, max_pairs, C.byref(h)))
    try:
        rows, pairs = C.c_uint32(), C.c_uint64()
        _lib.raise_for(L.dvs_pairs_info(h, C.byref(rows), C.byref(pairs)), None)
        row_start = np.zeros(rows.value + 1, dtype=np.uint64)
        col = np.zeros(pairs.value, dtype=np.uint32)
        dist = np.zeros(pairs.value, dtype=np.float64)
        _lib.raise_for(L.dvs_pairs_get(h, _lib.ptr(row_start, C.c_uint64), _lib.ptr(col, C.c_uint32),
                                       _lib.ptr(dist, C.c_double)), None)
    finally:
        L.dvs_pairs_destroy(h)
    return Neighbours(row_start.astype(np.int64), col.astype(np.int64), dist)


def _run_threshold_clusters(ctx, n: int, src: _lib.Source | None, radius: float) -> ThresholdClusters:
    """dvs_threshold_clusters over the n rows of `src` (not looked at for n == 0) -> ThresholdClusters"""
    labels = np.zeros(n, dtype=np.uint32)
    count = C.c_uint32(0)
    if n:
        ctx = ctx or engine.default_context()
        ctx.check(ctx._L.dvs_threshold_clusters(ctx._h, src, radius, _lib.ptr(labels, C.c_uint32), C.byref(count)))
    k = int(count.value)
    return ThresholdClusters(labels.astype(np.int64), k, np.bincount(labels, minlength=k).astype(np.int64))


def matrix_within(q: "engine.CountMatrix", r: "engine.CountMatrix", radius, mode: str = "jsd", q_rows=None, r_rows=None, *,
                  skip_self: bool = False, max_pairs: int | None = None) -> Neighbours:
    """for every row q_rows of q (None: all) the rows r_rows of r at a `mode` ("jsd", "euclidean") distance <= radius
    (`Neighbours`): the cells of `matrix_cross_distances(q, r, mode, q_rows, r_rows)`, compacted on the device strip by
    strip -- only the pairs listed cross to the host.  skip_self: row i against position i is left out (q_rows and
    r_rows name the same rows of one matrix)."""
    check_radius(radius)
    return _count_side(q, mode).within(_count_side(r, mode), radius, q_rows, r_rows, skip_self=skip_self, max_pairs=max_pairs)


def matrix_threshold_clusters(m: "engine.CountMatrix", radius, mode: str = "jsd", rows=None) -> ThresholdClusters:
    """the groups that "`mode` distance <= radius" makes of rows `rows` of m (None: all): `ThresholdClusters`, the flat
    clusters of their single-linkage tree cut at height radius, without the n x n matrix and without the tree"""
    check_radius(radius)
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
        return _run_threshold_clusters(ctx, 0, None, radius)
    with device_side(seqs, distance_mode, *mode_args(distance_mode, k, sketch_size, num_states, mash_canonical), ctx=ctx,
                     canonical=canonical) as dev:
        return dev.threshold_clusters(radius)


# ---- the minimum spanning tree: single linkage without the matrix (`MST`, `SpanningOps`)

def matrix_mst(m: "engine.CountMatrix", mode: str = "jsd", rows=None, *, min_samples: int | None = None, core=None) -> MST:
    """the minimum spanning tree (`MST`) of the `mode` ("jsd", "euclidean") distances of rows `rows` of m (None: all),
    a Boruvka round per pass over the strips: the n x n matrix never exists.  A row without a valid k-mer (NaN distances)
    is a tree of its own.  min_samples, core: as `SpanningOps.mst` takes them (mutual reachability)."""
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
        return run_mst(ctx, 0, None)
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


def run_pcoa(ctx: engine.Context | None, n: int, src: _lib.Source, n_axes: int, tol: float, max_basis: int,
             strict: bool = True) -> PCoA:
    """dvs_pcoa over `src` for n rows (the arguments as `check_pcoa_args` returns them) -> PCoA.  strict: RuntimeError,
    naming the worst residual, unless every axis converged; strict=False returns what the basis gave, `converged` False"""
    ctx = ctx or engine.default_context()
    params = _lib.PcoaParams(n_axes, max_basis, tol)
    info = _lib.PcoaInfo()
    values, residuals = np.zeros(n_axes, dtype=np.float64), np.zeros(n_axes, dtype=np.float64)
    vectors, mu = np.zeros((n, n_axes), dtype=np.float64), np.zeros(n, dtype=np.float64)
    ctx.check(ctx._L.dvs_pcoa(ctx._h, src, C.byref(params), _lib.ptr(values, C.c_double), _lib.ptr(vectors, C.c_double),
                              _lib.ptr(residuals, C.c_double), _lib.ptr(mu, C.c_double), C.byref(info)))
    converged = info.converged == n_axes
    if strict and not converged:
        worst = int(np.argmax(residuals))
        raise RuntimeError(f"principal coordinates: {n_axes - info.converged} of {n_axes} axes did not converge in a basis of "
                           f"{info.basis} columns ({info.steps} steps); the worst residual, axis {worst}, is "
                           f"{residuals[worst]:.3g} against tol * lambda_1 = {tol * max(values[0], 0.0):.3g} (a spectrum "
                           "without gaps is a property of the data: raise max_basis or tol, or pass strict=False)")
    pos = values > 0.0
    coordinates = np.where(pos, vectors * np.sqrt(np.where(pos, values, 0.0)), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        proportion = values / info.trace
    return PCoA(values, vectors, coordinates, proportion, residuals, mu, float(info.trace), bool(converged), int(info.basis),
                int(info.steps))


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


def run_kmedoids(ctx: engine.Context | None, n: int, src: _lib.Source, k: int, rows: np.ndarray | None,
                 max_swaps: int) -> KMedoids:
    """dvs_kmedoids over `src` for n rows -> KMedoids; rows: the initial medoids (uint32 [k]), None for BUILD"""
    ctx = ctx or engine.default_context()
    params = _lib.KmedoidsParams(k, _lib.KMEDOIDS_INIT_BUILD if rows is None else _lib.KMEDOIDS_INIT_GIVEN, max_swaps, 0)
    info = _lib.KmedoidsInfo()
    medoids = np.zeros(k, dtype=np.uint32) if rows is None else np.array(rows, dtype=np.uint32)
    labels = np.zeros(n, dtype=np.uint32)
    dist, second = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64)
    swaps = np.zeros((max(max_swaps, 1), 2), dtype=np.uint32)
    td = np.zeros(max_swaps + 1, dtype=np.float64)
    ctx.check(ctx._L.dvs_kmedoids(ctx._h, src, C.byref(params), _lib.ptr(medoids, C.c_uint32), _lib.ptr(labels, C.c_uint32),
                                  _lib.ptr(dist, C.c_double), _lib.ptr(second, C.c_double), _lib.ptr(swaps, C.c_uint32),
                                  _lib.ptr(td, C.c_double), C.byref(info)))
    m = int(info.n_swaps)
    return KMedoids(medoids.astype(np.int64), labels.astype(np.int64), dist, second, swaps[:m].astype(np.int64),
                    td[:m + 1].copy(), int(info.stop), int(info.passes))


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


def run_permanova(ctx: engine.Context | None, n: int, src: _lib.Source, labels: np.ndarray, n_groups: int,
                  perms: np.ndarray) -> PERMANOVA:
    """dvs_permanova over `src` for n rows with the checked labels and label vectors -> PERMANOVA"""
    ctx = ctx or engine.default_context()
    n_perm = int(perms.shape[0])
    perms = np.ascontiguousarray(perms, dtype=np.uint32)
    ss_total = C.c_double(0.0)
    ss_within = np.zeros(n_perm + 1, dtype=np.float64)
    group_ss = np.zeros(n_groups, dtype=np.float64)
    info = _lib.PermanovaInfo()
    ctx.check(ctx._L.dvs_permanova(ctx._h, src, _lib.ptr(labels, C.c_uint32), n_groups,
                                   _lib.ptr(perms, C.c_uint32) if n_perm else None, n_perm, C.byref(ss_total),
                                   _lib.ptr(ss_within, C.c_double), _lib.ptr(group_ss, C.c_double), C.byref(info)))
    ssa, f, r2 = permanova_statistics(n, n_groups, ss_total.value, ss_within)
    p_value = (1.0 + int(info.n_le)) / (1.0 + n_perm) if n_perm else float("nan")
    return PERMANOVA(float(f[0]), p_value, float(r2[0]), float(ss_total.value), float(ss_within[0]), float(ssa[0]), group_ss,
                     np.bincount(labels, minlength=n_groups).astype(np.int64), f[1:].copy(), n_perm)


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
        return run_permanova(dev.ctx, dev.n, dev._source(), *checked)


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
