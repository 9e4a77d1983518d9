"""What a distance mode keeps in HBM of one batch: `Sketches` (the handle of the mash mode; the count-matrix modes'
is engine.CountMatrix) and `DeviceSide`, either handle together with its mode and every operation as a method.  A
method checks its arguments (`_results`) and makes its call (`_calls`); the only C calls made here are those by which
`Sketches` manages its own handle."""

from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib, engine
from ._calls import (make_source, run_cluster_scores, run_cophenet, run_cross_distances, run_distances, run_kmedoids,
                     run_linkage, run_maxmin, run_mst, run_nearest, run_nj, run_pcoa, run_pcoa_project, run_permanova,
                     run_threshold_clusters, run_within)
from ._results import (_U32_MAX, CANONICAL_MASH, _dist_out, _row_list, _sketch_stride, check_core, check_kmedoids_args,
                       check_labels, check_linkage_matrix, check_max_pairs, check_maxmin_args, check_min_samples,
                       check_n_nearest, check_pcoa_args, check_pcoa_fit, check_permanova_args, check_radius,
                       linkage_method_code)  # (the result types stand in annotations only, as strings)

__all__ = ["Sketches", "DeviceSide", "device_side"]  # the public names of this layer, which the package re-exports


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

    @property
    def side(self) -> "DeviceSide":
        """these sketches as a `DeviceSide` of the mode "mash" that does not own them"""
        return DeviceSide(self, "mash")

    def linkage(self, method: str = "average") -> np.ndarray:
        """scipy's linkage matrix Z of `method` (LINKAGE_METHODS) over the mash distances of every pair: the N x N
        matrix is written and read in HBM (dvs_linkage); ZeroDivisionError as `distances`"""
        return self.side.linkage(method)

    def cross_distances(self, other: "Sketches", rows=None, other_rows=None) -> np.ndarray:
        """the mash distances of this set's sketches `rows` (None: all) against `other`'s `other_rows`: float64 [M, N],
        every cell the bits `distances` gives the same two sketches (dvs_cross_distances);
        ZeroDivisionError as `distances`"""
        return self.side.cross_distances(DeviceSide(other, "mash"), rows, other_rows)

    def nearest(self, other: "Sketches", n_nearest: int = 1, rows=None, other_rows=None):
        """the n_nearest sketches of `other` (positions into other_rows, or rows) nearest to each of this set's, nearest
        first, a tie to the lower position: (int64 [M, n_nearest], -1 in a slot without a reference; float64 distances,
        NaN there) (dvs_nearest)"""
        return self.side.nearest(DeviceSide(other, "mash"), n_nearest, rows, other_rows)

    def cluster_scores(self, labels, rows=None) -> "ClusterScores":
        """the scores of a labelling (`ClusterScores`) of this set's sketches `rows` (None: all; labels[i] belongs to
        rows[i]) over their mash distances, computed strip by strip (dvs_cluster_scores); ZeroDivisionError
        as `distances`"""
        return self.side.cluster_scores(labels, rows)

    def cophenet(self, Z, rows=None, matrix: bool = False) -> "CopheneticScores":
        """the cophenetic correlation (`CopheneticScores`) of the linkage matrix Z with the mash distances of this set's
        sketches `rows` (None: all; leaf i of Z is rows[i]), computed strip by strip (dvs_cophenet);
        ZeroDivisionError as `cluster_scores`"""
        return self.side.cophenet(Z, rows, matrix)

    def maxmin(self, n_select: int | None = None, *, seeds=(0,), min_distance: float | None = None) -> "MaxMin":
        """farthest-first selection (`MaxMin`) among this set's sketches by their mash distances, a row of distances
        per pick (dvs_maxmin); ZeroDivisionError where a pair the traversal visits has two empty sketches"""
        return self.side.maxmin(n_select, seeds=seeds, min_distance=min_distance)

    def kmedoids(self, n_medoids: int, *, init="build", max_swaps: int = 300) -> "KMedoids":
        """k-medoids (`KMedoids`) of this set's sketches over their mash distances, the N x N matrix written and only
        read in HBM (dvs_kmedoids); ZeroDivisionError as `distances`"""
        return self.side.kmedoids(n_medoids, init=init, max_swaps=max_swaps)

    def permanova(self, grouping, *, permutations: int = 999, seed=None, strata=None) -> "PERMANOVA":
        """PERMANOVA (`PERMANOVA`) of a grouping of this set's sketches over their mash distances, the N x N matrix
        written and only read in HBM (dvs_permanova); ZeroDivisionError as `distances`"""
        return self.side.permanova(grouping, permutations=permutations, seed=seed, strata=strata)

    def within(self, other: "Sketches", radius, rows=None, other_rows=None, *, skip_self: bool = False,
               max_pairs: int | None = None) -> "Neighbours":
        """for each of this set's sketches `rows` the sketches of `other` at a mash distance <= radius (`Neighbours`:
        the cells of `cross_distances`, compacted on the device; dvs_within); ZeroDivisionError as
        `cross_distances`"""
        return self.side.within(DeviceSide(other, "mash"), radius, rows, other_rows, skip_self=skip_self, max_pairs=max_pairs)

    def threshold_clusters(self, radius, rows=None) -> "ThresholdClusters":
        """the groups that "mash distance <= radius" makes of this set's sketches `rows` (`ThresholdClusters`;
        dvs_threshold_clusters); ZeroDivisionError as `cluster_scores`"""
        return self.side.threshold_clusters(radius, rows)


class DeviceSide:
    """What a distance mode keeps in HBM of one batch -- its `Sketches` (mash) or its count matrix (euclidean, jsd) --
    together with the mode: every operation over "the distances of a collection", whatever the mode.  `device_side`
    makes one that owns its handle; DeviceSide(handle, mode) wraps a handle of the caller's, which close() then leaves
    alone.  Every method checks its arguments before it touches the handle; what the results hold is told where the
    public functions of each operation are.  A new operation over distances is one C entry, its `run_` function and one
    method here."""

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
        return run_distances(self.ctx, self._source())

    def linkage(self, method: str = "average") -> np.ndarray:
        """scipy's linkage matrix Z of `method` (LINKAGE_METHODS), the N x N matrix written and read in HBM"""
        code = linkage_method_code(method)
        return run_linkage(self.ctx, self._source(), code)

    def nj(self) -> "NJTree":
        """the neighbour-joining tree, the N x N matrix left in HBM"""
        return run_nj(self.ctx, self._source())

    def cross_distances(self, other: "DeviceSide", rows=None, other_rows=None) -> np.ndarray:
        """this side's `rows` (None: all) against `other`'s `other_rows`: float64 [M, N], the cells of `distances`"""
        self._against(other)
        q, r = _row_list(rows, self.n), _row_list(other_rows, other.n)
        return run_cross_distances(self.ctx, self._source(q), other._source(r))

    def nearest(self, other: "DeviceSide", n_nearest: int = 1, rows=None, other_rows=None):
        """the n_nearest rows of `other` nearest to each of this side's -> (int64 [M, n_nearest] positions into
        other_rows with -1 for an empty slot, float64 [M, n_nearest])"""
        self._against(other)
        q, r = _row_list(rows, self.n), _row_list(other_rows, other.n)
        kk = check_n_nearest(n_nearest, r[1])
        return run_nearest(self.ctx, self._source(q), other._source(r), kk)

    def cluster_scores(self, labels, rows=None) -> "ClusterScores":
        """the scores of a labelling of this side's `rows` (None: all; labels[i] belongs to rows[i])"""
        listed = _row_list(rows, self.n)
        lab = check_labels(labels, listed[1])
        return run_cluster_scores(self.ctx, self._source(listed), lab)

    def cophenet(self, Z, rows=None, matrix: bool = False) -> "CopheneticScores":
        """the cophenetic correlation of Z with the distances of this side's `rows` (None: all; leaf i is rows[i])"""
        listed = _row_list(rows, self.n)
        pairs, heights = check_linkage_matrix(Z, listed[1])
        return run_cophenet(self.ctx, self._source(listed), pairs, heights, matrix)

    def maxmin(self, n_select: int | None = None, *, seeds=(0,), min_distance: float | None = None) -> "MaxMin":
        """farthest-first selection among this side's rows, a row of distances per pick"""
        args = check_maxmin_args(self.n, n_select, seeds, min_distance)
        return run_maxmin(self.ctx, self._source(), *args)

    def within(self, other: "DeviceSide", radius, rows=None, other_rows=None, *, skip_self: bool = False,
               max_pairs: int | None = None) -> "Neighbours":
        """for each of this side's `rows` (None: all) the rows of `other` (positions into other_rows, or rows) at a
        distance <= radius, in ascending position; skip_self: row i against position i is left out (both sides list
        the same rows); max_pairs: NotImplementedError once more pairs than that are found"""
        radius = check_radius(radius)
        limit = check_max_pairs(max_pairs)
        self._against(other)
        q, r = _row_list(rows, self.n), _row_list(other_rows, other.n)
        return run_within(self.ctx, self._source(q), other._source(r), radius, _lib.WITHIN_SKIP_SELF if skip_self else 0, limit)

    def threshold_clusters(self, radius, rows=None) -> "ThresholdClusters":
        """the groups that "distance <= radius" makes of this side's `rows` (None: all): connected components"""
        radius = check_radius(radius)
        return run_threshold_clusters(self.ctx, self._source(_row_list(rows, self.n)), radius)

    def pcoa(self, n_axes: int = 3, *, tol: float = 1e-8, max_basis: int | None = None, strict: bool = True) -> "PCoA":
        """the principal coordinates of the distances (`PCoA`), the N x N matrix written and only read in HBM"""
        args = check_pcoa_args(self.n, n_axes, tol, max_basis)
        return run_pcoa(self.ctx, self._source(), *args, strict)

    def pcoa_project(self, fit: "PCoA", other: "DeviceSide", rows=None, other_rows=None) -> np.ndarray:
        """the coordinates of this side's `rows` (None: all) in the ordination `fit` of `other`'s `other_rows` (None:
        all; they are the fitted rows, in the fit's order): float64 [M, n_axes]"""
        self._against(other)
        q, r = _row_list(rows, self.n), _row_list(other_rows, other.n)
        values, vectors, mu = check_pcoa_fit(fit, r[1])
        return run_pcoa_project(self.ctx, self._source(q), other._source(r), values, vectors, mu)

    def kmedoids(self, n_medoids: int, *, init="build", max_swaps: int = 300) -> "KMedoids":
        """k-medoids of the distances (`KMedoids`), the N x N matrix written and only read in HBM.  init: "build"
        (PAM's BUILD), "maxmin" (the first n_medoids farthest-first picks from row 0, `maxmin`, as the initial
        medoids) or the initial medoids themselves, n_medoids distinct rows"""
        k, kind, rows, max_swaps = check_kmedoids_args(self.n, n_medoids, init, max_swaps)
        if kind == "maxmin":
            rows = self.maxmin(k, seeds=(0,)).picks.astype(np.uint32)
            if rows.size != k:
                raise ValueError(f"farthest-first selection found only {rows.size} of {k} initial medoids")
        return run_kmedoids(self.ctx, self._source(), k, rows, max_swaps)

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
        return run_mst(self.ctx, self._source(listed), check_core(core, listed[1]))

    def permanova(self, grouping, *, permutations: int = 999, seed=None, strata=None) -> "PERMANOVA":
        """PERMANOVA of `grouping` over the distances (`PERMANOVA`), the N x N matrix written and only read in HBM; the
        arguments as `permanova`"""
        labels, n_groups, perms = check_permanova_args(self.n, grouping, permutations, seed, strata)
        return run_permanova(self.ctx, self._source(), labels, n_groups, perms)


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
