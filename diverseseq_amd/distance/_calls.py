"""The C calls of the distance layer: `make_source`, which fills the dvs_source an entry takes, and one `run_<op>` per
operation -- run_<op>(ctx, src, the checked arguments...), or (ctx, q, r, ...) for an operation between two sides.  The
number of rows is the source's own `n`.  ctx=None becomes engine.default_context() here and nowhere above, and only
where a device call follows: an empty input returns its empty result without a context.  The arguments are those the
`check_*` functions of `_results` return; nothing is checked a second time."""

from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib, engine
from ._results import (_U32_MAX, ClusterScores, CopheneticScores, KMedoids, MaxMin, MST, Neighbours, NJTree, PCoA, PERMANOVA,
                       ThresholdClusters, _dist_out, _no_neighbours, _sketch_stride, linkage_matrix, nj_outputs, nj_tree_of,
                       permanova_statistics, tree_outputs)

# the public names of this layer, which the package re-exports
__all__ = [
    "make_source", "sketch_batch", "distances_from_sketches", "run_distances", "run_linkage", "run_nj", "run_pcoa",
    "run_kmedoids", "run_permanova", "run_cross_distances", "run_nearest", "run_pcoa_project", "run_cluster_scores",
    "run_cophenet", "run_within", "run_threshold_clusters", "run_mst", "run_maxmin",
]


def make_source(kind: int, handle, n: int, rows: np.ndarray | None = None, *, k: int = 0, sketch_size: int = 0,
                on_device: int = 0, keep=None) -> _lib.Source:
    """the dvs_source of one call: `kind` (_lib.SRC_*), the handle or matrix pointer, the `n` rows taken and their
    optional uint32 row list.  What its pointers refer to -- the row array, and `keep`, the owner of a caller's
    matrix -- lives as long as the structure does"""
    src = _lib.Source(kind, handle, _lib.ptr(rows, C.c_uint32), n, k, sketch_size, on_device)
    src._keep = (handle, rows, keep)
    return src


_NO_ROWS = make_source(_lib.SRC_GIVEN, None, 0)  # the source of an empty collection: no entry is called over it


# ---- sketches and distances of arrays on the host

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


# ---- the whole matrix: written in HBM, and copied out or left there for a tree, an ordination, a search, a test

def run_distances(ctx: engine.Context | None, src: _lib.Source) -> np.ndarray:
    """dvs_distances over `src` -> the symmetric n x n matrix, float64"""
    ctx = ctx or engine.default_context()
    dist = np.zeros((src.n, src.n), dtype=np.float64)
    ctx.check(ctx._L.dvs_distances(ctx._h, src, _lib.ptr(dist, C.c_double)))
    return dist


def run_linkage(ctx: engine.Context | None, src: _lib.Source, code: int,
                too_few: str = "need at least two sequences to build a tree") -> np.ndarray:
    """dvs_linkage over `src` with the method `code` -> Z; ValueError(too_few) before any device work for fewer than
    two leaves"""
    if src.n < 2:
        raise ValueError(too_few)
    ctx = ctx or engine.default_context()
    pairs, heights, sizes = tree_outputs(src.n)
    ctx.check(ctx._L.dvs_linkage(ctx._h, src, code, _lib.ptr(pairs, C.c_uint32), _lib.ptr(heights, C.c_double),
                                 _lib.ptr(sizes, C.c_uint32)))
    return linkage_matrix(pairs, heights, sizes)


def run_nj(ctx: engine.Context | None, src: _lib.Source) -> NJTree:
    """dvs_nj over `src` -> NJTree; ValueError before any device work for fewer than three leaves"""
    if src.n < 3:
        raise ValueError("need at least three sequences for a neighbour-joining tree")
    ctx = ctx or engine.default_context()
    joins, lengths = nj_outputs(src.n)
    ctx.check(ctx._L.dvs_nj(ctx._h, src, _lib.ptr(joins, C.c_uint32), _lib.ptr(lengths, C.c_double)))
    return nj_tree_of(joins, lengths)


def run_pcoa(ctx: engine.Context | None, src: _lib.Source, n_axes: int, tol: float, max_basis: int,
             strict: bool = True) -> PCoA:
    """dvs_pcoa over `src` (the arguments as `check_pcoa_args` returns them) -> PCoA.  strict: RuntimeError,
    naming the worst residual, unless every axis converged; strict=False returns what the basis gave, `converged` False"""
    ctx = ctx or engine.default_context()
    params = _lib.PcoaParams(n_axes, max_basis, tol)
    info = _lib.PcoaInfo()
    values, residuals = np.zeros(n_axes, dtype=np.float64), np.zeros(n_axes, dtype=np.float64)
    vectors, mu = np.zeros((src.n, n_axes), dtype=np.float64), np.zeros(src.n, dtype=np.float64)
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


def run_kmedoids(ctx: engine.Context | None, src: _lib.Source, k: int, rows: np.ndarray | None, max_swaps: int) -> KMedoids:
    """dvs_kmedoids over `src` -> KMedoids; rows: the initial medoids (uint32 [k]), None for BUILD"""
    ctx = ctx or engine.default_context()
    n = src.n
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


def run_permanova(ctx: engine.Context | None, src: _lib.Source, labels: np.ndarray, n_groups: int,
                  perms: np.ndarray) -> PERMANOVA:
    """dvs_permanova over `src` with the checked labels and label vectors -> PERMANOVA"""
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
    ssa, f, r2 = permanova_statistics(src.n, n_groups, ss_total.value, ss_within)
    p_value = (1.0 + int(info.n_le)) / (1.0 + n_perm) if n_perm else float("nan")
    return PERMANOVA(float(f[0]), p_value, float(r2[0]), float(ss_total.value), float(ss_within[0]), float(ssa[0]), group_ss,
                     np.bincount(labels, minlength=n_groups).astype(np.int64), f[1:].copy(), n_perm)


# ---- strip by strip: the distances computed a strip of rows at a time and consumed on the device

def run_cross_distances(ctx: engine.Context | None, q: _lib.Source, r: _lib.Source) -> np.ndarray:
    """dvs_cross_distances of the rows of `q` against those of `r` -> float64 [M, N]"""
    ctx = ctx or engine.default_context()
    dist = np.zeros((q.n, r.n), dtype=np.float64)
    ctx.check(ctx._L.dvs_cross_distances(ctx._h, q, r, _lib.ptr(dist, C.c_double)))
    return dist


def run_nearest(ctx: engine.Context | None, q: _lib.Source, r: _lib.Source, n_nearest: int):
    """dvs_nearest of `q` against `r` -> (int64 [M, n_nearest] positions with -1 for an empty slot, float64 [M,
    n_nearest])"""
    ctx = ctx or engine.default_context()
    idx = np.zeros((q.n, n_nearest), dtype=np.uint32)
    dist = np.zeros((q.n, n_nearest), dtype=np.float64)
    ctx.check(ctx._L.dvs_nearest(ctx._h, q, r, n_nearest, _lib.ptr(idx, C.c_uint32), _lib.ptr(dist, C.c_double)))
    out = idx.astype(np.int64)
    out[idx == _U32_MAX] = -1
    return out, dist


def run_pcoa_project(ctx: engine.Context | None, q: _lib.Source, r: _lib.Source, values: np.ndarray, vectors: np.ndarray,
                     mu: np.ndarray) -> np.ndarray:
    """dvs_pcoa_project of the rows of `q` into the fit of the rows of `r` (the tables as `check_pcoa_fit` returns
    them) -> float64 [M, n_axes]"""
    ctx = ctx or engine.default_context()
    coords = np.zeros((q.n, values.size), dtype=np.float64)
    ctx.check(ctx._L.dvs_pcoa_project(ctx._h, q, r, values.size, _lib.ptr(values, C.c_double), _lib.ptr(vectors, C.c_double),
                                      _lib.ptr(mu, C.c_double), _lib.ptr(coords, C.c_double)))
    return coords


def run_cluster_scores(ctx: engine.Context | None, src: _lib.Source, lab: np.ndarray) -> ClusterScores:
    """dvs_cluster_scores over `src` with the checked labels (no call for an empty labelling) -> ClusterScores; the
    means per cluster and overall from the n silhouettes here"""
    n = lab.size
    k = int(lab.max()) + 1 if n else 0
    within, a, b, sil = (np.zeros(n, dtype=np.float64) for _ in range(4))
    nb = np.zeros(n, dtype=np.uint32)
    med = np.zeros(k, dtype=np.uint32)
    if n:
        ctx = ctx or engine.default_context()
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


def run_cophenet(ctx: engine.Context | None, src: _lib.Source, pairs: np.ndarray, heights: np.ndarray,
                 matrix: bool) -> CopheneticScores:
    """dvs_cophenet over `src` with the checked linkage matrix -> CopheneticScores"""
    ctx = ctx or engine.default_context()
    corr = C.c_double(float("nan"))
    sums = np.zeros((5, src.n), dtype=np.float64)
    coph = np.zeros((src.n, src.n), dtype=np.float64) if matrix else None
    ctx.check(ctx._L.dvs_cophenet(ctx._h, src, _lib.ptr(pairs, C.c_uint32), _lib.ptr(heights, C.c_double),
                                  C.byref(corr), _lib.ptr(sums, C.c_double), _lib.ptr(coph, C.c_double)))
    return CopheneticScores(float(corr.value), sums, coph)


def run_within(ctx: engine.Context | None, q: _lib.Source, r: _lib.Source | None, radius: float, flags: int,
               max_pairs: int) -> Neighbours:
    """dvs_within of `q` against `r` (None: a caller's matrix against itself; no call where that matrix is empty) ->
    Neighbours; the dvs_pairs is copied out and freed"""
    if r is None and not q.n:
        return _no_neighbours(0)
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


def run_threshold_clusters(ctx: engine.Context | None, src: _lib.Source, radius: float) -> ThresholdClusters:
    """dvs_threshold_clusters over `src` (no call for no rows) -> ThresholdClusters"""
    labels = np.zeros(src.n, dtype=np.uint32)
    count = C.c_uint32(0)
    if src.n:
        ctx = ctx or engine.default_context()
        ctx.check(ctx._L.dvs_threshold_clusters(ctx._h, src, radius, _lib.ptr(labels, C.c_uint32), C.byref(count)))
    k = int(count.value)
    return ThresholdClusters(labels.astype(np.int64), k, np.bincount(labels, minlength=k).astype(np.int64))


def run_mst(ctx: engine.Context | None, src: _lib.Source, core: np.ndarray | None = None) -> MST:
    """dvs_mst over `src` (no call for no rows) with the checked core vector -> MST"""
    n = src.n
    edges = np.zeros(2 * max(n - 1, 0), dtype=np.uint32)
    weights = np.zeros(max(n - 1, 0), dtype=np.float64)
    count, rounds = C.c_uint32(0), C.c_uint32(0)
    if n:
        ctx = ctx or engine.default_context()
        ctx.check(ctx._L.dvs_mst(ctx._h, src, _lib.ptr(core, C.c_double), _lib.ptr(edges, C.c_uint32),
                                 _lib.ptr(weights, C.c_double), C.byref(count), C.byref(rounds)))
    m = int(count.value)
    return MST(edges[:2 * m].astype(np.int64).reshape(m, 2), weights[:m].copy(), int(n), int(rounds.value))


# ---- row per step: one row of distances per pick, never the matrix

def run_maxmin(ctx: engine.Context | None, src: _lib.Source, n_select: int, seeds: np.ndarray, use_min: int,
               min_distance: float) -> MaxMin:
    """dvs_maxmin over the rows of `src` (the arguments as `check_maxmin_args` returns them) -> MaxMin"""
    ctx = ctx or engine.default_context()
    picks = np.zeros(n_select, dtype=np.uint32)
    radius = np.zeros(n_select, dtype=np.float64)
    owner = np.zeros(src.n, dtype=np.uint32)
    dist = np.zeros(src.n, dtype=np.float64)
    count, cover = C.c_uint32(0), C.c_double(0.0)
    ctx.check(ctx._L.dvs_maxmin(ctx._h, src, _lib.ptr(seeds, C.c_uint32), seeds.size, n_select, use_min, min_distance,
                                _lib.ptr(picks, C.c_uint32), _lib.ptr(radius, C.c_double), C.byref(count),
                                _lib.ptr(owner, C.c_uint32), _lib.ptr(dist, C.c_double), C.byref(cover)))
    own = owner.astype(np.int64)
    own[owner == _U32_MAX] = -1
    m = int(count.value)
    return MaxMin(picks[:m].astype(np.int64), radius[:m].copy(), own, dist, float(cover.value))
