"""`dvs ctree` path: distances and the linkage tree on the GPU.

Mirrors diverse_seq/cluster.py: `make_cluster_tree` (:191-237 -- sklearn
AgglomerativeClustering(metric="precomputed", linkage="average"), children_ folded into a
nested tuple, printed without quotes) and the argument checks of `dvs_ctree.__init__`
(:113-162).  The reference hands the string to cogent3's make_tree; here it is returned as a
Newick string.  `ctree` builds the tree on the device by default (`linkage`: scipy's
nearest-neighbour chain, or for single linkage its minimum spanning tree, in one persistent
workgroup, csrc/linkage.hip, the same linkage matrix bit for bit); `tree="sklearn"` keeps the
reference's host path (`make_cluster_tree`, average linkage only).

Beyond the reference: the flat clusters of a tree (`cut_tree`: scipy's fcluster partitions, on the host), the
scores of a labelling (`cluster_scores`, csrc/clusters.hip: sums within a cluster, the nearest other cluster,
silhouettes, medoids) and both behind one call (`ctree_clusters`); how well a tree represents its distances (`cophenet`:
scipy's cophenet, the correlation reduced on the GPU by csrc/cophenet.hip's cophenet_kernel; `ctree_cophenet`,
`compare_linkages`); and the tree of additive distances, neighbour joining (`neighbor_joining`, csrc/nj.hip: an unrooted
tree with branch lengths and no molecular clock; `nj_to_newick`, `patristic`, `nj_tree`); and farthest-first selection
of representatives over a caller's own distance matrix (`maxmin`, csrc/maxmin.hip); and the pairs of a caller's matrix
within a radius (`within`), the groups they make (`threshold_clusters`: the single-linkage clusters at that height
without the tree) and, over sequences, those groups with one representative each (`dereplicate`); and the picture of a
collection's distances, principal coordinates (`pcoa` over a caller's matrix, `ordinate` over sequences, csrc/pcoa.hip;
`landmark_pcoa`: the ordination of a few thousand farthest-first landmarks with every other sequence projected into
it, for collections whose N x N matrix could never exist); and the representatives that lie closest, in total, to
everything else, k-medoids (`kmedoids` over a caller's matrix, `representatives` over sequences, csrc/kmedoids.hip;
`sampled_kmedoids`: k-medoids of farthest-first landmarks with every sequence assigned to its nearest medoid, for
collections whose N x N matrix could never exist); and whether a grouping of the rows explains the distances, PERMANOVA
(`permanova` over a caller's matrix, csrc/permanova.hip); and the tree itself for such collections, the minimum spanning tree
(`minimum_spanning_tree` over a caller's matrix, `mst_ctree` over sequences, csrc/mst.hip: Boruvka rounds over strips of
distances; `mst_linkage`, `mst_to_edges`): single linkage, and with a core vector robust single linkage, in O(N) device
memory beside one strip.
"""

from __future__ import annotations

import contextlib
import ctypes as C
import sys
from collections.abc import Sequence

import numpy as np

from . import _lib, distance, engine


def nested_tuple_tree(seq_names: Sequence[str], pairwise_distances: np.ndarray):
    """diverse_seq/cluster.py:216-230"""
    from sklearn.cluster import AgglomerativeClustering

    clustering = AgglomerativeClustering(metric="precomputed", linkage="average")
    clustering.fit(np.asarray(pairwise_distances, dtype=np.float64))
    tree = {i: seq_names[i] for i in range(len(seq_names))}
    node = len(seq_names)
    for left, right in clustering.children_:
        tree[node] = (tree.pop(int(left)), tree.pop(int(right)))
        node += 1
    return tree[node - 1]


def make_cluster_tree(seq_names: Sequence[str], pairwise_distances: np.ndarray) -> str:
    """-> Newick string of the average-linkage tree (diverse_seq/cluster.py:231-233)"""
    if len(seq_names) < 2:
        raise ValueError("need at least two sequences to build a tree")
    return str(nested_tuple_tree(seq_names, pairwise_distances)).replace("'", "") + ";"


def _caller_matrix(dist):
    """a caller's n x n distance matrix -- a square, contiguous float64 torch tensor on the GPU, or anything
    np.asarray(dist, float64) takes -> (its `_lib.Source`, of kind GIVEN, which keeps the matrix alive; n; wait); wait()
    returns once the work torch has queued on the tensor's device's current stream is done (torch's stream -> the
    library's), at once for host memory"""
    torch = sys.modules.get("torch")
    if torch is not None and isinstance(dist, torch.Tensor) and dist.is_cuda:
        if dist.dtype != torch.float64 or dist.dim() != 2 or dist.shape[0] != dist.shape[1] or not dist.is_contiguous():
            raise ValueError("a device distance matrix must be a square, contiguous float64 tensor")
        wait = lambda: torch.cuda.current_stream(dist.device).synchronize()  # noqa: E731
        n = int(dist.shape[0])
        return distance.make_source(_lib.SRC_GIVEN, dist.data_ptr(), n, on_device=1, keep=dist), n, wait
    d = np.ascontiguousarray(np.asarray(dist, dtype=np.float64))
    if d.ndim != 2 or d.shape[0] != d.shape[1]:
        raise ValueError(f"expected a square distance matrix, got shape {d.shape}")
    return distance.make_source(_lib.SRC_GIVEN, d.ctypes.data, d.shape[0], keep=d), d.shape[0], lambda: None


def linkage(dist, method: str = "average", *, ctx: engine.Context | None = None) -> np.ndarray:
    """scipy.cluster.hierarchy.linkage(dist[np.triu_indices(n, 1)], method) on the GPU -> Z, float64 [n - 1, 4] in
    scipy's layout, bit for bit, for method "single", "complete", "average", "weighted" or "ward" ("centroid" and
    "median", which scipy builds by another algorithm, raise ValueError).  Only the upper triangle counts; a NaN or
    inf anywhere raises ValueError, as sklearn's check does, and so does a negative entry above the diagonal for
    "ward".  The method and the shape are checked before any device work.

    `dist`: anything np.asarray(dist, float64) takes (left as it is), or a square, contiguous float64 torch tensor
    on the GPU, which is used as the working buffer and OVERWRITTEN.  Such a tensor must live on the context's
    device (ValueError otherwise); the call waits for the work torch has queued on that device's current stream."""
    code = distance.linkage_method_code(method)
    src, n, wait = _caller_matrix(dist)
    wait()
    return distance.run_linkage(ctx, src, code, too_few=f"Found array with {n} sample(s) while a minimum of 2 is required")


def average_linkage(dist, *, ctx: engine.Context | None = None) -> np.ndarray:
    """`linkage(dist, "average")`: what sklearn's AgglomerativeClustering(metric="precomputed", linkage="average")
    runs (its children_ is Z[:, :2]), the tree of `dvs ctree`"""
    return linkage(dist, "average", ctx=ctx)


def linkage_to_newick(names: Sequence, Z) -> str:
    """scipy linkage matrix -> the string `make_cluster_tree` prints for the same merges: a leaf is repr(name), an
    inner node "(" + left + ", " + right + ")" with Z's two children in order, every "'" dropped, ";" at the end.
    Host only and iterative (no recursion limit: a caterpillar of 5 000 leaves is fine), one "".join."""
    n = len(names)
    if n < 2:
        raise ValueError("need at least two sequences to build a tree")
    z = np.asarray(Z)
    if z.shape != (n - 1, 4):
        raise ValueError(f"a linkage matrix of {n} leaves has shape ({n - 1}, 4), not {z.shape}")
    kids = z[:, :2].astype(np.int64).tolist()
    parts = []
    stack: list = [2 * n - 2]  # node ids, and the literal pieces between them
    while stack:
        item = stack.pop()
        if isinstance(item, str):
            parts.append(item)
        elif item < n:
            parts.append(repr(names[item]).replace("'", ""))
        else:
            left, right = kids[item - n]
            stack.extend((")", right, ", ", left, "("))
    parts.append(";")
    return "".join(parts)


def ctree(seqs: dict, *, k: int = 12, sketch_size: int | None = 3000, distance_mode: str = "mash",
          mash_canonical_kmers: bool | None = None, num_states: int = 4, tree: str = "device",
          linkage: str = "average", canonical: bool = False) -> str:
    """sequences {name: uint8 codes} -> Newick string (dvs_ctree.main, cluster.py:164-188).
    Argument checks as dvs_ctree.__init__ (cluster.py:139-162).  distance_mode: the reference's "mash" and
    "euclidean", and "jsd", the Jensen-Shannon divergence of the k-mer frequencies (`distance.jsd_distances`),
    which takes the euclidean mode's arguments.  canonical (euclidean, jsd; here and in the functions over sequences
    below): the count rows folded onto the canonical k-mer bins (`distance.device_side`), so that the tree does not tell a
    sequence from its reverse complement; ValueError for mash, which has mash_canonical_kmers.

    tree="device": the distances and the tree both on the GPU, the N x N matrix never leaves HBM
    (dvs_linkage over the mode's source), the string from
    `linkage_to_newick`; `linkage`: any method the module's `linkage` function builds.  tree="sklearn": the reference's path (the matrix copied to the host, sklearn, nested
    tuples; `make_cluster_tree`), average linkage only.  Both give the same string wherever the sklearn path
    returns one; the one intended difference is a tree deeper than Python's recursion limit (e.g. a caterpillar of
    a few thousand leaves), for which the device path returns the Newick string where the sklearn path raises
    RecursionError."""
    if mash_canonical_kmers is None:
        mash_canonical_kmers = False
    distance.check_mode_args(distance_mode, sketch_size, mash_canonical_kmers, canonical)
    if tree not in ("device", "sklearn"):
        raise ValueError(f"Unexpected tree {tree!r}: 'device' or 'sklearn'.")
    distance.linkage_method_code(linkage)
    if tree == "sklearn" and linkage != "average":
        raise ValueError(f"tree='sklearn' builds average linkage only, not {linkage!r}: use tree='device'")
    names = list(seqs)
    arrays = [seqs[n] for n in names]
    distances, tree_of = distance.MODES[distance_mode]
    args = distance.mode_args(distance_mode, k, sketch_size, num_states, mash_canonical_kmers)
    fold = {"canonical": True} if canonical else {}
    if tree == "sklearn":
        return make_cluster_tree(names, distances(arrays, *args, **fold))
    return linkage_to_newick(names, tree_of(arrays, *args, method=linkage, **fold))


def neighbor_joining(dist, *, ctx: engine.Context | None = None) -> "distance.NJTree":
    """the neighbour-joining tree (canonical Saitou-Nei / Studier-Keppler, include/dvs_hip.h) of an n x n distance
    matrix, n >= 3, on the GPU -> `distance.NJTree`: unrooted, with branch lengths, the generating tree wherever the
    distances are additive.  Only the upper triangle counts (the diagonal counts as 0); a NaN or inf anywhere raises
    ValueError.  Equal Q values go to the lowest pair of slots, so the records are the same bits wherever the arithmetic
    is exact; on general input compare two results as unrooted trees.  The shape and n >= 3 are checked before any device
    work.

    `dist`: as `linkage` takes it -- anything np.asarray(dist, float64) takes (left as it is), or a square, contiguous
    float64 torch tensor on the context's device, which is the working buffer and OVERWRITTEN; the call waits for the
    work torch has queued on that device's current stream."""
    src, n, wait = _caller_matrix(dist)
    if n < 3:
        raise ValueError(f"Found array with {n} sample(s) while a minimum of 3 is required for a neighbour-joining tree")
    wait()
    return distance.run_nj(ctx, src)


def nj_to_newick(names: Sequence, tree, *, lengths: bool = True) -> str:
    """a neighbour-joining tree -> Newick, e.g. "(a:0.1, b:0.2, (c:0.3, d:0.4):0.5);": the three children of the last
    record at the top level, a record's children in its order, a leaf as `linkage_to_newick` writes it (repr(name), every
    "'" dropped), every branch length as repr(float) so that it reads back to the same bits; lengths=False: the bare
    topology.  Host only and iterative (no recursion limit), one "".join."""
    n, joins, lens = distance.nj_inputs(tree)
    if len(names) != n:
        raise ValueError(f"{len(names)} names for a tree of {n} leaves")
    kids = joins.reshape(-1, 3).tolist()
    lens = lens.reshape(-1, 3).tolist()
    parts = []
    stack: list = [(2 * n - 3, None)]  # (node id, the length above it) and the literal pieces between them
    while stack:
        item = stack.pop()
        if isinstance(item, str):
            parts.append(item)
            continue
        v, above = item
        tail = f":{float(above)!r}" if lengths and above is not None else ""
        if v < n:
            parts.append(repr(names[v]).replace("'", "") + tail)
            continue
        t = v - n
        if not 0 <= t < n - 2:
            raise ValueError(f"node {v} is not a node of a tree of {n} leaves")
        count = 3 if t == n - 3 else 2
        stack.append(")" + tail)
        for c in range(count - 1, -1, -1):
            if kids[t][c] >= v:
                raise ValueError(f"record {t} joins node {kids[t][c]}, which does not exist at that point")
            stack.append((kids[t][c], lens[t][c]))
            if c:
                stack.append(", ")
        stack.append("(")
    parts.append(";")
    return "".join(parts)


def patristic(tree) -> np.ndarray:
    """the path length between every two leaves of a neighbour-joining tree -> float64 [n, n], symmetric, 0 on the
    diagonal; on additive distances the matrix the tree was built from.  Host only (dvs_nj_patristic), O(n^2);
    ValueError for records that name a node not yet made or already joined."""
    n, joins, lens = distance.nj_inputs(tree)
    out = np.zeros((n, n), dtype=np.float64)
    _lib.raise_for(_lib.load().dvs_nj_patristic(None, n, _lib.ptr(joins, C.c_uint32), _lib.ptr(lens, C.c_double),
                                                _lib.ptr(out, C.c_double)), None)
    return out


def nj_tree(seqs: dict, *, k: int = 12, sketch_size: int | None = 3000, distance_mode: str = "mash",
            mash_canonical_kmers: bool | None = None, num_states: int = 4, canonical: bool = False):
    """sequences {name: uint8 codes} -> (Newick string with branch lengths, distance.NJTree): the distances of
    `distance_mode` and their neighbour-joining tree both on the GPU, the N x N matrix never leaving HBM
    (dvs_nj over the mode's source); leaf i is the i-th name.  Argument checks as
    `ctree`, and three sequences at least, before any device work."""
    if mash_canonical_kmers is None:
        mash_canonical_kmers = False
    distance.check_mode_args(distance_mode, sketch_size, mash_canonical_kmers, canonical)
    names = list(seqs)
    if len(names) < 3:
        raise ValueError("need at least three sequences for a neighbour-joining tree")
    with distance.device_side([seqs[n] for n in names], distance_mode,
                              *distance.mode_args(distance_mode, k, sketch_size, num_states, mash_canonical_kmers),
                              canonical=canonical) as dev:
        tree = dev.nj()
    return nj_to_newick(names, tree), tree


def pcoa(dist, n_axes: int = 3, *, tol: float = 1e-8, max_basis: int | None = None, strict: bool = True,
         ctx: engine.Context | None = None) -> "distance.PCoA":
    """principal coordinates (PCoA, classical MDS; include/dvs_hip.h) of an n x n distance matrix on the GPU ->
    `distance.PCoA`: the n_axes largest eigenpairs of Gower's double-centred matrix, the coordinates, the proportion of
    the inertia on each axis and the true residual of every pair.  The entries are used as they are (no square root);
    the diagonal counts as 0 and is never read; the matrix must be symmetric bit for bit and finite off the diagonal
    (ValueError).  strict: RuntimeError unless every axis converged to tol; strict=False returns what the basis of
    max_basis columns (None: min(n - 1, 512)) gave, with `converged` False -- a spectrum without gaps is a property of
    the data.  The shape and the arguments are checked before any device work.

    `dist`: anything np.asarray(dist, float64) takes, or a square, contiguous float64 torch tensor on the context's
    device, which is only READ and the same afterwards -- unlike `linkage` and `neighbor_joining` next to it, which
    overwrite theirs; the call waits for the work torch has queued on that device's current stream."""
    src, n, wait = _caller_matrix(dist)
    args = distance.check_pcoa_args(n, n_axes, tol, max_basis)
    wait()
    return distance.run_pcoa(ctx, src, *args, strict)


def ordinate(seqs: dict, n_axes: int = 3, *, k: int = 12, sketch_size: int | None = 3000, distance_mode: str = "mash",
             mash_canonical_kmers: bool | None = None, num_states: int = 4, canonical: bool = False, tol: float = 1e-8,
             max_basis: int | None = None, strict: bool = True):
    """sequences {name: uint8 codes} -> (names, distance.PCoA): the distances of `distance_mode` and their principal
    coordinates both on the GPU, the N x N matrix never leaving HBM (dvs_pcoa over the mode's source); row i of the
    coordinates is the i-th name.  Argument checks as `ctree` and `pcoa`, before any device work."""
    if mash_canonical_kmers is None:
        mash_canonical_kmers = False
    distance.check_mode_args(distance_mode, sketch_size, mash_canonical_kmers, canonical)
    names = list(seqs)
    distance.check_pcoa_args(len(names), n_axes, tol, max_basis)
    with distance.device_side([seqs[n] for n in names], distance_mode,
                              *distance.mode_args(distance_mode, k, sketch_size, num_states, mash_canonical_kmers),
                              canonical=canonical) as dev:
        return names, dev.pcoa(n_axes, tol=tol, max_basis=max_basis, strict=strict)


def landmark_pcoa(seqs, n_landmarks: int, n_axes: int = 3, *, k: int = 12, sketch_size: int | None = 3000,
                  distance_mode: str = "mash", mash_canonical_kmers: bool | None = None, num_states: int = 4,
                  canonical: bool = False, tol: float = 1e-8, max_basis: int | None = None, strict: bool = True, seeds=(0,)):
    """sequences {name: uint8 codes} -> (names, coordinates float64 [N, n_axes], landmarks int64 [L], distance.PCoA of
    the landmarks): landmark MDS.  n_landmarks rows are picked farthest-first (`DeviceSide.maxmin` from `seeds`), their
    L x L distances go to the host (L a few thousand at most) and through `pcoa`, and every row -- the landmarks
    included, which get their own coordinates back -- is projected against the landmarks by Gower's formula
    (`DeviceSide.pcoa_project`).  The N x N matrix never exists; the sketches or the count matrix are made once and stay
    in HBM.  Argument checks as `ctree`, `maxmin` and `pcoa` (n_axes <= L - 1), before any device work.

    `seqs` may also be a `distance.DeviceSide` the caller has made (sketches or a count matrix already in HBM, frequency
    rows included): it is used as it is and left open, the mode arguments are not looked at, and names is None."""
    if isinstance(seqs, distance.DeviceSide):
        names, n, side = None, seqs.n, contextlib.nullcontext(seqs)
    else:
        if mash_canonical_kmers is None:
            mash_canonical_kmers = False
        distance.check_mode_args(distance_mode, sketch_size, mash_canonical_kmers, canonical)
        names = list(seqs)
        n = len(names)
    distance.check_maxmin_args(n, n_landmarks, seeds, None)
    distance.check_pcoa_args(int(n_landmarks), n_axes, tol, max_basis)
    if names is not None:
        side = distance.device_side([seqs[name] for name in names], distance_mode,
                                    *distance.mode_args(distance_mode, k, sketch_size, num_states, mash_canonical_kmers),
                                    canonical=canonical)
    with side as dev:
        marks = dev.maxmin(n_landmarks, seeds=seeds).picks
        if marks.size < 2 or n_axes > marks.size - 1:
            raise ValueError(f"only {marks.size} landmarks could be picked: too few for {n_axes} axes")
        fit = pcoa(dev.cross_distances(dev, marks, marks), n_axes, tol=tol, max_basis=max_basis, strict=strict, ctx=dev.ctx)
        return names, dev.pcoa_project(fit, dev, None, marks), marks.astype(np.int64), fit


def cut_tree(Z, *, n_clusters: int | None = None, height: float | None = None) -> np.ndarray:
    """the flat clusters of a linkage matrix Z (scipy's layout, as `linkage` returns it) -> int64 [n], the cluster
    of every leaf, numbered by first appearance in leaf order (leaf 0 is in cluster 0).  Exactly one of:
    height=t, every merge of height <= t applied: the partition of scipy's fcluster(Z, t, "distance");
    n_clusters=K, the partition of fcluster(Z, K, "maxclust"): the first n - K merges and every following merge of the
    same height as the last of them -- a cut never separates merges of equal height, so fewer than K clusters may
    come back.  scipy's partition, not its label numbers.  Host only (dvs_linkage_cut); ValueError for a Z of the
    wrong shape, children that are not cluster ids, heights that decrease, K < 1 or not an integer, NaN t."""
    if (n_clusters is None) == (height is None):
        raise ValueError("cut_tree takes exactly one of n_clusters and height")
    pairs, heights = distance.check_linkage_matrix(Z)
    n = heights.size + 1
    if n_clusters is not None:
        if isinstance(n_clusters, bool) or not isinstance(n_clusters, (int, np.integer)) or n_clusters < 1:
            raise ValueError(f"n_clusters must be an integer of 1 or more, not {n_clusters!r}")
        criterion, value = _lib.CUT_NCLUSTERS, float(min(int(n_clusters), n))
    else:
        criterion, value = _lib.CUT_HEIGHT, float(height)
    labels = np.zeros(n, dtype=np.uint32)
    count = C.c_uint32()
    _lib.raise_for(_lib.load().dvs_linkage_cut(None, n, _lib.ptr(pairs, C.c_uint32), _lib.ptr(heights, C.c_double),
                                               criterion, value, _lib.ptr(labels, C.c_uint32), C.byref(count)), None)
    return labels.astype(np.int64)


def cluster_scores(dist, labels, *, ctx: engine.Context | None = None) -> "distance.ClusterScores":
    """the scores of a labelling (`distance.ClusterScores`: within, a, b, neighbour, silhouette per row; sizes,
    medoids, mean silhouette per cluster; the overall mean) of the rows of a caller's n x n distance matrix, reduced
    on the GPU a strip of rows at a time.  The diagonal is never read.  sklearn's silhouette_samples(dist, labels,
    metric="precomputed") is `.silhouette`.

    `dist`: anything np.asarray(dist, float64) takes, or a square, contiguous float64 torch tensor on the GPU, handled
    as `linkage` handles it (it must live on the context's device) but only READ: it is the same afterwards.  The
    shapes and the labels are checked before any device work."""
    src, n, wait = _caller_matrix(dist)
    lab = distance.check_labels(labels, n)
    if n:
        wait()
    return distance.run_cluster_scores(ctx, src, lab)


def maxmin(dist, n_select: int | None = None, *, seeds=(0,), min_distance: float | None = None,
           ctx: engine.Context | None = None) -> "distance.MaxMin":
    """farthest-first (max-min) selection (`distance.MaxMin`) over a caller's n x n distance matrix: from the seeds
    on, the row whose distance to the nearest row already taken is largest (a tie to the lowest row), until n_select
    rows are taken (None: n) or every row lies within min_distance of one; one of the two must be given.  d(p, j) is
    dist[p, j]: a row is read as it stands (the matrix need not be symmetric), the diagonal never.

    `dist`: anything np.asarray(dist, float64) takes, or a square, contiguous float64 torch tensor on the GPU, handled
    as `cluster_scores` handles it and only READ.  The arguments are checked before any device work."""
    src, n, wait = _caller_matrix(dist)
    args = distance.check_maxmin_args(n, n_select, seeds, min_distance)
    wait()
    return distance.run_maxmin(ctx, src, *args)


def kmedoids(dist, n_medoids: int, *, init="build", max_swaps: int = 300,
             ctx: engine.Context | None = None) -> "distance.KMedoids":
    """k-medoids (PAM; include/dvs_hip.h "k-medoids") over a caller's n x n dissimilarity matrix on the GPU ->
    `distance.KMedoids`: the n_medoids rows that minimise the total distance of every row to its nearest one, with the
    partition they make.  d(x, o) is dist[x, o]: a row is read as it stands (the matrix need not be symmetric), the
    diagonal never; every other entry must be finite and >= 0 (ValueError).  init: "build" (PAM's BUILD), "maxmin"
    (the first n_medoids picks of `maxmin` from row 0) or the initial medoids as rows; max_swaps = 0 scores a set as it
    is -- the picks of `nmost` or `maxmin` as representatives, say.

    `dist`: anything np.asarray(dist, float64) takes, or a square, contiguous float64 torch tensor on the GPU, handled
    as `cluster_scores` handles it and only READ.  The arguments are checked before any device work."""
    src, n, wait = _caller_matrix(dist)
    k, kind, rows, max_swaps = distance.check_kmedoids_args(n, n_medoids, init, max_swaps)
    wait()
    if kind == "maxmin":
        rows = distance.run_maxmin(ctx, src, *distance.check_maxmin_args(n, k, (0,), None)).picks.astype(np.uint32)
        if rows.size != k:
            raise ValueError(f"farthest-first selection found only {rows.size} of {k} initial medoids")
    return distance.run_kmedoids(ctx, src, k, rows, max_swaps)


def permanova(dist, grouping, *, permutations: int = 999, seed=None, strata=None,
              ctx: engine.Context | None = None) -> "distance.PERMANOVA":
    """PERMANOVA (Anderson 2001; include/dvs_hip.h "PERMANOVA") of a grouping of the rows of a caller's n x n
    dissimilarity matrix on the GPU -> `distance.PERMANOVA`: the pseudo-F statistic of the sums of squared distances
    within the groups, and its p-value under permutations of the labels, a batch of permutations per pass over the
    matrix.  Only dist[i, j] with i < j counts: the matrix need not be symmetric, the diagonal and the lower triangle are
    never read; every entry above the diagonal must be finite and >= 0 (ValueError).  grouping, permutations, seed and
    strata as `distance.permanova`.

    `dist`: anything np.asarray(dist, float64) takes, or a square, contiguous float64 torch tensor on the GPU, handled
    as `cluster_scores` handles it and only READ.  The arguments are checked before any device work."""
    src, n, wait = _caller_matrix(dist)
    checked = distance.check_permanova_args(n, grouping, permutations, seed, strata)
    wait()
    return distance.run_permanova(ctx, src, *checked)


def representatives(seqs: dict, n: int, *, k: int = 12, sketch_size: int | None = 3000, distance_mode: str = "mash",
                    mash_canonical_kmers: bool | None = None, num_states: int = 4, canonical: bool = False, init="build",
                    max_swaps: int = 300):
    """sequences {name: uint8 codes} -> (the names of the n representatives, int64 [n] the size of each one's cluster,
    int64 [N] labels: the position among the representatives of every sequence's nearest one, in the order of seqs;
    the `distance.KMedoids`): the distances of `distance_mode` and k-medoids over them both on the GPU, the N x N
    matrix never leaving HBM.  Argument checks as `ctree` and `kmedoids`, before any device work."""
    if mash_canonical_kmers is None:
        mash_canonical_kmers = False
    distance.check_mode_args(distance_mode, sketch_size, mash_canonical_kmers, canonical)
    names = list(seqs)
    distance.check_kmedoids_args(len(names), n, init, max_swaps)
    with distance.device_side([seqs[name] for name in names], distance_mode,
                              *distance.mode_args(distance_mode, k, sketch_size, num_states, mash_canonical_kmers),
                              canonical=canonical) as dev:
        fit = dev.kmedoids(n, init=init, max_swaps=max_swaps)
    return [names[i] for i in fit.medoids.tolist()], np.bincount(fit.labels, minlength=n).astype(np.int64), fit.labels, fit


def sampled_kmedoids(seqs, n_medoids: int, n_sample: int, *, k: int = 12, sketch_size: int | None = 3000,
                     distance_mode: str = "mash", mash_canonical_kmers: bool | None = None, num_states: int = 4,
                     canonical: bool = False, init="build", max_swaps: int = 300, seeds=(0,)):
    """sequences {name: uint8 codes} -> (names, medoids int64 [n_medoids] as rows of the collection, labels int64 [N],
    dist float64 [N], landmarks int64 [L], distance.KMedoids of the landmarks): k-medoids of a collection whose N x N
    matrix cannot exist.  n_sample rows are picked farthest-first (`DeviceSide.maxmin` from `seeds`), their L x L
    distances go to the host and through `kmedoids`, and every row is given its nearest medoid
    (`DeviceSide.nearest(..., 1)`: labels, the position among the medoids; dist, the distance to it).  The sketches or
    the count matrix are made once and stay in HBM.  Argument checks as `ctree`, `maxmin` and `kmedoids` (n_medoids <=
    n_sample), before any device work.

    `seqs` may also be a `distance.DeviceSide` the caller has made: it is used as it is and left open, the mode
    arguments are not looked at, and names is None."""
    if isinstance(seqs, distance.DeviceSide):
        names, n, side = None, seqs.n, contextlib.nullcontext(seqs)
    else:
        if mash_canonical_kmers is None:
            mash_canonical_kmers = False
        distance.check_mode_args(distance_mode, sketch_size, mash_canonical_kmers, canonical)
        names = list(seqs)
        n = len(names)
    distance.check_maxmin_args(n, n_sample, seeds, None)
    distance.check_kmedoids_args(int(n_sample), n_medoids, init, max_swaps)
    if names is not None:
        side = distance.device_side([seqs[name] for name in names], distance_mode,
                                    *distance.mode_args(distance_mode, k, sketch_size, num_states, mash_canonical_kmers),
                                    canonical=canonical)
    with side as dev:
        marks = dev.maxmin(n_sample, seeds=seeds).picks
        if marks.size < n_medoids:
            raise ValueError(f"only {marks.size} landmarks could be picked: too few for {n_medoids} medoids")
        fit = kmedoids(dev.cross_distances(dev, marks, marks), n_medoids, init=init, max_swaps=max_swaps, ctx=dev.ctx)
        medoids = marks[fit.medoids]
        labels, dist = dev.nearest(dev, 1, None, medoids)
        return names, medoids.astype(np.int64), labels[:, 0], dist[:, 0], marks.astype(np.int64), fit


def within(dist, radius, *, skip_self: bool = True, max_pairs: int | None = None,
           ctx: engine.Context | None = None) -> "distance.Neighbours":
    """for every row of a caller's n x n distance matrix the columns with dist[i, j] <= radius (`distance.Neighbours`:
    ascending columns, the matrix's own bits), compacted on the GPU a strip of rows at a time.  skip_self (the default):
    the diagonal is left out and never read.  A NaN entry is never listed; the matrix need not be symmetric.

    `dist`: as `cluster_scores` takes it, only READ.  The radius and max_pairs are checked before any device work."""
    radius = distance.check_radius(radius)
    limit = distance.check_max_pairs(max_pairs)
    src, n, wait = _caller_matrix(dist)
    if n:
        wait()
    return distance.run_within(ctx, src, None, radius, _lib.WITHIN_SKIP_SELF if skip_self else 0, limit)


def threshold_clusters(dist, radius, *, ctx: engine.Context | None = None) -> "distance.ThresholdClusters":
    """the groups that "dist[i, j] <= radius" makes of the rows of a caller's n x n distance matrix
    (`distance.ThresholdClusters`): connected components, the labels of `cut_tree(linkage(dist, "single"), height=radius)`
    without the tree.  Only the entries above the diagonal are read, a strip of rows at a time; a NaN entry joins nothing.

    `dist`: as `cluster_scores` takes it, only READ.  The radius is checked before any device work."""
    radius = distance.check_radius(radius)
    src, n, wait = _caller_matrix(dist)
    if n:
        wait()
    return distance.run_threshold_clusters(ctx, src, radius)


def _check_symmetric(dist, n: int) -> None:
    """ValueError unless a caller's matrix equals its transpose, NaN cells in the same places: on the host for an array,
    with torch for a device tensor (one n x n boolean beside it)"""
    torch = sys.modules.get("torch")
    if torch is not None and isinstance(dist, torch.Tensor):
        same = bool(((dist == dist.T) | (torch.isnan(dist) & torch.isnan(dist.T))).all())
    else:
        d = np.asarray(dist, dtype=np.float64)
        same = bool(((d == d.T) | (np.isnan(d) & np.isnan(d.T))).all())
    if not same:
        raise ValueError(f"the {n} x {n} distance matrix is not symmetric (check_symmetric=False skips this check)")


def _kth_smallest(dist, m: int) -> np.ndarray:
    """the m-th smallest cell of every row of a caller's matrix, the row's own cell included, NaN cells last: float64
    [n] on the host (np.partition, or torch.kthvalue for a device tensor)"""
    torch = sys.modules.get("torch")
    if torch is not None and isinstance(dist, torch.Tensor):
        filled = torch.where(torch.isnan(dist), torch.full_like(dist, float("inf")), dist)
        return torch.kthvalue(filled, m, dim=1).values.cpu().numpy()
    d = np.asarray(dist, dtype=np.float64)
    return np.partition(np.where(np.isnan(d), np.inf, d), m - 1, axis=1)[:, m - 1]


def minimum_spanning_tree(dist, *, core=None, min_samples: int | None = None, check_symmetric: bool = True,
                          ctx: engine.Context | None = None) -> "distance.MST":
    """the minimum spanning tree (`distance.MST`: the edges in ascending (weight, lower row, higher row), unique under
    that order) of a caller's symmetric n x n distance matrix, a strip of rows at a time: a host matrix larger than the
    device's memory is served, where `linkage(dist, "single")` -- the faster route to the same heights when the matrix
    fits -- is not.  A NaN entry is no edge (a spanning forest comes back where they disconnect the rows); the diagonal
    is never taken.  core: one distance per row, the weights become max(dist[i, j], core[i], core[j]) (the
    mutual-reachability distance of HDBSCAN); or min_samples = m: core[i] the m-th smallest entry of row i, the diagonal
    included (sklearn's convention) -- ValueError for a row with fewer than m entries that are not NaN.
    check_symmetric=False skips the symmetry check; for an asymmetric matrix some spanning tree is returned and nothing
    more is promised.

    `dist`: as `cluster_scores` takes it, only READ.  The arguments are checked before the tree's device work."""
    if min_samples is not None and core is not None:
        raise ValueError("minimum_spanning_tree takes at most one of min_samples and core")
    src, n, wait = _caller_matrix(dist)
    if min_samples is not None:
        m = distance.check_min_samples(min_samples, n)
    core = distance.check_core(core, n)
    if n:
        wait()
    if check_symmetric and n:
        _check_symmetric(dist, n)
    if min_samples is not None:
        core = _kth_smallest(dist, m)
        if np.isinf(core).any():
            raise ValueError(f"row {int(np.argmax(np.isinf(core)))} has fewer than min_samples = {m} distances that are not NaN")
        core = distance.check_core(core, n)
    return distance.run_mst(ctx, src, core)


def mst_linkage(mst) -> np.ndarray:
    """a `distance.MST` -> scipy's linkage matrix Z of the single-linkage tree (host only, dvs_linkage_from_mst): the
    heights are the sorted weights, bit for bit those of `linkage(dist, "single")`; where no two weights are equal Z is
    scipy's, among equal weights the merges follow the edges' order (the same partitions at every cut).  ValueError for
    a forest (`mst.connected` is False) and for fewer than two rows"""
    n = int(mst.n)
    if n < 2:
        raise ValueError("need at least two sequences to build a tree")
    edges = np.ascontiguousarray(np.asarray(mst.edges, dtype=np.int64).reshape(-1, 2))
    weights = np.ascontiguousarray(np.asarray(mst.weights, dtype=np.float64))
    if edges.shape[0] != weights.size:
        raise ValueError(f"{edges.shape[0]} edges with {weights.size} weights")
    if weights.size != n - 1:
        raise ValueError(f"a spanning forest of {n - weights.size} trees ({weights.size} edges over {n} rows) has no linkage tree")
    if edges.size and (edges.min() < 0 or edges.max() >= n):
        raise ValueError(f"an edge names a row outside 0 .. {n - 1}")
    pairs, heights, sizes = distance.tree_outputs(n)
    e32 = np.ascontiguousarray(edges.astype(np.uint32).ravel())
    _lib.raise_for(_lib.load().dvs_linkage_from_mst(None, n, _lib.ptr(e32, C.c_uint32), _lib.ptr(weights, C.c_double),
                                                    _lib.ptr(pairs, C.c_uint32), _lib.ptr(heights, C.c_double),
                                                    _lib.ptr(sizes, C.c_uint32)), None)
    return distance.linkage_matrix(pairs, heights, sizes)


def mst_to_edges(names: Sequence, mst) -> list:
    """a `distance.MST` over the rows `names` -> [(name, name, weight)], in the tree's order"""
    if len(names) != mst.n:
        raise ValueError(f"{len(names)} names for a spanning tree over {mst.n} rows")
    return [(names[int(a)], names[int(b)], float(w)) for (a, b), w in zip(mst.edges.tolist(), mst.weights.tolist())]


def mst_ctree(seqs: dict, *, k: int = 12, sketch_size: int | None = 3000, distance_mode: str = "mash",
              mash_canonical_kmers: bool | None = None, num_states: int = 4, canonical: bool = False,
              min_samples: int | None = None) -> str:
    """sequences {name: uint8 codes} -> the Newick string of `ctree(..., linkage="single")` without the N x N matrix: the
    minimum spanning tree strip by strip (`distance.mst`), `mst_linkage`, `linkage_to_newick`.  The merge heights are
    ctree's bit for bit; among merges of equal height the nesting may differ.  min_samples: the tree of the
    mutual-reachability distance instead (robust single linkage).  Argument checks as `ctree`, before any device work;
    ValueError where NaN distances (a sequence without a valid k-mer) leave a forest."""
    if mash_canonical_kmers is None:
        mash_canonical_kmers = False
    distance.check_mode_args(distance_mode, sketch_size, mash_canonical_kmers, canonical)
    names = list(seqs)
    if len(names) < 2:
        raise ValueError("need at least two sequences to build a tree")
    tree = distance.mst([seqs[n] for n in names], distance_mode, k=k, sketch_size=sketch_size, num_states=num_states,
                        mash_canonical=mash_canonical_kmers, canonical=canonical, min_samples=min_samples)
    return linkage_to_newick(names, mst_linkage(tree))


def dereplicate(seqs: dict, radius, *, k: int = 12, sketch_size: int | None = 3000, distance_mode: str = "mash",
                mash_canonical_kmers: bool | None = None, num_states: int = 4, canonical: bool = False):
    """sequences {name: uint8 codes} -> (None, None, distance.ClusterScores): the groups of sequences joined by
    distances <= radius (`distance.threshold_clusters`: "cluster at mash distance 0.05") and their scores, whose
    `.medoids` name one representative per group -- the member with the least summed distance to the rest of it.  The
    shape is `ctree_clusters`', with None for the tree and its linkage matrix, which are not built: neither is the
    N x N matrix.  Argument checks as `ctree` and the radius, before any device work.

    The sketches (mash) or the count matrix (euclidean, jsd) are made once and stay in HBM; the groups and the scores
    each compute the distances strip by strip (the same cells bit for bit)."""
    if mash_canonical_kmers is None:
        mash_canonical_kmers = False
    radius = distance.check_radius(radius)
    distance.check_mode_args(distance_mode, sketch_size, mash_canonical_kmers, canonical)
    names = list(seqs)
    if not names:
        raise ValueError("no sequences")
    with distance.device_side([seqs[n] for n in names], distance_mode,
                              *distance.mode_args(distance_mode, k, sketch_size, num_states, mash_canonical_kmers),
                              canonical=canonical) as dev:
        return None, None, dev.cluster_scores(dev.threshold_clusters(radius).labels)


def ctree_clusters(seqs: dict, *, n_clusters: int | None = None, height: float | None = None, k: int = 12,
                   sketch_size: int | None = 3000, distance_mode: str = "mash", mash_canonical_kmers: bool | None = None,
                   num_states: int = 4, linkage: str = "average", canonical: bool = False):
    """sequences {name: uint8 codes} -> (Newick string, Z, distance.ClusterScores): `ctree`'s device tree, its cut
    (`cut_tree`: exactly one of n_clusters and height) and the scores of the cut's clusters, row i the i-th name.
    Argument checks as `ctree`, before any device work.

    The sketches (mash) or the count matrix (euclidean, jsd) are made once and stay in HBM.  The tree stage overwrites
    its N x N matrix, so the scores compute the distances a second time, strip by strip (the same cells bit for bit):
    one more pass of the pair kernels and no second N x N buffer."""
    if mash_canonical_kmers is None:
        mash_canonical_kmers = False
    distance.check_mode_args(distance_mode, sketch_size, mash_canonical_kmers, canonical)
    distance.linkage_method_code(linkage)
    if (n_clusters is None) == (height is None):
        raise ValueError("ctree_clusters takes exactly one of n_clusters and height")
    names = list(seqs)
    if len(names) < 2:
        raise ValueError("need at least two sequences to build a tree")
    with distance.device_side([seqs[n] for n in names], distance_mode,
                              *distance.mode_args(distance_mode, k, sketch_size, num_states, mash_canonical_kmers),
                              canonical=canonical) as dev:
        Z = dev.linkage(linkage)
        labels = cut_tree(Z, n_clusters=n_clusters, height=height)
        return linkage_to_newick(names, Z), Z, dev.cluster_scores(labels)


def cophenet(Z, dist=None, *, matrix: bool = False, ctx: engine.Context | None = None):
    """scipy.cluster.hierarchy.cophenet for a linkage matrix Z in scipy's layout -- any well-formed one: the heights
    need not be monotone, so scipy's centroid and median trees are fine.

    dist=None: the cophenetic distances as the square matrix, float64 [n, n] -- squareform(scipy's cophenet(Z)) bit for
    bit; host only (dvs_linkage_cophenet).  Otherwise `distance.CopheneticScores`: the correlation of the rows of a
    caller's n x n distance matrix with the cophenetic distances (scipy's cophenet(Z, Y)[0] for its condensed form Y),
    reduced on the GPU a strip of rows at a time; the diagonal is never read; matrix=True also brings the cophenetic
    matrix back.  `dist`: as `cluster_scores` takes it -- anything np.asarray(dist, float64) takes, or a square,
    contiguous float64 torch tensor on the context's device, which is only READ.  The shapes are checked before any
    device work; ValueError for a Z whose merges name a cluster not yet made or already merged."""
    if dist is None:
        pairs, heights = distance.check_linkage_matrix(Z)
        n = heights.size + 1
        coph = np.zeros((n, n), dtype=np.float64)
        _lib.raise_for(_lib.load().dvs_linkage_cophenet(None, n, _lib.ptr(pairs, C.c_uint32), _lib.ptr(heights, C.c_double),
                                                        _lib.ptr(coph, C.c_double)), None)
        return coph
    src, n, wait = _caller_matrix(dist)
    if n == 0:  # nothing to compute: no device work either
        if np.asarray(Z).size:
            raise ValueError(f"a linkage matrix of 0 leaves is empty, not of shape {np.asarray(Z).shape}")
        return distance.CopheneticScores(float("nan"), np.zeros((5, 0)), np.zeros((0, 0)) if matrix else None)
    pairs, heights = distance.check_linkage_matrix(Z, n)
    wait()
    return distance.run_cophenet(ctx, src, pairs, heights, matrix)


def ctree_cophenet(seqs: dict, *, linkage: str = "average", k: int = 12, sketch_size: int | None = 3000,
                   distance_mode: str = "mash", mash_canonical_kmers: bool | None = None, num_states: int = 4,
                   matrix: bool = False, canonical: bool = False):
    """sequences {name: uint8 codes} -> (Newick string, Z, distance.CopheneticScores): `ctree`'s device tree and its
    cophenetic correlation with the distances it was built from, leaf i the i-th name.  Argument checks as `ctree`,
    before any device work.  As in `ctree_clusters` the sketches or the count matrix are made once, and the walk computes
    the distances a second time, strip by strip (the same cells bit for bit)."""
    if mash_canonical_kmers is None:
        mash_canonical_kmers = False
    distance.check_mode_args(distance_mode, sketch_size, mash_canonical_kmers, canonical)
    distance.linkage_method_code(linkage)
    names = list(seqs)
    if len(names) < 2:
        raise ValueError("need at least two sequences to build a tree")
    with distance.device_side([seqs[n] for n in names], distance_mode,
                              *distance.mode_args(distance_mode, k, sketch_size, num_states, mash_canonical_kmers),
                              canonical=canonical) as dev:
        Z = dev.linkage(linkage)
        return linkage_to_newick(names, Z), Z, dev.cophenet(Z, matrix=matrix)


def compare_linkages(seqs: dict, methods: Sequence[str] = ("single", "complete", "average", "weighted", "ward"), *,
                     k: int = 12, sketch_size: int | None = 3000, distance_mode: str = "mash",
                     mash_canonical_kmers: bool | None = None, num_states: int = 4, canonical: bool = False) -> dict:
    """sequences {name: uint8 codes} -> {method: (Z, cophenetic correlation)} for every linkage method of `methods`:
    which of them represents these distances best.  The sketches or the count matrix are made once; then a tree and a
    walk per method (`ctree_cophenet`'s, the same bits).  Argument checks as `ctree`, before any device work."""
    if mash_canonical_kmers is None:
        mash_canonical_kmers = False
    distance.check_mode_args(distance_mode, sketch_size, mash_canonical_kmers, canonical)
    methods = list(methods)
    for method in methods:
        distance.linkage_method_code(method)
    names = list(seqs)
    if len(names) < 2:
        raise ValueError("need at least two sequences to build a tree")
    with distance.device_side([seqs[n] for n in names], distance_mode,
                              *distance.mode_args(distance_mode, k, sketch_size, num_states, mash_canonical_kmers),
                              canonical=canonical) as dev:
        out = {}
        for method in methods:
            Z = dev.linkage(method)
            out[method] = (Z, dev.cophenet(Z).correlation)
        return out
