"""`dvs ctree` path: distances and the linkage tree on the GPU.

Mirrors diverse_seq/cluster.py: `make_cluster_tree` (:191-237 -- sklearn
AgglomerativeClustering(metric="precomputed", linkage="average"), children_ folded into a
nested tuple, printed without quotes) and the argument checks of `dvs_ctree.__init__`
(:113-162).  The reference hands the string to cogent3's make_tree; here it is returned as a
Newick string.  `ctree` builds the tree on the device by default (`linkage`: scipy's
nearest-neighbour chain, or for single linkage its minimum spanning tree, in one persistent
workgroup, csrc/linkage.hip, the same linkage matrix bit for bit); `tree="sklearn"` keeps the
reference's host path (`make_cluster_tree`, average linkage only).
"""

from __future__ import annotations

import ctypes as C
import sys
from collections.abc import Sequence

import numpy as np

from . import distance, engine


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
    torch = sys.modules.get("torch")
    if torch is not None and isinstance(dist, torch.Tensor) and dist.is_cuda:
        if dist.dtype != torch.float64 or dist.dim() != 2 or dist.shape[0] != dist.shape[1] or not dist.is_contiguous():
            raise ValueError("a device distance matrix must be a square, contiguous float64 tensor")
        n = int(dist.shape[0])
        src, on_device = C.c_void_p(dist.data_ptr()), 1
        torch.cuda.current_stream(dist.device).synchronize()  # (torch's stream -> the library's)
    else:
        d = np.ascontiguousarray(np.asarray(dist, dtype=np.float64))
        if d.ndim != 2 or d.shape[0] != d.shape[1]:
            raise ValueError(f"expected a square distance matrix, got shape {d.shape}")
        n = d.shape[0]
        src, on_device = d.ctypes.data_as(C.c_void_p), 0
    return distance.run_linkage(ctx, n, "dvs_linkage", src, on_device, n, code,
                                too_few=f"Found array with {n} sample(s) while a minimum of 2 is required")


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
          linkage: str = "average") -> str:
    """sequences {name: uint8 codes} -> Newick string (dvs_ctree.main, cluster.py:164-188).
    Argument checks as dvs_ctree.__init__ (cluster.py:139-162).  distance_mode: the reference's "mash" and
    "euclidean", and "jsd", the Jensen-Shannon divergence of the k-mer frequencies (`distance.jsd_distances`),
    which takes the euclidean mode's arguments.

    tree="device": the distances and the tree both on the GPU, the N x N matrix never leaves HBM
    (dvs_sketches_linkage / dvs_matrix_euclidean_linkage / dvs_matrix_jsd_linkage), the string from
    `linkage_to_newick`; `linkage`: any method the module's `linkage` function builds.  tree="sklearn": the reference's path (the matrix copied to the host, sklearn, nested
    tuples; `make_cluster_tree`), average linkage only.  Both give the same string wherever the sklearn path
    returns one; the one intended difference is a tree deeper than Python's recursion limit (e.g. a caterpillar of
    a few thousand leaves), for which the device path returns the Newick string where the sklearn path raises
    RecursionError."""
    if mash_canonical_kmers is None:
        mash_canonical_kmers = False
    if distance_mode not in distance.MODES:
        raise ValueError(f"Unexpected distance {distance_mode!r}.")
    if distance_mode == "mash" and sketch_size is None:
        raise ValueError("Expected sketch size for mash distance measure.")
    if distance_mode != "mash" and sketch_size is not None:
        raise ValueError("Sketch size should only be specified for the mash distance.")
    if distance_mode != "mash" and mash_canonical_kmers:
        raise ValueError("Canonical kmers should only be specified for the mash distance.")
    if tree not in ("device", "sklearn"):
        raise ValueError(f"Unexpected tree {tree!r}: 'device' or 'sklearn'.")
    distance.linkage_method_code(linkage)
    if tree == "sklearn" and linkage != "average":
        raise ValueError(f"tree='sklearn' builds average linkage only, not {linkage!r}: use tree='device'")
    names = list(seqs)
    arrays = [seqs[n] for n in names]
    distances, tree_of = distance.MODES[distance_mode]
    args = distance.mode_args(distance_mode, k, sketch_size, num_states, mash_canonical_kmers)
    if tree == "sklearn":
        return make_cluster_tree(names, distances(arrays, *args))
    return linkage_to_newick(names, tree_of(arrays, *args, method=linkage))
