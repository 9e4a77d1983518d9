"""Neighbours within a radius against the dense route, and threshold clusters against the tree route (DESIGN.md 4.15,
profiles/within_bench.jsonl): N sequences of 3 000 bases in families of 20 (3 % substitutions), jsd at k = 6, a radius
that keeps 15 of a sequence's 19 relatives -- under 1 % of the pairs.  Every shape is warmed up once; the calls that are
compared alternate; a call returns after its stream is drained, so the host clock around it is the call's time.

  wall clock (profiler off):
    python scripts/bench_within.py >> profiles/within_bench.jsonl
  kernel times (profiler on, the within call alone):
    rocprofv3 --kernel-trace --stats -d DIR -o within --output-format csv -- python scripts/bench_within.py --only-within
"""
import argparse
import json
import os
import pathlib
import sys
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from diverseseq_amd import cluster, distance, engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10_000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--only-within", action="store_true", help="the within call alone, for a kernel trace")
args = ap.parse_args()
N, K = args.n, 6

rng = np.random.default_rng(1)
roots = [rng.integers(0, 4, 3000, dtype=np.uint8) for _ in range((N + 19) // 20)]
seqs = []
for i in range(N):
    s = roots[i // 20].copy()
    hit = rng.random(3000) < 0.03
    s[hit] = rng.integers(0, 4, int(hit.sum()), dtype=np.uint8)
    seqs.append(s)
ctx = engine.default_context()
m = ctx.build_matrix(seqs, K, 4)
sample = distance.matrix_cross_distances(m, m, "jsd", q_rows=np.arange(0, N, 20), r_rows=np.arange(N))
radius = float(np.quantile(sample, 0.0015))


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def within():
    return distance.matrix_within(m, m, radius, "jsd", skip_self=True)


def dense():
    return distance.matrix_cross_distances(m, m, "jsd")


side = distance.DeviceSide(m, "jsd")
nb = within()  # (the warm-up)
emit(what="setup", n=N, k=K, radius=radius, pairs=int(nb.row_start[-1]), fraction=float(nb.row_start[-1]) / (N * (N - 1)),
     device=ctx.device_info()["name"])
if args.only_within:
    for _ in range(args.reps):
        within()
    sys.exit(0)
d = dense()
keep = d <= radius
np.fill_diagonal(keep, False)
assert int(keep.sum()) == int(nb.row_start[-1]) and np.array_equal(np.nonzero(keep)[1], nb.index)  # the same pairs
del keep, d
for rep in range(args.reps):
    t_dense, _ = timed(dense)
    t_within, _ = timed(within)
    emit(what="within_vs_cross_distances", rep=rep, cross_distances_s=t_dense, within_s=t_within)
for strip in ("512", "2048", None):  # more strips, more per-strip synchronisations (default at N = 10 000: 3 328 rows a strip)
    if strip:
        os.environ["DVS_CROSS_STRIP_ROWS"] = strip
    else:
        os.environ.pop("DVS_CROSS_STRIP_ROWS", None)
    engine.refresh_all_knobs()
    within(), dense()
    t_within, _ = timed(within)
    t_dense, _ = timed(dense)
    emit(what="strip_rows", strip_rows=strip or "default", within_s=t_within, cross_distances_s=t_dense)
side.threshold_clusters(radius)
cluster.cut_tree(side.linkage("single"), height=radius)
for rep in range(args.reps):
    t_tree, lab_tree = timed(lambda: cluster.cut_tree(side.linkage("single"), height=radius))
    t_comp, comp = timed(lambda: side.threshold_clusters(radius))
    assert np.array_equal(lab_tree, comp.labels)  # the same labels
    emit(what="threshold_clusters_vs_single_linkage_cut", rep=rep, linkage_single_cut_s=t_tree,
         threshold_clusters_s=t_comp, n_clusters=comp.n_clusters)
