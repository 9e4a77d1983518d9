"""The cophenetic correlation against the nearest reference over the same strips (DESIGN.md 4.11,
profiles/cophenet_bench.jsonl): N uniform-random 5 kb sequences, k = 6 for jsd, k = 12 and s = 3 000 for mash, seeds
fixed; the tree is the device's own for the shape's linkage method (ward: balanced; single: a caterpillar-like chain).
Per shape `cophenet` and `nearest(..., n_nearest=1)` over the same rows alternate call by call, four times each (the
first is the warm-up): both walk the same strips and make one pass over every strip row, so the second is the yardstick
of the first.

  wall clock (profiler off):
    python scripts/bench_cophenet.py --wall >> profiles/cophenet_bench.jsonl
  kernel times (profiler on, the cophenet calls alone, so the stats file is theirs):
    rocprofv3 --kernel-trace --stats -d DIR -o cophenet --output-format csv -- python scripts/bench_cophenet.py --only-cophenet
    (DIR/cophenet_kernel_stats.csv -> profiles/cophenet_kernel_stats.csv)
  host baseline, for the table only (the N x N matrix copied out, then scipy's cophenet(Z, Y) on one core):
    python scripts/bench_cophenet.py --host-baseline >> profiles/cophenet_bench.jsonl"""
import argparse
import json
import pathlib
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

K, LENGTH, MASH_K, MASH_S = 6, 5000, 12, 3000
CALLS = 4

# (name, mode, N, linkage method)
SHAPES = [("jsd 10000 ward", "jsd", 10000, "ward"), ("jsd 10000 single", "jsd", 10000, "single"),
          ("mash 1000 average", "mash", 1000, "average")]


def device_side(ctx, mode, n):
    from diverseseq_amd import distance

    rng = np.random.default_rng(1)
    seqs = [rng.integers(0, 4, LENGTH, dtype=np.uint8) for _ in range(n)]
    return distance.device_side(seqs, mode, *((MASH_K, MASH_S) if mode == "mash" else (K,)), ctx=ctx)


def depth(Z):
    """the longest path from the root to a leaf, in merges"""
    n = Z.shape[0] + 1
    d = np.zeros(2 * n - 1, dtype=np.int64)
    for j in range(n - 2, -1, -1):
        d[int(Z[j, 0])] = d[int(Z[j, 1])] = d[n + j] + 1
    return int(d[:n].max())


def run(wall, only_cophenet):
    from diverseseq_amd import engine

    ctx = engine.Context(0)
    side = {}
    for name, mode, n, method in SHAPES:
        if (mode, n) not in side:
            for h in side.values():
                h.close()
            side = {(mode, n): device_side(ctx, mode, n)}
        dev = side[mode, n]
        Z = dev.linkage(method)
        calls = [("cophenet", lambda: dev.cophenet(Z)), ("nearest 1", lambda: dev.nearest(dev, 1))]
        if only_cophenet:
            calls = calls[:1]
        times = {what: [] for what, _ in calls}
        r = None
        for _ in range(CALLS):
            for what, fn in calls:
                t0 = time.perf_counter()
                out = fn()  # (returns once the stream is drained and the host outputs are written)
                times[what].append((time.perf_counter() - t0) * 1e3)
                if what == "cophenet":
                    r = out.correlation
        if wall:
            med = {what: statistics.median(ms[1:]) for what, ms in times.items()}
            for what, ms in times.items():
                print(json.dumps({"bench": "cophenet_wall", "shape": name, "call": what, "call_ms": [round(x, 2) for x in ms],
                                  "median_ms_after_warmup": round(med[what], 2)}), flush=True)
            row = {"bench": "cophenet_wall_ratio", "shape": name, "tree_depth": depth(Z), "correlation": r}
            if not only_cophenet:
                row.update(cophenet_over_nearest_1=round(med["cophenet"] / med["nearest 1"], 3), limit=1.25)
            print(json.dumps(row), flush=True)
    for h in side.values():
        h.close()


def host_baseline():
    from scipy.cluster.hierarchy import cophenet

    from diverseseq_amd import engine

    ctx = engine.Context(0)
    name, mode, n, method = SHAPES[0]
    dev = device_side(ctx, mode, n)
    Z = dev.linkage(method)
    got = dev.cophenet(Z).correlation
    t0 = time.perf_counter()
    d = dev.distances()  # the N x N matrix computed again and copied out of HBM
    t1 = time.perf_counter()
    y = d[np.triu_indices(n, 1)]
    t2 = time.perf_counter()
    r = float(cophenet(Z, y)[0])
    t3 = time.perf_counter()
    dev.close()
    print(json.dumps({"bench": "cophenet_host_baseline", "shape": name, "distances_and_copy_ms": round((t1 - t0) * 1e3, 1),
                      "condense_ms": round((t2 - t1) * 1e3, 1), "scipy_cophenet_ms": round((t3 - t2) * 1e3, 1),
                      "total_ms": round((t3 - t0) * 1e3, 1), "scipy_correlation": r, "device_correlation": got,
                      "difference": abs(r - got)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--wall", action="store_true", help="print wall-clock rows (run without the profiler)")
    ap.add_argument("--only-cophenet", action="store_true", help="no nearest calls (for a profiler run)")
    ap.add_argument("--host-baseline", action="store_true", help="scipy on the copied-out matrix, first shape")
    args = ap.parse_args()
    host_baseline() if args.host_baseline else run(args.wall, args.only_cophenet)
