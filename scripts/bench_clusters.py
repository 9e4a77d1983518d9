"""The scores of a labelling against the nearest reference over the same strips (DESIGN.md 4.10,
profiles/clusters_bench.jsonl): N uniform-random 5 kb sequences, k = 6 for jsd, k = 12 and s = 3 000 for mash, seeds
fixed, random labels in K clusters.  Per shape `cluster_scores` and `nearest(..., n_nearest=1)` over the same rows
alternate call by call, four times each (the first is the warm-up): both walk the same strips and make one pass over
every strip row, so the second is the yardstick of the first.

  kernel times (profiler on):
    rocprofv3 --kernel-trace --stats -d DIR -o clusters --output-format csv -- python scripts/bench_clusters.py --plan DIR/plan.json
    python scripts/bench_clusters.py --summarise DIR/clusters_kernel_trace.csv --plan DIR/plan.json >> profiles/clusters_bench.jsonl
  wall clock (profiler off):
    python scripts/bench_clusters.py --wall >> profiles/clusters_bench.jsonl

The run writes its plan -- per call, in order, how many launches of which kernel it makes -- and the summary cuts the
trace by it: per shape and kernel the median over the three calls after the warm-up of the call's summed kernel time."""
import argparse
import collections
import csv
import json
import pathlib
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

K, LENGTH, MASH_K, MASH_S = 6, 5000, 12, 3000
STRIP_BYTES, TILE = 256 << 20, 32  # csrc/crossdist.hip
CALLS = 4

# (name, mode, N, clusters)
SHAPES = [("jsd 10000 K=10", "jsd", 10000, 10), ("jsd 10000 K=100", "jsd", 10000, 100),
          ("jsd 10000 K=5000", "jsd", 10000, 5000), ("mash 1000 K=10", "mash", 1000, 10)]
PAIR_KERNEL = {"jsd": "jsd_cross_kernel", "mash": "mash_pairs_kernel<true>"}


def strips(n):
    rows = min(n, max(STRIP_BYTES // (n * 8) // TILE * TILE, TILE))
    return -(-n // rows)


def run(plan_path, wall):
    from diverseseq_amd import distance, engine

    ctx = engine.Context(0)
    plan, side = [], {}
    for name, mode, n, k_clusters in SHAPES:
        if (mode, n) not in side:
            for h in side.values():
                h.close()
            rng = np.random.default_rng(1)
            seqs = [rng.integers(0, 4, LENGTH, dtype=np.uint8) for _ in range(n)]
            side = {(mode, n): distance.Sketches(seqs, MASH_K, MASH_S, ctx=ctx) if mode == "mash" else ctx.build_matrix(seqs, K)}
        dev = side[mode, n]
        labels = np.random.default_rng(k_clusters).integers(0, k_clusters, size=n)
        ns = strips(n)
        base = {PAIR_KERNEL[mode]: ns}
        if mode == "jsd":
            base["jsd_entropy_kernel"] = 2
        if mode == "mash":
            calls = [("cluster_scores", lambda: dev.cluster_scores(labels), {**base, "cluster_scores_kernel": ns}),
                     ("nearest 1", lambda: dev.nearest(dev, 1), {**base, "cross_topk_kernel": ns})]
        else:
            calls = [("cluster_scores", lambda: distance.matrix_cluster_scores(dev, labels, mode),
                      {**base, "cluster_scores_kernel": ns}),
                     ("nearest 1", lambda: distance.matrix_nearest(dev, dev, 1, mode), {**base, "cross_topk_kernel": ns})]
        times = collections.defaultdict(list)
        for _ in range(CALLS):
            for what, fn, launches in calls:
                t0 = time.perf_counter()
                fn()
                times[what].append((time.perf_counter() - t0) * 1e3)
                plan.append({"label": f"{name} {what}", "launches": launches})
        if wall:
            med = {what: statistics.median(ms[1:]) for what, ms in times.items()}
            for what, ms in times.items():
                print(json.dumps({"bench": "clusters_wall", "shape": name, "call": what, "call_ms": [round(x, 2) for x in ms],
                                  "median_ms_after_warmup": round(med[what], 2)}), flush=True)
            print(json.dumps({"bench": "clusters_wall_ratio", "shape": name,
                              "cluster_scores_over_nearest_1": round(med["cluster_scores"] / med["nearest 1"], 3),
                              "limit": 1.25}), flush=True)
    for h in side.values():
        h.close()
    if plan_path:
        pathlib.Path(plan_path).write_text(json.dumps(plan))


def summarise(trace, plan_path):
    plan = json.loads(pathlib.Path(plan_path).read_text())
    runs = collections.defaultdict(list)  # kernel -> durations in launch order
    names = sorted({k for c in plan for k in c["launches"]}, key=len, reverse=True)
    rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        for name in names:
            if name in r["Kernel_Name"]:
                runs[name].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
                break
    at = collections.defaultdict(int)
    per = collections.defaultdict(lambda: collections.defaultdict(list))  # label -> kernel -> per-call ms
    for c in plan:
        for name, count in c["launches"].items():
            ms = runs[name][at[name]: at[name] + count]
            assert len(ms) == count, (c["label"], name, count, len(runs[name]))
            at[name] += count
            per[c["label"]][name].append(sum(ms))
    for name in names:
        assert at[name] == len(runs[name]), (name, at[name], len(runs[name]))
    for label, kernels in per.items():
        total = sum(statistics.median(ms[1:]) for ms in kernels.values())
        for name, ms in kernels.items():
            med = statistics.median(ms[1:])
            print(json.dumps({"bench": "clusters_kernel", "call": label, "kernel": name, "call_ms": [round(x, 3) for x in ms],
                              "median_ms_after_warmup": round(med, 3), "share_of_the_calls_kernel_time": round(med / total, 4)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--plan", default=None, help="where the run writes (or the summary reads) the launch plan")
    ap.add_argument("--wall", action="store_true", help="print wall-clock rows (run without the profiler)")
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV", default=None)
    args = ap.parse_args()
    summarise(args.summarise, args.plan) if args.summarise else run(args.plan, args.wall)
