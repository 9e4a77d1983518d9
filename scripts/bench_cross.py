"""Rectangular distances and nearest references against the square path (profiles/bench_cross.jsonl):
N uniform-random 5 kb sequences, k = 6 for jsd / euclidean, k = 12 and s = 3 000 for mash, seeds fixed.  Every shape
is called four times (the first is the warm-up); the like-for-like shapes alternate the rectangular and the square call.

  kernel times (profiler on):
    rocprofv3 --kernel-trace --stats -d DIR -o cross --output-format csv -- python scripts/bench_cross.py --plan DIR/plan.json
    python scripts/bench_cross.py --summarise DIR/cross_kernel_trace.csv --plan DIR/plan.json >> profiles/bench_cross.jsonl
  wall clock (profiler off):
    python scripts/bench_cross.py --wall >> profiles/bench_cross.jsonl

The run writes its plan -- per call, in order, how many launches of which kernel it makes -- and the summary cuts the
trace by it: per shape and kernel the median over the three calls after the warm-up of the call's summed kernel time,
pairs per second, and for jsd the bin-pairs per second as a fraction of the FP64 planning rate."""
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
PLANNING_RATE = 78.6e12 / 2 / 20   # bin-pairs per second (scripts/jsd_kernel_times.py)
STRIP_BYTES, TILE = 256 << 20, 32  # csrc/crossdist.hip
CALLS = 4

# (name, mode, M, N or None for the square path over M rows)
SHAPES = [
    ("jsd 7071x7071", "jsd", 7071, 7071), ("jsd square 10000", "jsd", 10000, None),
    ("euclidean 7071x7071", "euclidean", 7071, 7071), ("euclidean square 10000", "euclidean", 10000, None),
    ("jsd 100000x100", "jsd", 100000, 100), ("jsd 100000x1000", "jsd", 100000, 1000), ("jsd 50x10000", "jsd", 50, 10000),
    ("mash 707x707", "mash", 707, 707), ("mash square 1000", "mash", 1000, None), ("mash 50x10000", "mash", 50, 10000),
]
KERNEL_OF = {"jsd": ("jsd_cross_kernel", "jsd_pairs_kernel"), "euclidean": ("euclid_cross_kernel", "euclid_kernel"),
             "mash": ("mash_pairs_kernel<true>", "mash_pairs_kernel<false>")}


def strips(m, n):
    rows = min(m, max(STRIP_BYTES // (n * 8) // TILE * TILE, TILE))
    return -(-m // rows)


def seqs(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 4, LENGTH, dtype=np.uint8) for _ in range(n)]


class Sides:
    """the device side of a mode over M query and N reference sequences, built once per size and kept"""

    def __init__(self, ctx):
        self.ctx, self.cache = ctx, {}

    def get(self, mode, n, seed):
        from diverseseq_amd import distance

        key = ("mash" if mode == "mash" else "counts", n, seed)
        if key not in self.cache:
            s = seqs(n, seed)
            self.cache[key] = (distance.Sketches(s, MASH_K, MASH_S, ctx=self.ctx) if mode == "mash"
                               else self.ctx.build_matrix(s, K))
        return self.cache[key]

    def drop(self):
        for h in self.cache.values():
            h.close()
        self.cache = {}


def calls_of(shape, sides):
    """-> [(label, function, {kernel: launches per call})] for one shape"""
    from diverseseq_amd import distance

    name, mode, m, n = shape
    cross_k, square_k = KERNEL_OF[mode]
    q = sides.get(mode, m, 1)
    if n is None:
        square = {"jsd": distance.matrix_jsd_distances, "euclidean": distance.matrix_euclidean_distances}
        fn = q.distances if mode == "mash" else (lambda: square[mode](q))
        launches = {square_k: 1}
        if mode == "jsd":
            launches["jsd_finish_kernel"] = 1
        return [(name, fn, launches)]
    r = sides.get(mode, n, 2)
    ns = strips(m, n)
    base = {cross_k: ns}
    if mode == "jsd":
        base["jsd_entropy_kernel"] = 2
    out = [(name, (lambda: q.cross_distances(r)) if mode == "mash" else (lambda: distance.matrix_cross_distances(q, r, mode)), base)]
    for kk in (1, 16):
        near = (lambda kk=kk: q.nearest(r, kk)) if mode == "mash" else (lambda kk=kk: distance.matrix_nearest(q, r, kk, mode))
        out.append((f"{name} nearest {kk}", near, {**base, "cross_topk_kernel": ns}))
    return out


def run(plan_path, wall):
    from diverseseq_amd import engine

    ctx = engine.Context(0)
    sides = Sides(ctx)
    plan = []
    # the like-for-like pairs alternate call by call: rectangular, square, rectangular, ...
    groups = [SHAPES[0:2], SHAPES[2:4], [SHAPES[4]], [SHAPES[5]], [SHAPES[6]], SHAPES[7:9], [SHAPES[9]]]
    for group in groups:
        todo = [c for shape in group for c in calls_of(shape, sides)]
        times = collections.defaultdict(list)
        for _ in range(CALLS):
            for label, fn, launches in todo:
                t0 = time.perf_counter()
                fn()
                times[label].append((time.perf_counter() - t0) * 1e3)
                plan.append({"label": label, "launches": launches})
        if wall:
            for label, ms in times.items():
                print(json.dumps({"bench": "cross_wall", "shape": label, "call_ms": [round(x, 2) for x in ms],
                                  "median_ms_after_warmup": round(statistics.median(ms[1:]), 2)}), flush=True)
        if group is groups[2]:
            continue  # (the 100 000-row matrix serves the next shape too)
        sides.drop()
        ctx._L.dvs_ctx_trim(ctx._h)
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
    shape_of = {s[0]: s for s in SHAPES}
    for label, kernels in per.items():
        base = label.split(" nearest")[0]
        _, mode, m, n = shape_of[base]
        pairs = m * (m - 1) // 2 if n is None else m * n
        for name, ms in kernels.items():
            med = statistics.median(ms[1:])
            row = {"bench": "cross_kernel", "shape": label, "kernel": name, "pairs": pairs, "call_ms": [round(x, 3) for x in ms],
                   "median_ms_after_warmup": round(med, 3)}
            if name in KERNEL_OF[mode]:
                row["ns_per_pair"] = round(med * 1e6 / pairs, 4)
                if mode == "jsd":
                    rate = pairs * 4 ** K / (med * 1e-3)
                    row.update(bin_pairs_per_s=round(rate), fraction_of_fp64_planning_rate=round(rate / PLANNING_RATE, 3))
            print(json.dumps(row))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--plan", default=None, help="where the run writes (or the summary reads) the launch plan")
    ap.add_argument("--wall", action="store_true", help="print wall-clock rows (run without the profiler)")
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV", default=None)
    args = ap.parse_args()
    summarise(args.summarise, args.plan) if args.summarise else run(args.plan, args.wall)
