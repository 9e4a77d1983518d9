"""Kernel times of the jsd and euclidean pair kernels (profiles/jsd_kernel_times.jsonl): N uniform-random
5 kb sequences at k = 6, four calls of each distance entry per N (the first is the warm-up).

  rocprofv3 --kernel-trace --stats -d DIR -o jsd --output-format csv -- python scripts/jsd_kernel_times.py
  python scripts/jsd_kernel_times.py --summarise DIR/jsd_kernel_trace.csv > profiles/jsd_kernel_times.jsonl

The summary takes the median of the launches after the first per kernel and N, and for jsd_pairs_kernel the bin-pairs
per second, N (N - 1) / 2 x 4^k, as a fraction of the FP64 planning rate (78.6 TFLOPS counted 2 per fma, 20 instructions
per bin-pair)."""
import argparse
import collections
import csv
import ctypes as C
import json
import pathlib
import statistics
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

K, LENGTH = 6, 5000
PLANNING_RATE = 78.6e12 / 2 / 20  # bin-pairs per second
KERNELS = ("jsd_pairs_kernel", "jsd_finish_kernel", "euclid_kernel")


def run(sizes):
    from diverseseq_amd import _lib, distance, engine

    ctx = engine.Context(0)
    for n in sizes:
        rng = np.random.default_rng(n + 1)
        m = ctx.build_matrix([rng.integers(0, 4, LENGTH, dtype=np.uint8) for _ in range(n)], K)
        out = np.zeros((n, n))
        p = out.ctypes.data_as(C.POINTER(C.c_double))
        for kind in (_lib.SRC_JSD, _lib.SRC_EUCLIDEAN):
            src = distance.make_source(kind, m._h, n)
            for _ in range(4):
                ctx.check(ctx._L.dvs_distances(ctx._h, src, p))
        m.close()


def summarise(trace, sizes):
    runs = collections.defaultdict(list)  # kernel -> durations in launch order
    for r in csv.DictReader(open(trace)):
        for name in KERNELS:
            if name in r["Kernel_Name"]:
                runs[name].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    for name in KERNELS:
        assert len(runs[name]) == 4 * len(sizes), (name, len(runs[name]))
        for i, n in enumerate(sizes):
            ms = runs[name][4 * i: 4 * i + 4]
            row = {"kernel": name, "n": n, "k": K, "nbins": 4 ** K, "launch_ms": [round(x, 3) for x in ms],
                   "median_ms_after_warmup": round(statistics.median(ms[1:]), 3)}
            if name == "jsd_pairs_kernel":
                rate = n * (n - 1) // 2 * 4 ** K / (statistics.median(ms[1:]) * 1e-3)
                row.update(bin_pairs=n * (n - 1) // 2 * 4 ** K, bin_pairs_per_s=round(rate),
                           fraction_of_fp64_planning_rate=round(rate / PLANNING_RATE, 3))
            print(json.dumps(row))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,4000,10000")
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV", default=None)
    args = ap.parse_args()
    sizes = [int(v) for v in args.sizes.split(",")]
    summarise(args.summarise, sizes) if args.summarise else run(sizes)
