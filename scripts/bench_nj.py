"""Time the neighbour-joining tree: for N in 1 000, 4 000, 10 000 one JSON line with
  nj_tensor_ms       cluster.neighbor_joining of a noisy additive N x N matrix already in HBM (a torch tensor, the
                     working buffer: no upload); wall clock around the call, median of --reps runs after a warm-up
  floor_read_ms      sum over r = 4 .. N of r (r - 1) / 2 * 8 bytes at --hbm-tbs (what the scans must read)
  floor_launch_ms    2 (N - 3) launch boundaries at --boundary-us
  average_tensor_ms  cluster.linkage(..., "average") of the same matrix in HBM, the same way: the O(N^2) tree beside
                     the O(N^3) one
  same_tree          the device tree's splits are those of the tree the matrix was made from (N <= 4 000); false is
                     expected: the 5 % noise is far above that tree's shortest branches (1 / 1024)
and, for the sizes of --restated, restated_numpy_ms: the vectorised numpy restatement of the algorithm
(tests/test_nj_host.py) on this host; and, for the sizes of --fused, fused_jsd_ms: distance.jsd_nj, sequences -> counts
-> N x N divergences -> tree, all in HBM (uniform-random 5 kb sequences, k = --k).

  python scripts/bench_nj.py [--sizes 1000,4000,10000] [--restated 1000] [--fused 10000] [--k 6] [--reps 3] [--out FILE]
--out appends."""
import argparse
import json
import os
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def noisy_additive(n: int, seed: int):
    """(the generating tree's children, A * (1 + 0.05 * random)): a random tree with branch lengths in (0, 1]"""
    from test_nj_host import dyadic_tree

    tree, A = dyadic_tree(n, "random", seed=seed)
    rng = np.random.default_rng(seed)
    noise = np.triu(rng.random((n, n)), 1)
    return tree, A * (1.0 + 0.05 * (noise + noise.T))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,4000,10000")
    ap.add_argument("--restated", default="1000", help="sizes at which the numpy restatement is timed too")
    ap.add_argument("--fused", default="10000", help="sizes at which the fused jsd entry is timed too")
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM rate of the floor, TB/s")
    ap.add_argument("--boundary-us", type=float, default=1.45, help="a dependent launch boundary of the floor, us")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from diverseseq_amd import cluster, distance, engine
    from test_nj_host import restated, split_lengths

    ctx = engine.Context(0)
    info = ctx.device_info()
    sizes = [int(v) for v in args.sizes.split(",") if v]
    also = lambda text: {int(v) for v in text.split(",") if v}
    warm = noisy_additive(300, 1)[1]
    cluster.neighbor_joining(warm, ctx=ctx)
    cluster.linkage(warm, "average", ctx=ctx)

    def tensor_ms(dev, fn):
        ts = []
        for _ in range(args.reps + 1):  # (the first run of a shape is the warm-up)
            t = dev.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(t)
            ts.append((time.perf_counter() - t0) * 1e3)
            del t
        return float(np.median(ts[1:])), out

    for n in sizes:
        tree, d = noisy_additive(n, n)
        dev = torch.from_numpy(d).to("cuda:0")
        nj_ms, got = tensor_ms(dev, lambda t: cluster.neighbor_joining(t, ctx=ctx))
        avg_ms, _ = tensor_ms(dev, lambda t: cluster.linkage(t, "average", ctx=ctx))
        del dev
        read_bytes = sum(r * (r - 1) // 2 for r in range(4, n + 1)) * 8
        line = {"bench": "nj", "n": n, "nj_tensor_ms": round(nj_ms, 3), "average_tensor_ms": round(avg_ms, 3),
                "floor_read_ms": round(read_bytes / (args.hbm_tbs * 1e12) * 1e3, 3),
                "floor_launch_ms": round(2 * (n - 3) * args.boundary_us * 1e-3, 3),
                "scan_read_gb": round(read_bytes / 1e9, 2)}
        if n <= 4000:
            line["same_tree"] = bool(set(split_lengths(got, n)) == set(split_lengths(tree, n)))
        if n in also(args.restated):
            t0 = time.perf_counter()
            restated(d)
            line["restated_numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        if n in also(args.fused):
            rng = np.random.default_rng(n + 1)
            seqs = [rng.integers(0, 4, 5000, dtype=np.uint8) for _ in range(n)]
            ts = []
            for _ in range(args.reps + 1):
                t0 = time.perf_counter()
                distance.jsd_nj(seqs, args.k, ctx=ctx)
                ts.append((time.perf_counter() - t0) * 1e3)
            line["fused_jsd_ms"] = round(float(np.median(ts[1:])), 3)
            line["k"] = args.k
        line.update({"reps": args.reps, "device": info["name"], "host_cpus": len(os.sched_getaffinity(0))})
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        ctx.check(ctx._L.dvs_ctx_trim(ctx._h))


if __name__ == "__main__":
    main()
