"""Time the tree stage of `dvs ctree`: for N in 1 000, 4 000, 10 000 and every linkage method of
--methods one JSON line with
  device_host_ms    cluster.linkage of a host float64 N x N matrix (upload + check/mirror + tree loop + relabel)
  device_tensor_ms  the same matrix already in HBM (a torch tensor, the working buffer: no upload)
  fused_mash_ms     distance.mash_linkage: sketches -> N x N mash distances -> tree, all in HBM
                    (N families of 5 kb sequences, k = 12, s = 3 000)
  scipy_ms          scipy.cluster.hierarchy.linkage(condensed, method) on the host (one run)
  sklearn_fit_ms    average only: AgglomerativeClustering(metric="precomputed", linkage="average").fit on the same
                    host matrix
and, with --distance jsd|euclidean (uniform-random 5 kb sequences, k = --k), for that distance mode
  <mode>_matrix_ms  the N x N distances of a count matrix already in HBM into a host array that exists (the pair
                    kernel and the copy of the matrix to the host)
  fused_<mode>_ms   distance.<mode>_linkage: sequences -> counts -> N x N distances -> tree, all in HBM
and whether the device Z equals scipy's (z_equal).  Wall clock around calls that end in a device synchronise;
median of --reps runs after one warm-up of every shape.

  python scripts/bench_tree.py [--sizes 1000,4000,10000] [--methods average] [--distance jsd] [--k 6] [--reps 3]
                               [--out FILE]"""
import argparse
import json
import os
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def family_seqs(n: int, length: int, seed: int) -> list:
    rng = np.random.default_rng(seed)
    roots = rng.integers(0, 4, (max(1, n // 20), length), dtype=np.uint8)
    out = []
    for i in range(n):
        s = roots[i % len(roots)].copy()
        hit = rng.random(length) < rng.uniform(0.005, 0.05)
        s[hit] = rng.integers(0, 4, int(hit.sum()), dtype=np.uint8)
        out.append(s)
    return out


def uniform_seqs(n: int, length: int, seed: int) -> list:
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 4, length, dtype=np.uint8) for _ in range(n)]


def median_ms(fn, reps: int) -> float:
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,4000,10000")
    ap.add_argument("--methods", default="average", help="comma-separated: single,complete,average,weighted,ward")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sklearn-reps", type=int, default=1)
    ap.add_argument("--distance", choices=["jsd", "euclidean"], default=None,
                    help="also time this distance mode's matrix and its fused sequences -> distances -> tree path")
    ap.add_argument("--k", type=int, default=6, help="k of the --distance columns")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import ctypes as C

    import torch
    from scipy.cluster.hierarchy import linkage
    from sklearn.cluster import AgglomerativeClustering

    from diverseseq_amd import cluster, distance, engine

    methods = args.methods.split(",")
    for method in methods:
        distance.linkage_method_code(method)
    ctx = engine.Context(0)
    info = ctx.device_info()
    warm = np.random.default_rng(0).random((300, 300))
    warm_seqs = family_seqs(64, 5000, 1)
    for method in methods:
        cluster.linkage(warm, method, ctx=ctx)
        distance.mash_linkage(warm_seqs, 12, 3000, method=method, ctx=ctx)
    if args.distance:
        dist_mode = distance.DeviceSide.MODE_NAMES.index(args.distance)  # the kind of the dvs_source
        dist_linkage = getattr(distance, f"{args.distance}_linkage")
        for method in methods:
            dist_linkage(uniform_seqs(64, 5000, 1), args.k, method=method, ctx=ctx)
    lines = []
    for n in (int(v) for v in args.sizes.split(",")):
        d = np.random.default_rng(n).random((n, n))
        d = np.triu(d, 1) + np.triu(d, 1).T
        y = d[np.triu_indices(n, 1)]
        seqs = family_seqs(n, 5000, n)
        for method in methods:
            z = cluster.linkage(d, method, ctx=ctx)
            t0 = time.perf_counter()
            z_ref = linkage(y, method)
            scipy_ms = (time.perf_counter() - t0) * 1e3
            z_equal = bool(np.array_equal(z, z_ref))
            host_ms = median_ms(lambda: cluster.linkage(d, method, ctx=ctx), args.reps)
            dev = torch.from_numpy(d).to("cuda:0")
            tensor_ts = []
            for _ in range(args.reps):
                t = dev.clone()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                cluster.linkage(t, method, ctx=ctx)
                tensor_ts.append((time.perf_counter() - t0) * 1e3)
                del t
            del dev
            distance.mash_linkage(seqs, 12, 3000, method=method, ctx=ctx)
            fused_ms = median_ms(lambda: distance.mash_linkage(seqs, 12, 3000, method=method, ctx=ctx), args.reps)
            line = {"n": n, "method": method, "device_host_ms": round(host_ms, 3),
                    "device_tensor_ms": round(float(np.median(tensor_ts)), 3), "fused_mash_ms": round(fused_ms, 3),
                    "scipy_ms": round(scipy_ms, 3)}
            if args.distance:
                useqs = uniform_seqs(n, 5000, n + 1)
                m = ctx.build_matrix(useqs, args.k)
                out = np.zeros((n, n))
                src = distance.make_source(dist_mode, m._h, n)
                run = lambda: ctx.check(ctx._L.dvs_distances(ctx._h, src, out.ctypes.data_as(C.POINTER(C.c_double))))
                run()
                line[f"{args.distance}_matrix_ms"] = round(median_ms(run, args.reps), 3)
                m.close()
                del out
                dist_linkage(useqs, args.k, method=method, ctx=ctx)
                line[f"fused_{args.distance}_ms"] = round(
                    median_ms(lambda: dist_linkage(useqs, args.k, method=method, ctx=ctx), args.reps), 3)
                line["k"] = args.k
            if method == "average":
                line["sklearn_fit_ms"] = round(median_ms(
                    lambda: AgglomerativeClustering(metric="precomputed", linkage="average").fit(d), args.sklearn_reps), 3)
            line.update({"z_equal": z_equal, "reps": args.reps, "device": info["name"],
                         "host_cpus": len(os.sched_getaffinity(0))})
            print(json.dumps(line), flush=True)
            lines.append(line)
            ctx.check(ctx._L.dvs_ctx_trim(ctx._h))
    if args.out:
        pathlib.Path(args.out).write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
