"""Time k-medoids: one JSON line per size and number of medoids over families of mutated sequences,
the jsd count matrix (k = --k) already in HBM; wall clock around each call, median of --reps runs after a warm-up.
  total_ms        distance.matrix_kmedoids(m, n_medoids): the distances, the entry check, BUILD and the swap phase
  distance_ms     the distance stage: the call with given medoids and max_swaps = 0 over the count matrix minus the same
                  call over the N x N matrix as a device tensor (the entry check and one assignment, nothing else)
  build_ms        the call with max_swaps = 0 minus the call with BUILD's medoids given and max_swaps = 0
  swap_ms, rounds, round_us   the rest; the scored rounds (the exchanges and the one that finds none); swap_ms / rounds
  floor_us, x_floor           a round's byte floor, 8 N^2 bytes at --hbm-tbs, and round_us over it
  pcoa_pass_us, x_pcoa_pass   with --pcoa-pass-us "N:us,...": one pass of pcoa_product_kernel at the same N, from the
                              kernel trace of this script run with --pcoa under rocprofv3 (it reads the same matrix once)
  maxmin_ms, maxmin_td, maxmin_rounds   the same call with init="maxmin"; build_td: the final td of init="build"
  --batches "1,4,...": total_ms per DVS_KMEDOIDS_BATCH at the first size and number of medoids, as batch_ms

  python scripts/bench_kmedoids.py [--sizes 1000,4000,10000] [--medoids 10,100] [--reps 3] [--out FILE] [--pcoa]
--out appends.  --pcoa also runs cluster.pcoa over the device tensor, so that a kernel trace holds both kernels."""
import argparse
import json
import os
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,4000,10000")
    ap.add_argument("--medoids", default="10,100")
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--length", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", default="")
    ap.add_argument("--pcoa", action="store_true")
    ap.add_argument("--pcoa-pass-us", default="")
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM rate of the floor, TB/s")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from bench_maxmin import family_rows
    from diverseseq_amd import cluster, distance, engine

    ctx = engine.Context(0)
    info = ctx.device_info()
    ints = lambda text: [int(v) for v in text.split(",") if v]
    pcoa_pass = dict((int(a), float(b)) for a, b in (item.split(":") for item in args.pcoa_pass_us.split(",") if item))

    def timed(fn):
        ts = []
        for _ in range(args.reps + 1):  # (the first run is the warm-up)
            ctx.sync()
            t0 = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts[1:])), out

    def emit(line):
        line.update({"reps": args.reps, "device": info["name"], "host_cpus": len(os.sched_getaffinity(0))})
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")

    first = True
    for n in ints(args.sizes):
        rows = family_rows(n, args.length, n)
        m = ctx.build_matrix(list(rows), args.k, 4)
        del rows
        t = torch.from_numpy(distance.matrix_jsd_distances(m)).to("cuda:0")
        torch.cuda.synchronize()
        if args.pcoa:
            cluster.pcoa(t, 3, strict=False, ctx=ctx)
        for k in ints(args.medoids):
            if k > n:
                continue
            total_ms, fit = timed(lambda: distance.matrix_kmedoids(m, k))
            built_ms, built = timed(lambda: distance.matrix_kmedoids(m, k, max_swaps=0))
            given_ms, _ = timed(lambda: distance.matrix_kmedoids(m, k, init=built.medoids, max_swaps=0))
            tensor_ms, _ = timed(lambda: cluster.kmedoids(t, k, init=built.medoids, max_swaps=0, ctx=ctx))
            tensor_total_ms, on_tensor = timed(lambda: cluster.kmedoids(t, k, ctx=ctx))
            mm_ms, mm = timed(lambda: distance.matrix_kmedoids(m, k, init="maxmin"))
            rounds = fit.passes - k
            swap_ms = total_ms - built_ms
            floor_us = 8.0 * n * n / (args.hbm_tbs * 1e12) * 1e6
            line = {"bench": "kmedoids", "mode": "jsd", "k": args.k, "n": n, "n_medoids": k, "total_ms": round(total_ms, 3),
                    "distance_ms": round(given_ms - tensor_ms, 3), "build_ms": round(built_ms - given_ms, 3),
                    "check_assign_ms": round(tensor_ms, 3), "swap_ms": round(swap_ms, 3), "rounds": rounds,
                    "n_swaps": len(fit.swaps), "stop": fit.stop, "round_us": round(swap_ms / max(rounds, 1) * 1e3, 1),
                    "floor_us": round(floor_us, 1), "x_floor": round(swap_ms / max(rounds, 1) * 1e3 / floor_us, 2),
                    "tensor_total_ms": round(tensor_total_ms, 3),
                    "same_as_tensor": bool(all(np.array_equal(a, b) for a, b in zip(fit, on_tensor))),
                    "td_init": float(fit.td[0]), "build_td": float(fit.td[-1]), "maxmin_ms": round(mm_ms, 3),
                    "maxmin_td_init": float(mm.td[0]), "maxmin_td": float(mm.td[-1]), "maxmin_rounds": mm.passes - 1,
                    "maxmin_stop": mm.stop}
            if n in pcoa_pass:
                line.update({"pcoa_pass_us": pcoa_pass[n], "x_pcoa_pass": round(line["round_us"] / pcoa_pass[n], 2)})
            if first and args.batches:
                batch_ms = {}
                for b in ints(args.batches):
                    os.environ["DVS_KMEDOIDS_BATCH"] = str(b)
                    ctx.refresh_knobs()
                    batch_ms[str(b)] = round(timed(lambda: distance.matrix_kmedoids(m, k))[0], 3)
                del os.environ["DVS_KMEDOIDS_BATCH"]
                ctx.refresh_knobs()
                line["batch_ms"] = batch_ms
            first = False
            emit(line)
        m.close()
        del t
        ctx.check(ctx._L.dvs_ctx_trim(ctx._h))


if __name__ == "__main__":
    main()
