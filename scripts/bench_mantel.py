"""Time the Mantel test: one JSON line per size and number of permutations over families of mutated
sequences, jsd (k = --k) against mash (k = --mash-k, sketch size --sketch) of the same sequences; wall clock around each
call, median of --reps runs after a warm-up, profiler off.
  draw_ms         the Python layer's own part: the permutations drawn (mantel.permutations)
  call_ms         dvs_mantel over the two N x N matrices as device tensors: the entry and centre passes, the second
                  matrix's copy, the host's check and staging of the permutations, their uploads, one scoring pass a batch
  fused_ms        the same over the count matrix and the sketches: both matrices written first
  perm_us         (call_ms - the call_ms of 0 permutations) / P: a permutation with the host work beside it
  floor_us, x_floor   the time ONE matrix's bytes (8 N^2) need at --hbm-tbs, and perm_us over it
  host_perm_ms, host_ms   the host route on the same box: numpy's gather of n^2 doubles plus a dot product (the median of
                  --host-perms permutations), and (P + 1) host_perm_ms, extrapolated
  batches         at the largest number of permutations: call_ms and perm_us per DVS_MANTEL_BATCH of --batches
Kernel times come from a trace of this script, in a run of its own:
  rocprofv3 --kernel-trace --stats -d DIR -o mantel --output-format csv -- python scripts/bench_mantel.py --reps 1

  python scripts/bench_mantel.py [--sizes 10000,2000] [--perms 0,99,999] [--batches 8,16,32] [--reps 3] [--out FILE]
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
sys.path.insert(0, str(ROOT / "scripts"))


def host_cross_sum(u: np.ndarray, V: np.ndarray, pi: np.ndarray, iu) -> float:
    """one permutation's Z on the host: the gather of n^2 doubles and a dot product over the upper triangle"""
    return float(np.dot(u, V[np.ix_(pi, pi)][iu]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,2000")
    ap.add_argument("--perms", default="0,99,999")
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--mash-k", type=int, default=12)
    ap.add_argument("--sketch", type=int, default=1000)
    ap.add_argument("--length", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", default="8,16,32")
    ap.add_argument("--host-perms", type=int, default=3)
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM rate of the floor, TB/s")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from bench_maxmin import family_rows
    from diverseseq_amd import _lib, distance, engine, mantel

    ctx = engine.Context(0)
    info = ctx.device_info()
    ints = lambda text: [int(v) for v in text.split(",") if v]

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

    def with_env(env: dict, fn):
        for key, value in env.items():
            os.environ[key] = value
        ctx.refresh_knobs()
        try:
            return fn()
        finally:
            for key in env:
                del os.environ[key]
            ctx.refresh_knobs()

    for n in ints(args.sizes):
        rows = list(family_rows(n, args.length, n))
        m = ctx.build_matrix(rows, args.k, 4)
        sk = distance.Sketches(rows, args.mash_k, args.sketch, 4, False, ctx=ctx)
        del rows
        side_x, side_y = distance.DeviceSide(m, "jsd"), distance.DeviceSide(sk, "mash")
        dx, dy = side_x.distances(), side_y.distances()
        tx, ty = torch.from_numpy(dx).to("cuda:0"), torch.from_numpy(dy).to("cuda:0")
        torch.cuda.synchronize()
        src = lambda t: distance.make_source(_lib.SRC_GIVEN, t.data_ptr(), n, on_device=1, keep=t)
        iu = np.triu_indices(n, 1)
        u = dx[iu] - dx[iu].mean()
        V = dy - dy[iu].mean()
        floor_us = 8.0 * n * n / (args.hbm_tbs * 1e12) * 1e6
        base_ms = None
        for P in ints(args.perms):
            draw_ms, perms = timed(lambda: mantel.permutations(n, P, 1))
            call_ms, fit = timed(lambda: mantel.run_mantel(ctx, src(tx), src(ty), perms))
            fused_ms, fused = timed(lambda: mantel.run_mantel(ctx, side_x._source(), side_y._source(), perms))
            per = []
            for pi in [np.arange(n)] + [perms[p].astype(np.int64) for p in range(min(P, args.host_perms - 1))]:
                t0 = time.perf_counter()
                host_cross_sum(u, V, pi, iu)
                per.append((time.perf_counter() - t0) * 1e3)
            host_perm_ms = float(np.median(per))
            line = {"bench": "mantel", "x": f"jsd k={args.k}", "y": f"mash k={args.mash_k} s={args.sketch}", "n": n, "permutations": P,
                    "draw_ms": round(draw_ms, 3), "call_ms": round(call_ms, 3), "fused_ms": round(fused_ms, 3), "r": fit.r,
                    "p_value": fit.p_value, "passes": fit.passes,
                    "same_as_fused": bool(np.array_equal(fit.z, fused.z) and np.array_equal(fit.moments, fused.moments)),
                    "floor_us": round(floor_us, 1), "host_perm_ms": round(host_perm_ms, 3), "host_ms": round((P + 1) * host_perm_ms, 1)}
            if P == 0:
                base_ms = call_ms
            elif base_ms is not None:
                perm_us = (call_ms - base_ms) / P * 1e3
                line.update({"perm_us": round(perm_us, 2), "x_floor": round(perm_us / floor_us, 2)})
            if args.batches and P == max(ints(args.perms)) and P:
                batches = {}
                for b in ints(args.batches):
                    knobs = {"DVS_MANTEL_BATCH": str(b)}
                    zero = with_env(knobs, lambda: timed(lambda: mantel.run_mantel(ctx, src(tx), src(ty), perms[:0]))[0])
                    ms, got = with_env(knobs, lambda: timed(lambda: mantel.run_mantel(ctx, src(tx), src(ty), perms)))
                    batches[str(b)] = {"call_ms": round(ms, 3), "perm_us": round((ms - zero) / P * 1e3, 2),
                                       "same_bits": bool(np.array_equal(got.z, fit.z))}
                line["batches"] = batches
            emit(line)
        m.close()
        sk.close()
        del tx, ty, dx, dy, u, V
        ctx.check(ctx._L.dvs_ctx_trim(ctx._h))


if __name__ == "__main__":
    main()
