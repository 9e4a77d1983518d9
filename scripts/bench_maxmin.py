"""Time farthest-first selection: one JSON line per mode and size with
  maxmin_ms          the call -- distance.matrix_maxmin (jsd, k = --k) or Sketches.maxmin (mash, k = 12, s = 3 000) with
                     n_select = --select -- over inputs already in HBM; wall clock around the call, median of --reps
                     runs after a warm-up
  floor_ms, x_floor  (a) per step one pass over the rows (N x bins x count bytes, or N x s x 4 sketch bytes) at --hbm-tbs
                     plus the step's launches (jsd: 2, mash: 3) at --boundary-us; times the steps; and the ratio to it
  matrix_route_ms    (b) where the N x N matrix fits (N <= --matrix-max): what the code before this feature would do,
                     matrix_jsd_distances / Sketches.distances on the same inputs plus a vectorised host greedy over
                     the matrix (tests/test_maxmin_host.py's maxmin_ref); x_matrix_route = that over maxmin_ms; same_picks:
                     the two agree
  cross_kernel_ms    (c) jsd only: the same traversal with jsd_cross_kernel launched on one query row in place of
                     jsd_row_kernel (DVS_MAXMIN_JSD_CROSS=1); x_cross_kernel = that over maxmin_ms

  python scripts/bench_maxmin.py [--jsd-sizes 10000,100000] [--mash-sizes 1000,10000] [--select 100] [--reps 3] [--out FILE]
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


def family_rows(n: int, length: int, seed: int) -> np.ndarray:
    """uint8 [n, length]: families of 20 copies of a random root with 1-8 % substitutions"""
    rng = np.random.default_rng(seed)
    roots = rng.integers(0, 4, ((n + 19) // 20, length), dtype=np.uint8)
    out = np.repeat(roots, 20, axis=0)[:n].copy()
    hit = rng.random(out.shape, dtype=np.float32) < rng.uniform(0.01, 0.08, (n, 1)).astype(np.float32)
    out[hit] = rng.integers(0, 4, int(hit.sum()), dtype=np.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jsd-sizes", default="10000,100000")
    ap.add_argument("--mash-sizes", default="1000,10000")
    ap.add_argument("--select", type=int, default=100)
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--length", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--matrix-max", type=int, default=10000, help="largest N at which the matrix route is timed too")
    ap.add_argument("--no-ab", action="store_true", help="skip (c), the jsd_cross_kernel traversal")
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM rate of the floor, TB/s")
    ap.add_argument("--boundary-us", type=float, default=1.45, help="a dependent launch boundary of the floor, us")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from diverseseq_amd import distance, engine
    from test_maxmin_host import maxmin_ref

    ctx = engine.Context(0)
    info = ctx.device_info()
    sizes = lambda text: [int(v) for v in text.split(",") if v]

    def timed(fn):
        ts = []
        for _ in range(args.reps + 1):  # (the first run is the warm-up)
            ctx.sync()
            t0 = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts[1:])), out

    def emit(line):
        line.update({"n_select": args.select, "reps": args.reps, "device": info["name"],
                     "host_cpus": len(os.sched_getaffinity(0))})
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        ctx.check(ctx._L.dvs_ctx_trim(ctx._h))

    def matrix_route(line, ms, got, square):
        def route():
            return maxmin_ref(square(), args.select)

        route_ms, ref = timed(route)
        line.update({"matrix_route_ms": round(route_ms, 3), "x_matrix_route": round(route_ms / ms, 2),
                     "same_picks": bool(np.array_equal(ref.picks, got.picks))})

    for n in sizes(args.jsd_sizes):
        rows = family_rows(n, args.length, n)
        m = ctx.build_matrix(list(rows), args.k, 4)
        del rows
        ms, got = timed(lambda: distance.matrix_maxmin(m, args.select, mode="jsd"))
        steps = len(got.picks)
        pass_bytes = n * m.nbins * m.count_bytes
        floor = steps * (pass_bytes / (args.hbm_tbs * 1e12) * 1e3 + 2 * args.boundary_us * 1e-3)
        line = {"bench": "maxmin", "mode": "jsd", "k": args.k, "n": n, "steps": steps, "maxmin_ms": round(ms, 3),
                "pass_mb": round(pass_bytes / 1e6, 2), "floor_ms": round(floor, 3), "x_floor": round(ms / floor, 2),
                "count_bytes": m.count_bytes}
        if n <= args.matrix_max:
            matrix_route(line, ms, got, lambda: distance.matrix_jsd_distances(m))
        if not args.no_ab:
            os.environ["DVS_MAXMIN_JSD_CROSS"] = "1"
            ctx.refresh_knobs()
            ab_ms, ab = timed(lambda: distance.matrix_maxmin(m, args.select, mode="jsd"))
            del os.environ["DVS_MAXMIN_JSD_CROSS"]
            ctx.refresh_knobs()
            line.update({"cross_kernel_ms": round(ab_ms, 3), "x_cross_kernel": round(ab_ms / ms, 2),
                         "cross_kernel_same_picks": bool(np.array_equal(ab.picks, got.picks))})
        m.close()
        emit(line)

    for n in sizes(args.mash_sizes):
        k, s = 12, 3000
        rows = family_rows(n, 5000, n + 1)
        sk = distance.Sketches(list(rows), k, s, ctx=ctx)
        del rows
        ms, got = timed(lambda: sk.maxmin(args.select))
        steps = len(got.picks)
        pass_bytes = n * s * 4
        floor = steps * (pass_bytes / (args.hbm_tbs * 1e12) * 1e3 + 3 * args.boundary_us * 1e-3)
        line = {"bench": "maxmin", "mode": "mash", "k": k, "sketch_size": s, "n": n, "steps": steps,
                "maxmin_ms": round(ms, 3), "pass_mb": round(pass_bytes / 1e6, 2), "floor_ms": round(floor, 3),
                "x_floor": round(ms / floor, 2)}
        if n <= args.matrix_max:
            matrix_route(line, ms, got, sk.distances)
        sk.close()
        emit(line)


if __name__ == "__main__":
    main()
