"""Time PERMANOVA: one JSON line per size and number of permutations over families of mutated sequences,
the jsd count matrix (k = --k) already in HBM, --groups groups of consecutive sequences; wall clock around each call, median of
--reps runs after a warm-up.
  draw_ms         the Python layer's own part: the grouping encoded and the permutations drawn (distance.check_permanova_args)
  call_ms         dvs_permanova over the N x N matrix as a device tensor: the host's check and narrowing of the label
                  vectors, their uploads, the entry check and one pass a batch
  fused_ms        the same over the count matrix: the distances written first
  passes, batch   what the call reports; pass_us = (call_ms - the call_ms of 0 permutations) / (passes - 2): a batch's
                  pass with the host work beside it; perm_us the same per permutation
  floor_us, x_floor   the time HALF the matrix's bytes (4 N^2) need at --hbm-tbs, and pass_us over it
  host_dist_ms, host_perm_ms, host_ms   the host route on the same box: the matrix to the host (jsd_distances), one label
                  vector's SS_W in numpy (the median of --host-perms vectors), and host_dist_ms + (P + 1) host_perm_ms
  --batches "8,16,32": call_ms per DVS_PERMANOVA_BATCH at the first size and the largest number of permutations, as batch_ms
Kernel times come from a trace of this script, in a run of its own:
  rocprofv3 --kernel-trace --stats -d DIR -o permanova --output-format csv -- python scripts/bench_permanova.py --reps 1 --entry
--entry also runs the k-medoids entry pass (kmed_score_kernel<0>) over the same tensor, so that the trace holds both.

  python scripts/bench_permanova.py [--sizes 10000] [--perms 0,99,999] [--groups 10] [--reps 3] [--out FILE]
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


def host_ss_within(q: np.ndarray, labels: np.ndarray, a: int) -> float:
    """one label vector's SS_W from the squared upper triangle, group by group"""
    order = np.argsort(labels, kind="stable")
    bounds = np.searchsorted(labels[order], np.arange(a + 1))
    return float(sum(q[np.ix_(order[bounds[g]:bounds[g + 1]], order[bounds[g]:bounds[g + 1]])].sum() / (bounds[g + 1] - bounds[g])
                     for g in range(a)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000")
    ap.add_argument("--perms", default="0,99,999")
    ap.add_argument("--groups", type=int, default=10)
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--length", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", default="")
    ap.add_argument("--host-perms", type=int, default=3)
    ap.add_argument("--entry", action="store_true")
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM rate of the floor, TB/s")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from bench_maxmin import family_rows
    from diverseseq_amd import _lib, cluster, distance, engine

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

    first = True
    for n in ints(args.sizes):
        rows = family_rows(n, args.length, n)
        m = ctx.build_matrix(list(rows), args.k, 4)
        del rows
        host_dist_ms, dist = timed(lambda: distance.matrix_jsd_distances(m))
        t = torch.from_numpy(dist).to("cuda:0")
        torch.cuda.synchronize()
        grouping = (np.arange(n) * args.groups // n).tolist()  # (whole families: the groups do explain the distances)
        tensor_src = distance.make_source(_lib.SRC_GIVEN, t.data_ptr(), n, on_device=1, keep=t)
        side = distance.DeviceSide(m, "jsd")
        if args.entry:
            cluster.kmedoids(t, 2, max_swaps=0, ctx=ctx)
        iu = np.triu_indices(n, 1)
        q = np.zeros((n, n))
        q[iu] = dist[iu] ** 2
        del iu
        base_ms = None
        for P in ints(args.perms):
            draw_ms, checked = timed(lambda: distance.check_permanova_args(n, grouping, P, 1, None))
            call_ms, fit = timed(lambda: distance.run_permanova(ctx, tensor_src, *checked))
            fused_ms, fused = timed(lambda: distance.run_permanova(ctx, side._source(), *checked))
            labels, a, perms = checked
            vectors = [labels] + [perms[p] for p in range(min(P, args.host_perms - 1))]
            per = []
            for v in vectors:
                t0 = time.perf_counter()
                host_ss_within(q, v.astype(np.int64), a)
                per.append((time.perf_counter() - t0) * 1e3)
            host_perm_ms = float(np.median(per))
            passes = 1 + -(-(P + 1) // 16)
            floor_us = 4.0 * n * n / (args.hbm_tbs * 1e12) * 1e6
            line = {"bench": "permanova", "mode": "jsd", "k": args.k, "n": n, "groups": a, "permutations": P,
                    "draw_ms": round(draw_ms, 3), "call_ms": round(call_ms, 3), "fused_ms": round(fused_ms, 3),
                    "f": fit.f, "p_value": fit.p_value, "same_as_fused": bool(all(np.array_equal(x, y, equal_nan=True) for x, y in zip(fit, fused))),
                    "floor_us": round(floor_us, 1), "host_dist_ms": round(host_dist_ms, 3), "host_perm_ms": round(host_perm_ms, 3),
                    "host_ms": round(host_dist_ms + (P + 1) * host_perm_ms, 1)}
            if P == 0:
                base_ms = call_ms
            elif base_ms is not None and passes > 2:
                pass_us = (call_ms - base_ms) / (passes - 2) * 1e3
                line.update({"passes": passes, "pass_us": round(pass_us, 1), "perm_us": round((call_ms - base_ms) / P * 1e3, 2),
                             "x_floor": round(pass_us / floor_us, 2)})
            if first and args.batches and P == max(ints(args.perms)):
                batch_ms = {}
                for b in ints(args.batches):
                    os.environ["DVS_PERMANOVA_BATCH"] = str(b)
                    ctx.refresh_knobs()
                    batch_ms[str(b)] = round(timed(lambda: distance.run_permanova(ctx, tensor_src, *checked))[0], 3)
                del os.environ["DVS_PERMANOVA_BATCH"]
                ctx.refresh_knobs()
                line["batch_ms"] = batch_ms
                first = False
            emit(line)
        m.close()
        del t, q
        ctx.check(ctx._L.dvs_ctx_trim(ctx._h))


if __name__ == "__main__":
    main()
