"""Time the canonical fold and selections over folded rows: per k one JSON line for the fold and one
per n for the selections, over sequences that are already in HBM (random bases, --rows x --length)
  fold_ms            (a) CountMatrix.canonical() alone -- dvs_matrix_fold_canonical, which returns when the folded rows are
                     written -- wall clock around the call, median of --reps runs after a warm-up
  floor_ms, x_floor  the bytes of the source rows plus the bytes of the folded rows at --hbm-tbs; the ratio to it
  plain / folded     (b) nmost(n) over the plain and over the folded matrix: wall clock of the call (median of --reps after
                     a warm-up), and of the last run the engine (0: one scan launch per window, 1: persistent), the sum of
                     its scan launches' durations and the rows it scored

  python scripts/bench_canonical.py [--rows 100000] [--length 5000] [--ks 6,7] [--ns 10,100] [--reps 3] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--length", type=int, default=5000)
    ap.add_argument("--ks", default="6,7")
    ap.add_argument("--ns", default="10,100")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM rate of the floor, TB/s")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from diverseseq_amd import engine

    ctx = engine.Context(0)
    info = ctx.device_info()
    ints = lambda text: [int(v) for v in text.split(",") if v]

    def timed(fn, done=lambda out: None):
        ts, out = [], None
        for _ in range(args.reps + 1):  # (the first run is the warm-up)
            done(out)
            ctx.sync()
            t0 = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts[1:])), out

    def emit(line):
        line.update({"bench": "canonical", "rows": args.rows, "length": args.length, "reps": args.reps,
                     "device": info["name"], "host_cpus": len(os.sched_getaffinity(0))})
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")

    gen = torch.Generator(device="cuda:0").manual_seed(args.rows + args.length)
    seqs = torch.randint(0, 4, (args.rows * args.length + 16,), dtype=torch.uint8, device="cuda:0", generator=gen)
    torch.cuda.synchronize()
    offsets = np.arange(args.rows + 1, dtype=np.uint64) * np.uint64(args.length)
    close = lambda h: h.close() if h is not None else None
    ctx.set_timing(True)
    for k in ints(args.ks):
        plain = ctx.build_matrix_device(seqs.data_ptr(), offsets, k, 4)
        ctx.sync()
        fold_ms, folded = timed(plain.canonical, close)
        moved = args.rows * (plain.nbins + folded.nbins) * plain.count_bytes
        floor = moved / (args.hbm_tbs * 1e12) * 1e3
        emit({"what": "fold", "k": k, "count_bytes": plain.count_bytes, "plain_bins": plain.nbins,
              "folded_bins": folded.nbins, "fold_ms": round(fold_ms, 3), "moved_mb": round(moved / 1e6, 1),
              "floor_ms": round(floor, 3), "x_floor": round(fold_ms / floor, 2)})
        for n in ints(args.ns):
            line = {"what": "nmost", "k": k, "n": n}
            for name, m in (("plain", plain), ("folded", folded)):
                ms, sel = timed(lambda: m.nmost(n), close)
                s = sel.summary()
                line[name] = {"bins": m.nbins, "wall_ms": round(ms, 3), "engine": int(s.engine), "scan_ms": round(s.scan_ms, 3),
                              "scan_launches": int(s.scan_launches), "rows_scored": int(s.rows_scored),
                              "n_accepts": int(s.n_accepts), "total_jsd": s.total_jsd}
                sel.close()
            line["x_wall"] = round(line["folded"]["wall_ms"] / line["plain"]["wall_ms"], 3)
            emit(line)
        folded.close()
        plain.close()
        ctx.check(ctx._L.dvs_ctx_trim(ctx._h))


if __name__ == "__main__":
    main()
