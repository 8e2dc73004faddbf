"""The batch planner's throughput curve on maze_6 (690 x 402): config 4's query plus Q - 1 further free (start, end) pairs drawn with a
fixed seed, threshold 0.1, max_iter 250.  For each Q: aggregate pivots/s of vhp_planner_solve_batch (outputs=False) against the same
queries solved one after another through planner_solve_device in the same process on the same context, and their ratio.  Also the G
the group rule picks on maze_6, on a 1000^2 and on a 4096^2 map.

usage: planner_batch_bench.py [--q 1,2,4,8,16,32] [--reps N] [--out FILE] [--batch-only] [--kernel-trace DIR]
  --batch-only     no sequential solves and no group report (a run under rocprofv3 --kernel-trace, so that the trace holds the batch's
                   launches alone)
  --kernel-trace   DIR: read the *kernel_trace.csv a rocprofv3 --kernel-trace run left under DIR and report the per-launch times of the
                   latency sweep and of the batch epilogue (nothing is run on the GPU)"""
import argparse
import csv
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
from importlib import import_module  # noqa: E402


def queries_for(occ, q, seed=2024):
    synth = import_module("visibility-heuristic-path-planner_amd.synth")
    ny = occ.shape[0]
    out = [(345, ny - 1 - 391, 341, ny - 1 - 10)]   # BASELINE config 4 (mode 2 flips y)
    pts = synth.free_sources(occ, 2 * 31, seed)
    out += [tuple(int(v) for v in pts[2 * k]) + tuple(int(v) for v in pts[2 * k + 1]) for k in range(31)]
    return out[:q]


def curve(ctx, occ, qs, reps, batch_only, log):
    import torch
    log("Q  G   pivots  batch ms  batch pivots/s  seq ms  seq pivots/s  ratio   (median of %d; wall clock per call)" % reps)
    for q in qs:
        queries = queries_for(occ, q)
        res = ctx.planner_solve_batch(queries, 0.1, 250, outputs=False)   # (warm-up: allocations, the first launches)
        n_piv = sum(r["n_pivots"] for r in res)
        tb = []
        for _ in range(reps):
            t0 = time.perf_counter()
            ctx.planner_solve_batch(queries, 0.1, 250, outputs=False)
            tb.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        g = ctx.planner_batch_group()
        b = float(np.median(tb))
        if batch_only:
            log("%-2d %-3d %6d  %8.3f  %14.0f" % (q, g, n_piv, b * 1e3, n_piv / b))
            continue
        for s, e in ((qq[:2], qq[2:]) for qq in queries):
            ctx.planner_solve_device(s, e, 0.1, 250)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            n_seq = 0
            for s, e in ((qq[:2], qq[2:]) for qq in queries):
                n_seq += ctx.planner_solve_device(s, e, 0.1, 250)[1]
            ts.append(time.perf_counter() - t0)
        assert n_seq == n_piv, (n_seq, n_piv)
        sq = float(np.median(ts))
        log("%-2d %-3d %6d  %8.3f  %14.0f  %7.3f  %12.0f  %5.2fx" % (q, g, n_piv, b * 1e3, n_piv / b, sq * 1e3, n_piv / sq, sq / b))
        for r in res:
            assert r["status"] in (0, 20), r   # (VHP_OK or VHP_ERR_MAX_ITER: every query of the curve runs its loop)


def groups(vhp, log):
    synth = import_module("visibility-heuristic-path-planner_amd.synth")
    maps = [("maze_6 690x402", synth.maze_6()), ("1000^2", synth.random_rect_map(1000, 1000, 15, 100, 200, 100, 200, seed=1)),
            ("4096^2", synth.random_rect_map(4096, 4096, 60, 100, 400, 100, 400, seed=1))]
    for name, occ in maps:
        c = vhp.Context(0)
        c.set_map(occ)
        pts = synth.free_sources(occ, 64, 5)
        queries = [tuple(int(v) for v in pts[2 * k]) + tuple(int(v) for v in pts[2 * k + 1]) for k in range(32)]
        c.planner_solve_batch(queries, 0.25, 1, outputs=False)
        log("group rule on %s (32 queries, max_iter 1): G = %d, sweep kernel %d" % (name, c.planner_batch_group(), c.last_sweep_kernel()))
        c.close()


def kernel_trace(d, log):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        log("no kernel_trace.csv under %s" % d)
        return
    by = {}
    for f in files:
        for row in csv.DictReader(open(f)):
            name = row.get("Kernel_Name", "")
            key = "batch epilogue" if "vhp_planner_batch_epilogue" in name else "latency sweep" if "vhp_lat_sweep" in name else None
            if key:
                by.setdefault(key, []).append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    for key, v in sorted(by.items()):
        us = np.array([t for _, t in sorted(v)])
        log("%-15s launches %6d  per launch us: mean %7.1f  median %7.1f  max %7.1f" % (key, len(us), us.mean(), np.median(us), us.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--q", default="1,2,4,8,16,32")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch-only", action="store_true")
    ap.add_argument("--kernel-trace", default=None)
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    if a.kernel_trace:
        kernel_trace(a.kernel_trace, log)
    else:
        import torch  # noqa: F401  (loaded first so the library shares its HIP runtime)
        import vhp_amd
        synth = import_module("visibility-heuristic-path-planner_amd.synth")
        occ = synth.maze_6()
        ctx = vhp_amd.Context(0)
        ctx.set_map(occ)
        log("batch planner on maze_6 (690x402), threshold 0.1, max_iter 250: config 4 + seeded free pairs (%s)" % vhp_amd.version())
        curve(ctx, occ, [int(v) for v in a.q.split(",")], a.reps, a.batch_only, log)
        if not a.batch_only:
            groups(vhp_amd, log)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
