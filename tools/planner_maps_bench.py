"""The batch planner across a stack of maps (vhp_planner_solve_maps_batch) against what it replaces, wall clock per call (every call ends
in a synchronisation of the context's stream), every shape warmed up first, median of --reps calls, the two sides of each comparison
alternated call by call in one process:
  (a) the cost of a map per source: Q = 16 and 32 queries (config 4 + seeded free pairs, planner_batch_bench.py's) on a stack of Q
      copies of maze_6, map_idx = 0..Q-1, against planner_solve_batch of the same queries on maze_6 (threshold 0.1, max_iter 250);
  (b) the reference's own evaluation (MATLAB_code/f_comparison_to_a_star.m: start (5, 5) -> end (95, 95) on freshly generated 100 x 100
      random environments): 64 seeded 100 x 100 random-rectangle maps, that query on each, threshold 0.25, against a loop of
      set_map_device + planner_solve_device per map;
  (c) a larger grid: 16 maps of 1000^2 x 2 queries, threshold 0.25, max_iter 40, against the same loop per query.

usage: planner_maps_bench.py [--reps N] [--out FILE] [--only a|b|c] [--kernel-trace DIR]
  --only           run one case (a run under rocprofv3 --kernel-trace: --only a --stack-only, so that the trace holds the stack's launches)
  --stack-only     no comparison side
  --kernel-trace   DIR: read the *kernel_trace.csv a rocprofv3 --kernel-trace run left under DIR and report the per-launch times of the
                   map-stack latency sweep, the one-map latency sweep and the batch epilogue (nothing is run on the GPU)"""
import argparse
import csv
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
from importlib import import_module  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def alternate(sides, reps):
    """{name: fn}: each warmed up, then called in turn reps times; {name: median seconds}"""
    for fn in sides.values():
        fn()
    ts = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            ts[k].append(timed(fn))
    return {k: float(np.median(v)) for k, v in ts.items()}


def case_a(vhp, synth, reps, stack_only, log):
    from planner_batch_bench import queries_for
    occ = synth.maze_6()
    log("(a) Q queries on a stack of Q copies of maze_6 (690x402, map_idx 0..Q-1) vs planner_solve_batch on maze_6; thr 0.1, max_iter 250")
    log("Q   G   pivots  stack ms  one-map ms  stack/one-map")
    for q in (16, 32):
        queries = queries_for(occ, q)
        cs = vhp.Context(0)
        cs.set_maps(np.stack([occ] * q))
        idx = list(range(q))
        c1 = vhp.Context(0)
        c1.set_map(occ)
        res = cs.planner_solve_maps_batch(queries, idx, 0.1, 250, outputs=False)
        n_piv = sum(r["n_pivots"] for r in res)

        def stack():
            cs.planner_solve_maps_batch(queries, idx, 0.1, 250, outputs=False)
            cs.sync()

        def one():
            c1.planner_solve_batch(queries, 0.1, 250, outputs=False)
            c1.sync()
        sides = {"stack": stack} if stack_only else {"stack": stack, "one": one}
        t = alternate(sides, reps)
        if stack_only:
            log("%-3d %-3d %6d  %8.3f" % (q, cs.planner_maps_batch_group(), n_piv, t["stack"] * 1e3))
        else:
            assert [r["n_pivots"] for r in c1.planner_solve_batch(queries, 0.1, 250, outputs=False)] == [r["n_pivots"] for r in res]
            log("%-3d %-3d %6d  %8.3f  %10.3f  %6.3fx" % (q, cs.planner_maps_batch_group(), n_piv, t["stack"] * 1e3, t["one"] * 1e3,
                                                       t["stack"] / t["one"]))
        cs.close()
        c1.close()


def loop_vs_stack(vhp, stack, queries, idx, thr, max_iter, reps, stack_only, log, label):
    import torch
    m, ny, nx = stack.shape
    d_stack = torch.from_numpy(np.ascontiguousarray(stack, np.uint8)).cuda()
    cs = vhp.Context(0)
    cs.set_maps_device(d_stack.data_ptr(), m, nx, ny)
    cl = vhp.Context(0)
    res = cs.planner_solve_maps_batch(queries, idx, thr, max_iter, outputs=False)
    n_piv = sum(r["n_pivots"] for r in res)

    def stack_call():
        cs.planner_solve_maps_batch(queries, idx, thr, max_iter, outputs=False)
        cs.sync()

    def loop():
        n = 0
        for (sx, sy, ex, ey), k in zip(queries, idx):
            cl.set_map_device(d_stack.data_ptr() + k * nx * ny, nx, ny)
            n += cl.planner_solve_device((sx, sy), (ex, ey), thr, max_iter)[1]
        cl.sync()
        return n
    sides = {"stack": stack_call} if stack_only else {"stack": stack_call, "loop": loop}
    t = alternate(sides, reps)
    if not stack_only:
        assert loop() == n_piv
    log("%s: %d queries on %d maps, %d pivots, G %d, kernel %d: stack %.3f ms%s" % (
        label, len(queries), m, n_piv, cs.planner_maps_batch_group(), cs.last_sweep_kernel(), t["stack"] * 1e3,
        "" if stack_only else "  per-map loop %.3f ms  loop/stack %.2fx" % (t["loop"] * 1e3, t["loop"] / t["stack"])))
    st = sorted(set(r["status"] for r in res))
    log("    statuses %r" % st)
    cs.close()
    cl.close()


def case_b(vhp, synth, reps, stack_only, log):
    maps = []
    for seed in range(64):
        occ = synth.random_rect_map(100, 100, 25, 2, 20, 2, 20, seed=100 + seed)
        occ[5, 5] = occ[95, 95] = 1
        maps.append(occ)
    stack = np.stack(maps)
    loop_vs_stack(vhp, stack, [(5, 5, 95, 95)] * 64, list(range(64)), 0.25, 250, reps, stack_only, log,
                  "(b) 64 random 100x100 maps, (5,5) -> (95,95), thr 0.25, max_iter 250")


def case_c(vhp, synth, reps, stack_only, log):
    stack = np.stack([synth.random_rect_map(1000, 1000, 15, 60, 200, 60, 200, seed=200 + k) for k in range(16)])
    queries, idx = [], []
    for k in range(16):
        pts = synth.free_sources(stack[k], 4, 7 + k)
        queries += [tuple(int(v) for v in pts[0]) + tuple(int(v) for v in pts[1]), tuple(int(v) for v in pts[2]) + tuple(int(v) for v in pts[3])]
        idx += [k, k]
    loop_vs_stack(vhp, stack, queries, idx, 0.25, 40, reps, stack_only, log, "(c) 16 random 1000^2 maps x 2 queries, thr 0.25, max_iter 40")


def kernel_trace(d, log):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        log("no kernel_trace.csv under %s" % d)
        return
    by = {}
    for f in files:
        for row in csv.DictReader(open(f)):
            name = row.get("Kernel_Name", "")
            key = ("batch epilogue" if "vhp_planner_batch_epilogue" in name else "map-stack sweep" if "vhp_lat_maps_sweep" in name
                   else "latency sweep" if "vhp_lat_sweep" in name else None)
            if key:
                by.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    for key, v in sorted(by.items()):
        us = np.array(v)
        log("%-16s launches %6d  per launch us: mean %7.1f  median %7.1f  max %7.1f" % (key, len(us), us.mean(), np.median(us), us.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="abc")
    ap.add_argument("--stack-only", action="store_true")
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
        log("batch planner across a stack of maps (%s), median of %d calls, sides alternated" % (vhp_amd.version(), a.reps))
        for key, fn in (("a", case_a), ("b", case_b), ("c", case_c)):
            if key in a.only:
                fn(vhp_amd, synth, a.reps, a.stack_only, log)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
