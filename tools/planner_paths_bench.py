#!/usr/bin/env python3
"""From a batch solve to the paths: the device route (solve + vhp_planner_[maps_]batch_paths) against the route it replaces (solve +
per query vhp_planner_[maps_]batch_results(came_from, pivots only) + vhp_reconstruct_path).  A diagnostic, not bench.py: wall clock per
call ending in a synchronisation, every shape warmed up, median of --reps (11), the two sides alternated (a process each, two rounds).
Both sides run on this tree's library: the old route's entry points are older than the path calls and unchanged by them (the package
refuses a library that lacks a symbol of the ABI, so an older build cannot be loaded through it).  --out profiles/planner_paths.txt."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def side(args):
    """One side in a process of its own (its library is chosen when the package is imported): prints `case ms ms ...` lines."""
    import torch  # noqa: F401
    import vhp_amd
    from importlib import import_module
    synth = import_module("visibility-heuristic-path-planner_amd.synth")
    lib = vhp_amd.load_library()
    new = args.side == "new"
    vp = C.c_void_p

    def ptr(a):
        return a.ctypes.data_as(vp)

    def run(label, c, solve, nx, ny, results, paths, queries, reps):
        n = len(queries)
        st, npiv = solve()
        cap = int(npiv.max()) + 3
        xy, cnt, ln, ps = np.zeros((n, cap, 2), np.int32), np.zeros(n, np.uint32), np.zeros(n), np.zeros(n, np.int32)
        came, piv = np.empty((ny, nx), np.uint64), np.zeros((cap, 2), np.int32)

        def old_route():
            k, d = C.c_uint32(0), C.c_double(0)
            for q in range(n):
                if st[q] in (0, 3, 20):
                    c._check(results(c.h, q, ptr(came), None, None, ptr(piv)))
                    lib.vhp_reconstruct_path(ptr(came), ptr(piv), int(npiv[q]), nx, ny, int(queries[q][2]), int(queries[q][3]), ptr(xy[q]), cap,
                                             C.byref(k), C.byref(d))

        def new_route():
            c._check(paths(c.h, ptr(xy), cap, ptr(cnt), ptr(ln), ptr(ps)))

        route = new_route if new else old_route
        t = {"solve": [], "solve+paths": [], "paths": []}
        for r in range(reps + 2):   # (two warm-up rounds)
            t0 = time.perf_counter(); solve(); t1 = time.perf_counter(); route(); t2 = time.perf_counter()
            solve(); t3 = time.perf_counter()
            if r >= 2:
                t["solve+paths"].append(1e3 * (t2 - t0)); t["paths"].append(1e3 * (t2 - t1)); t["solve"].append(1e3 * (t3 - t2))
        moved = n * (8 * cap + 16) if new else int(sum(8 * nx * ny + 8 * (int(npiv[q]) + 1) for q in range(n) if st[q] in (0, 3, 20)))
        print("RESULT|%s|%s|%.3f|%.3f|%.3f|%d|%d" % (label, args.side, statistics.median(t["solve"]), statistics.median(t["solve+paths"]),
                                                     statistics.median(t["paths"]), moved, int((ps == 0).sum()) if new else -1), flush=True)

    def batch(label, occ, queries, thr, max_iter, reps):
        c = vhp_amd.Context(0)
        c.set_map(occ)
        q = np.ascontiguousarray(queries, np.int32)
        n = len(q)
        t = np.ascontiguousarray(np.broadcast_to(np.float64(thr), (n,)))
        st, npiv = np.zeros(n, np.int32), np.zeros(n, np.uint32)

        def solve():
            c._check(lib.vhp_planner_solve_batch(c.h, ptr(q), ptr(t), n, max_iter, ptr(st), ptr(npiv)))
            return st, npiv
        run(label, c, solve, c.nx, c.ny, lib.vhp_planner_batch_results, getattr(lib, "vhp_planner_batch_paths", None), q, reps)

    def maps_batch(label, stack, queries, idx, thr, max_iter, reps):
        c = vhp_amd.Context(0)
        c.set_maps(stack)
        q = np.ascontiguousarray(queries, np.int32)
        n = len(q)
        ix = np.ascontiguousarray(idx, np.int32)
        t = np.ascontiguousarray(np.broadcast_to(np.float64(thr), (n,)))
        st, npiv = np.zeros(n, np.int32), np.zeros(n, np.uint32)

        def solve():
            c._check(lib.vhp_planner_solve_maps_batch(c.h, ptr(q), ptr(ix), ptr(t), n, max_iter, ptr(st), ptr(npiv)))
            return st, npiv
        run(label, c, solve, c.maps_nx, c.maps_ny, lib.vhp_planner_maps_batch_results, getattr(lib, "vhp_planner_maps_batch_paths", None), q, reps)

    occ = synth.maze_6()
    ny = occ.shape[0]
    c4 = (345, ny - 1 - 391, 341, ny - 1 - 10)
    pts = synth.free_sources(occ, 62, 7)
    free = [tuple(int(v) for v in pts[2 * k]) + tuple(int(v) for v in pts[2 * k + 1]) for k in range(31)]
    for n in (16, 32):
        batch("maze_6 Q=%d thr 0.1" % n, occ, [c4] + free[: n - 1], 0.1, 250, args.reps)
    stack = []
    for s in range(64):
        m = synth.random_rect_map(100, 100, 25, 2, 20, 2, 20, seed=100 + s)
        m[5, 5] = m[95, 95] = 1
        stack.append(m)
    maps_batch("64 random 100x100 maps (5,5)->(95,95) thr 0.25", np.stack(stack), [(5, 5, 95, 95)] * 64, list(range(64)), 0.25, 250, args.reps)
    big = np.stack([synth.random_rect_map(1000, 1000, 15, 60, 200, 60, 200, seed=200 + k) for k in range(16)])
    qs, ix = [], []
    for k in range(16):
        p = synth.free_sources(big[k], 4, 3 + k)
        qs += [tuple(int(v) for v in p[0]) + tuple(int(v) for v in p[1]), tuple(int(v) for v in p[2]) + tuple(int(v) for v in p[3])]
        ix += [k, k]
    maps_batch("16 random 1000x1000 maps x 2 queries thr 0.25", big, qs, ix, 0.25, 60, max(3, args.reps // 2))
    if new:   # the paths call alone on solves that commit hundreds to thousands of pivots (the live-lock of threshold 0.25)
        for max_iter in (250, 2000):
            batch("maze_6 config 4 thr 0.25 max_iter %d (paths call alone: see the paths column)" % max_iter, occ, [c4], 0.25, max_iter, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=None)
    ap.add_argument("--side", choices=("old", "new"), default=None)
    args = ap.parse_args()
    if args.side:
        return side(args)
    rows = {}
    for s in ("old", "new", "old", "new"):   # (the two sides alternated: two rounds each, the better median kept per row)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--side", s, "--reps", str(args.reps)], capture_output=True,
                           text=True, timeout=900)
        if p.returncode != 0:
            sys.exit("side %s failed (exit %d):\n%s" % (s, p.returncode, p.stderr[-3000:]))
        for line in p.stdout.splitlines():
            if line.startswith("RESULT|"):
                _, label, sd, solve, both, paths, moved, ok = line.split("|")
                cur = rows.setdefault(label, {}).get(sd)
                if cur is None or float(both) < cur[1]:
                    rows[label][sd] = (float(solve), float(both), float(paths), int(moved), int(ok))
    out = ["# tools/planner_paths_bench.py: ms per call (median of %d, wall clock, each call ends in a synchronisation)" % args.reps,
           "# old = solve + per query results(came_from, pivots) + vhp_reconstruct_path; new = solve + the batch paths call",
           "# case | solve alone | old solve+paths | new solve+paths | old paths part | new paths call | old bytes to host | new bytes to host | paths with status 0"]
    for label, r in rows.items():
        o, n = r.get("old"), r.get("new")
        out.append("%s | %.3f | %s | %.3f | %s | %.3f | %s | %d | %d" % (label, n[0], "%.3f" % o[1] if o else "-", n[1], "%.3f" % o[2] if o else "-",
                                                                       n[2], o[3] if o else "-", n[3], n[4]))
    text = "\n".join(out) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
