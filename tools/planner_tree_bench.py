#!/usr/bin/env python3
"""From a batch solve to path lengths at many goals and to whole length fields: the device route (vhp_planner_goal_paths,
vhp_planner_length_fields) against the route it replaces (per query vhp_planner_[maps_]batch_results(came_from, pivots only), then one
vhp_reconstruct_path call per goal).  A diagnostic, not bench.py: wall clock per call ending in a synchronisation, every shape warmed
up, median of --reps (11), the two sides alternated (a process each, two rounds).  Both sides run on this tree's library: the old
route's entry points are older than the tree calls and unchanged by them.
The old route's whole field is nx * ny host calls per query; it is timed on --field-sample cells per query and scaled to the field,
and marked so.  The new side also times the field kernel's device form into a buffer whose store-probe rates (vhp_probe_stores, as
bench.py reports them) are printed beside the bytes it moves: 12 bytes per cell out, 4 in.
--side profile runs the 1000 x 1000 field call alone, for `rocprofv3 --kernel-trace --stats -- python tools/planner_tree_bench.py
--side profile` in a run of its own.  --out profiles/planner_tree.txt."""
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
GOALS = (1, 64, 4096)


def cases(synth, which):
    out = []
    if which in ("all", "maze"):
        occ = synth.maze_6()
        ny = occ.shape[0]
        c4 = (345, ny - 1 - 391, 341, ny - 1 - 10)
        pts = synth.free_sources(occ, 62, 7)
        free = [tuple(int(v) for v in pts[2 * k]) + tuple(int(v) for v in pts[2 * k + 1]) for k in range(31)]
        out.append(("maze_6 Q=32 thr 0.1", occ[None], [c4] + free, [0] * 32, 0.1, 250))
    if which in ("all", "big"):
        big = np.stack([synth.random_rect_map(1000, 1000, 15, 60, 200, 60, 200, seed=200 + k) for k in range(16)])
        qs = []
        for k in range(16):
            p = synth.free_sources(big[k], 2, 3 + k)
            qs.append(tuple(int(v) for v in p[0]) + tuple(int(v) for v in p[1]))
        out.append(("16 random 1000x1000 maps thr 0.25", big, qs, list(range(16)), 0.25, 60))
    return out


def side(args):
    """One side in a process of its own: prints RESULT lines."""
    import torch
    import vhp_amd
    from importlib import import_module
    synth = import_module("visibility-heuristic-path-planner_amd.synth")
    lib = vhp_amd.load_library()
    vp = C.c_void_p

    def ptr(a):
        return a.ctypes.data_as(vp)

    def med(fn, reps):
        fn(); fn()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); t.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(t)

    for label, stack, queries, idx, thr, max_iter in cases(synth, "big" if args.side == "profile" else "all"):
        c = vhp_amd.Context(0)
        c.set_maps(stack)
        ny, nx = stack.shape[1:]
        q = np.ascontiguousarray(queries, np.int32)
        n = len(q)
        st, npiv = np.zeros(n, np.int32), np.zeros(n, np.uint32)
        c._check(lib.vhp_planner_solve_maps_batch(c.h, ptr(q), ptr(np.ascontiguousarray(idx, np.int32)), ptr(np.full(n, thr, np.float64)), n, max_iter,
                                                  ptr(st), ptr(npiv)))
        cap = int(npiv.max()) + 3
        rng = np.random.default_rng(1)
        if args.side == "profile":
            d_len = torch.empty(n * ny * nx, dtype=torch.float64, device="cuda")
            d_cnt = torch.empty(n * ny * nx, dtype=torch.int32, device="cuda")
            for _ in range(5):
                c.planner_length_fields_device(d_len.data_ptr(), d_cnt.data_ptr(), "maps")
                c.sync()
            continue
        for g in GOALS:
            goals = np.ascontiguousarray([(k, int(rng.integers(0, nx)), int(rng.integers(0, ny))) for k in range(n) for _ in range(g)], np.int32)
            cnt, ln, ps = np.zeros(len(goals), np.uint32), np.zeros(len(goals)), np.zeros(len(goals), np.int32)
            if args.side == "new":
                xy = np.zeros((len(goals), cap, 2), np.int32)
                ms = med(lambda: c._check(lib.vhp_planner_goal_paths(c.h, 2, ptr(goals), len(goals), ptr(xy), cap, ptr(cnt), ptr(ln), ptr(ps))), args.reps)
                print("RESULT|%s|%d goals per query|new|%.3f|%d" % (label, g, ms, int((ps == 0).sum())), flush=True)
            else:
                came, piv, xy1 = np.empty((ny, nx), np.uint64), np.zeros((cap, 2), np.int32), np.zeros((cap, 2), np.int32)

                def old():
                    k, d = C.c_uint32(0), C.c_double(0)
                    for qq in range(n):
                        if st[qq] in (0, 3, 20):
                            c._check(lib.vhp_planner_maps_batch_results(c.h, qq, ptr(came), None, None, ptr(piv)))
                            for _, x, y in goals[qq * g: (qq + 1) * g]:
                                lib.vhp_reconstruct_path(ptr(came), ptr(piv), int(npiv[qq]), nx, ny, int(x), int(y), ptr(xy1), cap, C.byref(k), C.byref(d))
                ms = med(old, max(3, args.reps // 3) if g > 64 else args.reps)
                print("RESULT|%s|%d goals per query|old|%.3f|-1" % (label, g, ms), flush=True)
        # the whole field
        if args.side == "new":
            length, cnt = np.empty((n, ny, nx), np.float64), np.empty((n, ny, nx), np.uint32)
            ms = med(lambda: c._check(lib.vhp_planner_length_fields(c.h, 2, 0, n, ptr(length), ptr(cnt))), args.reps)
            print("RESULT|%s|whole field, host form|new|%.3f|%d" % (label, ms, int((cnt > 0).sum())), flush=True)
            bytes_out = 12 * n * ny * nx
            d_buf = torch.empty(max(bytes_out, 128 << 20) // 8, dtype=torch.float64, device="cuda")
            d_len, d_cnt = d_buf.data_ptr(), d_buf.data_ptr() + 8 * n * ny * nx

            def dev():
                c.planner_length_fields_device(d_len, d_cnt, "maps")
                c.sync()
            ms = med(dev, args.reps)
            whole, split = c.probe_stores(d_buf.data_ptr(), d_buf.numel() * 8)
            moved = 16 * n * ny * nx
            print("RESULT|%s|whole field, device form (%d bytes moved; buffer probes %.2f / %.2f TB/s whole / split lines: %.3f ms at the whole-line rate)"
                  "|new|%.3f|-1" % (label, moved, whole, split, moved / (whole * 1e9) if whole > 0 else float("nan"), ms), flush=True)
        else:
            s = args.field_sample
            cells = [(int(rng.integers(0, nx)), int(rng.integers(0, ny))) for _ in range(s)]
            came, piv = np.empty((ny, nx), np.uint64), np.zeros((cap, 2), np.int32)

            def old_field():
                k, d = C.c_uint32(0), C.c_double(0)
                for qq in range(n):
                    if st[qq] in (0, 3, 20):
                        c._check(lib.vhp_planner_maps_batch_results(c.h, qq, ptr(came), None, None, ptr(piv)))
                        for x, y in cells:
                            lib.vhp_reconstruct_path(ptr(came), ptr(piv), int(npiv[qq]), nx, ny, x, y, None, 0, C.byref(k), C.byref(d))

            def copies():
                for qq in range(n):
                    if st[qq] in (0, 3, 20):
                        c._check(lib.vhp_planner_maps_batch_results(c.h, qq, ptr(came), None, None, ptr(piv)))
            t_all, t_copy = med(old_field, 3), med(copies, 3)
            ms = t_copy + (t_all - t_copy) * (nx * ny / s)
            print("RESULT|%s|whole field, host form|old (scaled from %d cells per query)|%.3f|-1" % (label, s, ms), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--field-sample", type=int, default=16384)
    ap.add_argument("--out", default=None)
    ap.add_argument("--side", choices=("old", "new", "profile"), default=None)
    args = ap.parse_args()
    if args.side:
        return side(args)
    rows = {}
    for s in ("old", "new", "old", "new"):   # (the two sides alternated: two rounds each, the better median kept per row)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--side", s, "--reps", str(args.reps), "--field-sample", str(args.field_sample)],
                           capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.exit("side %s failed (exit %d):\n%s" % (s, p.returncode, p.stderr[-3000:]))
        for line in p.stdout.splitlines():
            if line.startswith("RESULT|"):
                _, label, what, sd, ms, ok = line.split("|")
                key = (label, what.split(" (")[0])
                cur = rows.setdefault(key, {}).get(sd[:3])
                if cur is None or float(ms) < cur[0]:
                    rows[key][sd[:3]] = (float(ms), int(ok), what, sd)
    out = ["# tools/planner_tree_bench.py: ms per call (median of %d, wall clock, each call ends in a synchronisation)" % args.reps,
           "# old = per query results(came_from, pivots) + vhp_reconstruct_path per goal; new = one vhp_planner_goal_paths / _length_fields call",
           "# case | what | old ms | new ms | goals or cells with a path (new)"]
    for (label, _), r in rows.items():
        o, n = r.get("old"), r.get("new")
        what = (n or o)[2]
        out.append("%s | %s | %s | %s | %s" % (label, what, ("%.3f%s" % (o[0], " " + o[3][4:] if len(o[3]) > 3 else "")) if o else "-",
                                             "%.3f" % n[0] if n else "-", n[1] if n else "-"))
    text = "\n".join(out) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
