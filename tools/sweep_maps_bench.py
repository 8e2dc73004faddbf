"""Throughput of the sweep over a stack of maps (vhp_sweep_maps_batch_device), in fields/s, against what the same work costs without it.

Cases (maps of one side, seeded synth.random_rect_map; sources from synth.free_sources, seeded per map):
  a  101^2, 4096 maps x 1 source     b  101^2, 256 maps x 16 sources     c  250^2, 256 maps x 1 source
  d  1000^2, 64 maps x 4 sources
For a-c the comparisons are (i) the same source positions on one map (map 0) through vhp_sweep_batch_device with "kernel" = 1 (the
same units and launch shape, one map), and (ii) the per-map loop a caller has without the stack: vhp_set_map_device + vhp_sweep_batch_device
per map (automatic kernel choice), one synchronisation at the end.  For d: the same positions on map 0 with the automatic choice.

Kernel time: vhp_timing's per-launch events (from the unit-ordering pre-kernel to the end of the sweep), median over the repetitions;
for the loop, the sum over its launches.  Wall time: per call (per whole loop), the repetitions back to back with one synchronisation
after the last, averaged.

usage: sweep_maps_bench.py [--cases abcd] [--reps N] [--loop-reps N] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
from importlib import import_module  # noqa: E402

CASES = {"a": (101, 4096, 1), "b": (101, 256, 16), "c": (250, 256, 1), "d": (1000, 64, 4)}


def stack_for(side, n_maps, per_map, seed=7):
    synth = import_module("visibility-heuristic-path-planner_amd.synth")
    nb = max(4, round(25 * (side / 101) ** 2))
    wmax = max(4, side // 5)
    occ = np.stack([synth.random_rect_map(side, side, nb, 2, wmax, 2, wmax, seed=seed + 31 * k) for k in range(n_maps)])
    src = np.concatenate([synth.free_sources(occ[k], per_map, seed=seed + 1 + 31 * k) for k in range(n_maps)])
    idx = np.repeat(np.arange(n_maps, dtype=np.int32), per_map)
    return occ, src, idx


def timed(ctx, launch, reps):
    """(median kernel ms per call, mean wall ms per call); launch() issues one call's work"""
    import torch
    launch()   # (warm-up: scratch allocations, first launches)
    torch.cuda.synchronize()
    ctx.timing_collect()
    ctx.timing(True, prealloc=8)
    per_call = []
    for _ in range(reps):
        launch()
        torch.cuda.synchronize()
        per_call.append(float(ctx.timing_collect(cap=1 << 16).sum()))
    t0 = time.perf_counter()
    for _ in range(reps):
        launch()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / reps
    ctx.timing(False)
    ctx.timing_collect()
    return float(np.median(per_call)), wall * 1e3


def run_case(vhp, name, reps, loop_reps, log):
    import torch
    side, n_maps, per_map = CASES[name]
    occ, src, idx = stack_for(side, n_maps, per_map)
    n = len(src)
    stream = torch.cuda.current_stream().cuda_stream
    d_occ = torch.from_numpy(occ).cuda()
    d_src = torch.from_numpy(src).cuda()
    d_idx = torch.from_numpy(idx).cuda()
    d_out = torch.empty((n, side, side), dtype=torch.float64, device="cuda")

    ctx = vhp.Context(0)
    ctx.set_stream(stream)
    t0 = time.perf_counter()
    ctx.set_maps_device(d_occ.data_ptr(), n_maps, side, side)
    set_ms = (time.perf_counter() - t0) * 1e3
    k_ms, w_ms = timed(ctx, lambda: ctx.sweep_maps_batch_device(d_src.data_ptr(), d_idx.data_ptr(), n, d_out.data_ptr()), reps)
    rows = [("stack", 1, k_ms, w_ms)]

    one = vhp.Context(0)
    one.set_stream(stream)
    one.set_map_device(d_occ.data_ptr(), side, side)   # (map 0)
    if name != "d":
        one.set_option("kernel", 1)
    k1, w1 = timed(one, lambda: one.sweep_batch_device(d_src.data_ptr(), n, d_out.data_ptr()), reps)
    rows.append(("one map, same positions" + (", kernel 1" if name != "d" else ", automatic"), one.last_sweep_kernel(), k1, w1))

    if name != "d":
        loop = vhp.Context(0)
        loop.set_stream(stream)

        def per_map_loop():
            for k in range(n_maps):
                loop.set_map_device(d_occ[k].data_ptr(), side, side)
                lo = k * per_map
                loop.sweep_batch_device(d_src[lo:].data_ptr(), per_map, d_out[lo:].data_ptr())
        kl, wl = timed(loop, per_map_loop, loop_reps)
        rows.append(("per-map loop (set_map_device + sweep_batch_device)", loop.last_sweep_kernel(), kl, wl))

    log("case %s: %d^2, %d maps x %d sources = %d fields (fp64); set_maps_device %.2f ms" % (name, side, n_maps, per_map, n, set_ms))
    log("  %-52s %6s %10s %14s %10s %14s" % ("", "kernel", "kernel ms", "fields/s", "wall ms", "fields/s"))
    for what, kern, km, wm in rows:
        log("  %-52s %6d %10.3f %14.0f %10.3f %14.0f" % (what, kern, km, n / km * 1e3, wm, n / wm * 1e3))
    for what, _, km, wm in rows[1:]:
        log("  stack's fields/s over %s's: kernel %.2fx, wall %.2fx" % (what.split(" (")[0], km / k_ms, wm / w_ms))
    del d_out
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abcd")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (first, so the extension shares torch's HIP runtime)
    import vhp_amd
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log("sweep over a stack of maps (%s); kernel ms: median of %d (loop: %d), wall ms: mean per call" % (vhp_amd.version(), a.reps, a.loop_reps))
    for name in a.cases:
        run_case(vhp_amd, name, a.reps, a.loop_reps, log)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
