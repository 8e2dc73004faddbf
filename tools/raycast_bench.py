"""Ray casting for a batch of sources (vhp_raycast_batch_device) against the one-source entry point it stands beside, and against the sweep.

Workload: the C3 map (1000^2, 50 rectangles, map seed 1) and the benchmark's 256 seeded sources (synth.config_c3); one further line for
the C5 map (4096^2) with 16 sources.
  batch     one vhp_raycast_batch_device call per dtype (fp64, fp32, uint8), timed by vhp_last_elapsed_ms: fill plus kernel
  baseline  the same sources one at a time through the unchanged vhp_raycast_all; the sum of its vhp_last_elapsed_ms, which is fill plus
            kernel as well (its 8 bytes per cell to the host are NOT in that time)
  sweep     vhp_sweep_batch_device on the same sources (fp64, automatic kernel), vhp_last_elapsed_ms -- the ratio ray casting / sweep is the
            figure the reference's benchmark() prints (src/visibilityBasedSolver.cpp:247-249)
After one warm-up of each, the three alternate `--rounds` times in one process; reported are the median and the spread (min .. max).

usage: raycast_bench.py [--rounds N] [--out FILE]      the table
       raycast_bench.py --profile [--dtype 0|1|2]      the batch call alone, three times (for a kernel trace in a run of its own)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
from importlib import import_module  # noqa: E402

DTYPES = {0: "fp64", 1: "fp32", 2: "uint8"}


def med(v):
    return "%9.3f (%.3f .. %.3f)" % (float(np.median(v)), min(v), max(v))


def run(vhp, occ, src, rounds, log, what):
    import torch
    ny, nx = occ.shape
    n = len(src)
    tdt = {0: torch.float64, 1: torch.float32, 2: torch.uint8}
    ctx = vhp.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_map(occ)
    d_src = torch.from_numpy(np.ascontiguousarray(src, np.int32)).cuda()
    d_out = torch.empty((n, ny, nx), dtype=torch.float64, device="cuda")   # (the fp32 and uint8 fields use its first bytes)

    def batch(dtype):
        ctx.raycast_batch_device(d_src.data_ptr(), n, d_out.data_ptr(), dtype)
        return ctx.last_elapsed_ms()

    def baseline():
        total = 0.0
        for x, y in src:
            ctx.raycast_all(int(x), int(y))
            total += ctx.last_elapsed_ms()
        return total

    def sweep():
        ctx.sweep_batch_device(d_src.data_ptr(), n, d_out.data_ptr())
        return ctx.last_elapsed_ms()

    # the results first: the batch's fp64 fields are the one-source entry point's, byte for byte
    batch(vhp.F64)
    ctx.sync()
    for k in sorted({0, n // 2, n - 1}):
        assert d_out[k].cpu().numpy().tobytes() == ctx.raycast_all(int(src[k][0]), int(src[k][1])).tobytes(), "field %d differs" % k
    for dtype in DTYPES:
        batch(dtype)
    baseline()
    sweep()
    t = {("batch", d): [] for d in DTYPES}
    t["baseline"], t["sweep"] = [], []
    for _ in range(rounds):
        for d in DTYPES:
            t[("batch", d)].append(batch(d))
        t["baseline"].append(baseline())
        t["sweep"].append(sweep())
    log("%s: %d x %d, %d sources; ms, median (min .. max) of %d alternating rounds" % (what, nx, ny, n, rounds))
    for d, name in DTYPES.items():
        log("  batch %-5s                      %s   per source %.4f" % (name, med(t[("batch", d)]), np.median(t[("batch", d)]) / n))
    log("  vhp_raycast_all x %-4d (fp64)     %s   per source %.4f" % (n, med(t["baseline"]), np.median(t["baseline"]) / n))
    log("  sweep batch (fp64, kernel %d)     %s   per source %.4f" % (ctx.last_sweep_kernel(), med(t["sweep"]), np.median(t["sweep"]) / n))
    b, o, s = (float(np.median(t[k])) for k in (("batch", 0), "baseline", "sweep"))
    log("  one-source calls / batch fp64: %.2fx; ray casting (batch fp64) / sweep: %.1fx; ray casting (one-source calls) / sweep: %.1fx" % (o / b, b / s, o / s))
    del d_out
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--dtype", type=int, default=0, choices=sorted(DTYPES))
    a = ap.parse_args()
    import torch  # (first, so the extension shares torch's HIP runtime)
    import vhp_amd
    synth = import_module("visibility-heuristic-path-planner_amd.synth")
    if a.profile:
        occ, src = synth.config_c3(256)
        ctx = vhp_amd.Context(0)
        ctx.set_map(occ)
        d_src = torch.from_numpy(src).cuda()
        d_out = torch.empty((len(src),) + occ.shape, dtype=torch.float64, device="cuda")
        for _ in range(3):
            ctx.raycast_batch_device(d_src.data_ptr(), len(src), d_out.data_ptr(), a.dtype)
            ctx.sync()
            print("batch %s: %.3f ms" % (DTYPES[a.dtype], ctx.last_elapsed_ms()))
        return
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log("ray casting for a batch of sources (%s)" % vhp_amd.version())
    run(vhp_amd, *synth.config_c3(256), a.rounds, log, "C3")
    run(vhp_amd, *synth.config_c5(16), a.rounds, log, "C5 map")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
