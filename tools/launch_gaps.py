"""What a pool-sweep launch spends outside its sweep kernel, from a rocprofv3 kernel trace: per step of the timed region the sweep
kernel, the idle time between the end of the previous sweep and the start of this step's order kernel, the order kernel, the gap
from the order kernel to the sweep, and the period (end of sweep to end of sweep).
usage: launch_gaps.py table <kernel_trace.csv> <warmup> <steps> [label]   the table of launches warmup+1 .. warmup+steps
       launch_gaps.py run <timing 0|1> [warmup steps]                     the C3 launches alone (256 sources at 1000^2, fp64) through
                                                                          vhp_sweep_batch_device, vhp_timing on or off: what to trace
                                                                          beside bench.py, whose timed regions always have it on
(VHP_LIB in the environment picks the library, as everywhere.)"""
import csv, os, sys


def table(path, warm, steps, label):
    rows = [r for r in csv.DictReader(open(path)) if "vhp_pool_sweep" in r["Kernel_Name"] or "vhp_pool_order" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    seq = [("order" if "vhp_pool_order" in r["Kernel_Name"] else "sweep", int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows]
    # a launch = an order kernel and the sweep behind it
    launches = [(seq[i], seq[i + 1]) for i in range(len(seq) - 1) if seq[i][0] == "order" and seq[i + 1][0] == "sweep"]
    cols = {"sweep": [], "idle before order": [], "order": [], "order -> sweep": [], "period": []}
    for k in range(max(warm, 1), min(warm + steps, len(launches))):
        (_, o0, o1), (_, s0, s1) = launches[k]
        prev_end = launches[k - 1][1][2]
        cols["sweep"].append((s1 - s0) / 1e3)
        cols["idle before order"].append((o0 - prev_end) / 1e3)
        cols["order"].append((o1 - o0) / 1e3)
        cols["order -> sweep"].append((s0 - o1) / 1e3)
        cols["period"].append((s1 - prev_end) / 1e3)
    n = len(cols["sweep"])
    print("%s: %d launches in the trace, launches %d..%d tabulated (us)" % (label, len(launches), max(warm, 1) + 1, max(warm, 1) + n))
    print("  %-18s %9s %9s %9s %9s" % ("piece of one step", "median", "mean", "min", "max"))
    for name, v in cols.items():
        s = sorted(v)
        print("  %-18s %9.1f %9.1f %9.1f %9.1f" % (name, s[len(s) // 2], sum(s) / len(s), s[0], s[-1]))
    out = sorted(cols["period"][i] - cols["sweep"][i] for i in range(n))
    print("  %-18s %9.1f %9.1f %9.1f %9.1f" % ("period - sweep", out[n // 2], sum(out) / n, out[0], out[-1]))


def run(timing, warm, steps):
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    import numpy as np, torch
    from importlib import import_module
    mod = import_module("visibility-heuristic-path-planner_amd")
    synth = import_module("visibility-heuristic-path-planner_amd.synth")
    occ, src = synth.config_c3(256)
    d_src = torch.from_numpy(np.ascontiguousarray(src, np.int32)).cuda()
    out = torch.empty((256, 1000, 1000), dtype=torch.float64, device="cuda")
    c = mod.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    c.set_map(occ)
    for _ in range(warm):
        c.sweep_batch_device(d_src.data_ptr(), 256, out.data_ptr())
    torch.cuda.synchronize()
    if timing:
        c.timing(True, prealloc=steps + 2)
    for _ in range(steps):
        c.sweep_batch_device(d_src.data_ptr(), 256, out.data_ptr())
    torch.cuda.synchronize()
    c.sync()
    print("%d + %d launches of kernel %d, vhp_timing %s, library %s" % (warm, steps, c.last_sweep_kernel(), "on" if timing else "off", mod.LIB_PATH))


if sys.argv[1] == "table":
    table(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5] if len(sys.argv) > 5 else os.path.basename(sys.argv[2]))
else:
    run(int(sys.argv[2]) != 0, int(sys.argv[3]) if len(sys.argv) > 3 else 5, int(sys.argv[4]) if len(sys.argv) > 4 else 25)
