"""Windows of the map as a stack of maps: the cut on the device (vhp_set_maps_windows_device) against the routes that hand the stack bytes.

Workloads: a 2000^2 map with 5 % blocked cells and 4096 windows of 101^2 at seeded random origins (some hang over the edges), then a
4000^2 map and 256 windows of 1001^2.
  (a) windows   vhp_set_maps_windows_device, the origins resident on the device
  (b) bytes     vhp_set_maps_device on the same windows already resident as bytes: the byte route's best case, no PCIe in it
  (c) host      the windows cut on the host with numpy, then vhp_set_maps (the first workload only)
None of these is timed by vhp_last_elapsed_ms: the host clock is put around each call, which ends in the stream synchronise that leaves
the stack on the device.  After two warm-ups of each, the candidates alternate `--rounds` times in one process; reported are the median
and the spread (min .. max).  Before any timing the three stacks are read back (vhp_maps_occupancy_device) and compared byte for byte.

usage: windows_bench.py [--rounds N] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def med(v):
    return "%9.3f (%.3f .. %.3f)" % (float(np.median(v)), min(v), max(v))


def numpy_cut(occ, origin_xy, side):
    """the windows as bytes [n, side, side], blocked outside the grid: what a caller of vhp_set_maps has to make on the host"""
    ny, nx = occ.shape
    padded = np.zeros((ny + 2 * side, nx + 2 * side), np.uint8)
    padded[side: side + ny, side: side + nx] = occ
    out = np.empty((len(origin_xy), side, side), np.uint8)
    for k, (x, y) in enumerate(origin_xy):
        out[k] = padded[y + side: y + 2 * side, x + side: x + 2 * side]
    return out


def run(vhp, n_side, n_win, side, rounds, with_host, log):
    import torch
    rng = np.random.default_rng(n_side + side)
    occ = (rng.random((n_side, n_side)) >= 0.05).astype(np.uint8)
    origin_xy = rng.integers(-(side // 2), n_side - side // 2, (n_win, 2)).astype(np.int32)   # (inside the padding of numpy_cut)
    ctx = vhp.Context(0)
    ctx.set_map(occ)
    d_origin = torch.from_numpy(origin_xy).cuda()
    d_bytes = torch.empty((n_win, side, side), dtype=torch.uint8, device="cuda")
    d_check = torch.empty_like(d_bytes)

    def windows():
        t0 = time.perf_counter()
        ctx.set_maps_windows_device(d_origin.data_ptr(), n_win, side, side)
        return (time.perf_counter() - t0) * 1e3

    def from_bytes():
        t0 = time.perf_counter()
        ctx.set_maps_device(d_bytes.data_ptr(), n_win, side, side)
        return (time.perf_counter() - t0) * 1e3

    def host():
        t0 = time.perf_counter()
        ctx.set_maps(numpy_cut(occ, origin_xy, side))
        return (time.perf_counter() - t0) * 1e3

    # the results first: the three routes leave the same stack
    windows()
    ctx.maps_occupancy_device(d_bytes.data_ptr())
    ctx.sync()
    from_bytes()
    ctx.maps_occupancy_device(d_check.data_ptr())
    ctx.sync()
    assert torch.equal(d_bytes, d_check), "the stack from bytes differs from the cut one"
    picks = rng.integers(0, n_win, 16)
    assert np.array_equal(d_bytes[torch.from_numpy(picks).cuda()].cpu().numpy(), numpy_cut(occ, origin_xy[picks], side)), "the cut differs from numpy's"
    free = float(d_bytes.float().mean())
    candidates = [("(a) windows: set_maps_windows_device", windows), ("(b) bytes:   set_maps_device", from_bytes)]
    if with_host:
        host()
        ctx.maps_occupancy_device(d_check.data_ptr())
        ctx.sync()
        assert torch.equal(d_bytes, d_check), "the stack from the host's windows differs from the cut one"
        candidates.append(("(c) host:    numpy cut + set_maps", host))
    for _ in range(2):
        for _, f in candidates:
            f()
    t = {name: [] for name, _ in candidates}
    for _ in range(rounds):
        for name, f in candidates:
            t[name].append(f())
    log("%d windows of %d^2 from a %d^2 map (%.1f %% of the windows' cells free); wall-clock ms around the call, median (min .. max) of %d alternating rounds"
        % (n_win, side, n_side, 100 * free, rounds))
    m = {name: float(np.median(v)) for name, v in t.items()}
    a = m[candidates[0][0]]
    for name, _ in candidates:
        log("  %-40s %s   %.2fx of (a)" % (name, med(t[name]), m[name] / a))
    del d_bytes, d_check
    torch.cuda.empty_cache()
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (first, so the extension shares torch's HIP runtime)
    import vhp_amd
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log("windows of the map as a stack of maps (%s)" % vhp_amd.version())
    run(vhp_amd, 2000, 4096, 101, a.rounds, True, log)
    run(vhp_amd, 4000, 256, 1001, a.rounds, False, log)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
