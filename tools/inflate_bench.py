"""Obstacles grown by a robot's footprint: the inflation on the device (vhp_inflate_map, vhp_inflate_maps) against what a caller had
before it.

Single map: the 1000^2 and 4096^2 random-rectangle maps of the benchmark configurations 3 and 5; footprints disc of radius 3, 8 and 64
and square 8.  Per combination
  (a) inflate   vhp_set_map_device of the map's bytes (resident), then vhp_inflate_map: only the second call is timed
  (b) floor     vhp_set_map_device of the already inflated bytes (resident): the repacking every route ends in
  (c) host      a numpy inflation of the host map, then vhp_set_map: the caller's route until now.  The numpy code is not the
                brute force over every offset (12 853 of them for the disc of radius 64): per distinct half-width of the footprint one
                windowed count along x from a single cumulative sum, then an OR of the rows shifted by the line offsets with that
                half-width
Stack: vhp_inflate_maps with the disc of radius 3 on 256 windows of 101^2 and on 16 copies of a 1000^2 map (vhp_set_maps_windows_device
before each timed call, untimed, so that every round inflates the same maps), and with the disc of radius 8 on the copies.
None of these is timed by vhp_last_elapsed_ms: the host clock is put around each synchronous call.  After a warm-up of each, the
candidates alternate `--rounds` times in one process; reported are the median and the spread (min .. max).  Before any timing the
routes' maps are read back (vhp_map_occupancy) and compared byte for byte.

usage: inflate_bench.py [--rounds N] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def med(v):
    return "%9.3f (%.3f .. %.3f)" % (float(np.median(v)), min(v), max(v))


def half_widths(shape, p):
    """hw[d], d = 0 .. reach, of a footprint given as the C ABI gives it: the largest |dx| at line offset d"""
    from math import isqrt
    if shape == "disc":
        return [isqrt(p - d * d) for d in range(isqrt(p) + 1)]
    return [p if shape == "square" else p - d for d in range(p + 1)]


def numpy_inflate(occ, shape, p):
    """uint8 [ny, nx], 1 = free -> the inflated map, cells outside the grid free"""
    ny, nx = occ.shape
    hw = half_widths(shape, p)
    reach = len(hw) - 1
    count = np.zeros((ny, nx + 2 * reach + 1), np.int32)
    np.cumsum(occ == 0, axis=1, dtype=np.int32, out=count[:, reach + 1: reach + 1 + nx])
    count[:, reach + 1 + nx:] = count[:, reach + nx: reach + nx + 1]
    blocked = np.zeros((ny + 2 * reach, nx), bool)
    grown = blocked[reach: reach + ny]
    for h in sorted(set(hw)):
        # blocked cells in x - h .. x + h, for every x at once
        wide = count[:, reach + 1 + h: reach + 1 + h + nx] != count[:, reach - h: reach - h + nx]
        for d in (d for d, v in enumerate(hw) if v == h):
            for dy in {d, -d}:
                blocked[reach - dy: reach - dy + ny] |= wide
    return (~grown).astype(np.uint8)


def run_map(vhp, name, occ, footprints, rounds, log):
    import torch
    ny, nx = occ.shape
    ctx = vhp.Context(0)
    d_occ = torch.from_numpy(occ).cuda()
    log("%s, %d x %d, %.1f %% free; wall-clock ms around the call, median (min .. max) of %d alternating rounds" % (name, nx, ny, 100.0 * occ.mean(), rounds))
    out = {}
    for shape, radius in footprints:
        _, p = vhp.footprint(radius, shape)
        want = numpy_inflate(occ, shape, p)
        d_want = torch.from_numpy(want).cuda()

        def inflate():
            ctx.set_map_device(d_occ.data_ptr(), nx, ny)
            t0 = time.perf_counter()
            ctx.inflate_map(p=p, shape=shape)
            return (time.perf_counter() - t0) * 1e3

        def floor():
            t0 = time.perf_counter()
            ctx.set_map_device(d_want.data_ptr(), nx, ny)
            return (time.perf_counter() - t0) * 1e3

        def host():
            t0 = time.perf_counter()
            ctx.set_map(numpy_inflate(occ, shape, p))
            return (time.perf_counter() - t0) * 1e3

        candidates = [("(a) inflate: vhp_inflate_map", inflate), ("(b) floor:   vhp_set_map_device, inflated bytes", floor),
                      ("(c) host:    numpy inflation + vhp_set_map", host)]
        for cname, f in candidates:   # the results first (this is also the warm-up): the three routes leave the same map
            f()
            assert np.array_equal(ctx.map_occupancy(), want), "%s: the map differs from numpy's" % cname
        t = {cname: [] for cname, _ in candidates}
        for _ in range(rounds):
            for cname, f in candidates:
                t[cname].append(f())
        m = {cname: float(np.median(v)) for cname, v in t.items()}
        a = m[candidates[0][0]]
        log(" %s of radius %d (p = %d), %.1f %% free afterwards" % (shape, radius, p, 100.0 * want.mean()))
        for cname, _ in candidates:
            log("  %-50s %s   %.2fx of (a)" % (cname, med(t[cname]), m[cname] / a))
        out[(shape, radius)] = m
    return out


def run_stack(vhp, what, occ, origins, w, h, footprints, rounds, log):
    import torch
    ctx = vhp.Context(0)
    ctx.set_map(occ)
    n = len(origins)
    d_origin = torch.from_numpy(np.ascontiguousarray(origins, np.int32)).cuda()
    log("%s; vhp_inflate_maps on all of them, wall-clock ms around the call, median (min .. max) of %d rounds" % (what, rounds))
    for shape, radius in footprints:
        _, p = vhp.footprint(radius, shape)

        def inflate():
            ctx.set_maps_windows_device(d_origin.data_ptr(), n, w, h)
            t0 = time.perf_counter()
            ctx.inflate_maps(p=p, shape=shape)
            return (time.perf_counter() - t0) * 1e3

        inflate()   # the result first (this is also the warm-up): a map of the middle of the stack against numpy on the map as cut
        k = n // 2
        got = ctx.maps_occupancy(k, 1)[0]
        ctx.set_maps_windows_device(d_origin.data_ptr(), n, w, h)
        assert np.array_equal(got, numpy_inflate(ctx.maps_occupancy(k, 1)[0], shape, p)), "map %d differs from numpy's" % k
        t = [inflate() for _ in range(rounds)]
        log("  %-50s %s" % ("%s of radius %d (p = %d)" % (shape, radius, p), med(t)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (first, so the extension shares torch's HIP runtime)
    import vhp_amd
    from importlib import import_module
    synth = import_module("visibility-heuristic-path-planner_amd.synth")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log("obstacles grown by a footprint, on the device and on the host (%s)" % vhp_amd.version())
    single = (("disc", 3), ("disc", 8), ("disc", 64), ("square", 8))
    occ3, _ = synth.config_c3(1)
    occ5, _ = synth.config_c5(1)
    run_map(vhp_amd, "random-rectangle map (benchmark configuration 3)", occ3, single, a.rounds, log)
    run_map(vhp_amd, "random-rectangle map (benchmark configuration 5)", occ5, single, a.rounds, log)
    rng = np.random.default_rng(7)
    occ2k = (rng.random((2000, 2000)) >= 0.05).astype(np.uint8)
    run_stack(vhp_amd, "256 windows of 101^2 from a 2000^2 map with 5 % blocked cells", occ2k, rng.integers(-50, 1950, (256, 2)).astype(np.int32), 101, 101,
              (("disc", 3),), a.rounds, log)
    run_stack(vhp_amd, "16 copies of the 1000^2 random-rectangle map", occ3, np.zeros((16, 2), np.int32), 1000, 1000, (("disc", 3), ("disc", 8)), a.rounds, log)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
