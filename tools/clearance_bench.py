"""The clearance field on the device (vhp_map_clearance_device, vhp_maps_clearance_device) against the nearest existing call and a host
route.

Single map: the 1000^2 and 4096^2 random-rectangle maps of the benchmark configurations 3 and 5; p_max disc 9, 64 and 4096 and square
8, border off.  Per combination
  (a) field     vhp_map_clearance_device into a resident buffer, then a synchronise of the context's stream
  (b) inflate   vhp_set_map_device of the map's bytes (resident, not timed), then vhp_inflate_map of the same footprint: the mask for
                that one p only, where the field gives the mask for every p <= p_max
  (c) host      scipy.ndimage's distance transforms of the host map (the exact Euclidean one, squared and rounded, for the disc; the
                chessboard one for the square), capped at p_max -- or, without scipy, numpy: the distance along each row from two
                running extrema, then the minimum over the row offsets
Stack: vhp_maps_clearance_device with the disc p_max 9 on 256 windows of 101^2 and on 16 copies of the 1000^2 map, and p_max 64 on
the copies.
The host clock is put around each call and the synchronise that ends it.  After a warm-up of each, the candidates alternate `--rounds`
times in one process; reported are the median and the spread (min .. max).  Before any timing the field is compared, byte for byte,
with the host route's, and (field > p_max) with the map (b) leaves.

The floor of (a) is the field itself: 2 bytes written per cell (the packed map is 1 bit per cell from memory, 1/16 of that; its
re-reads for the neighbour words and the halo rows are served by the caches), at the 6.3 TB/s a streaming kernel reaches on this
device.

usage: clearance_bench.py [--rounds N] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

FAR = 0xFFFF
STREAM_TBS = 6.3   # achievable HBM bandwidth of the device, TB/s


def med(v):
    return "%9.3f (%.3f .. %.3f)" % (float(np.median(v)), min(v), max(v))


def reach_of(shape, p):
    from math import isqrt
    return isqrt(p) if shape == "disc" else p


def numpy_field(occ, shape, p_max):
    """uint8 [ny, nx], 1 = free -> the uint16 field, cells outside the grid free (shapes disc and square)"""
    ny, nx = occ.shape
    reach = reach_of(shape, p_max)
    x = np.arange(nx, dtype=np.int32)
    at = np.where(occ == 0, x, -10 ** 6)
    left = x - np.maximum.accumulate(at, axis=1)
    at = np.where(occ == 0, x, 10 ** 6)
    right = np.minimum.accumulate(at[:, ::-1], axis=1)[:, ::-1] - x
    g = np.minimum(np.minimum(left, right), 255).astype(np.int32)
    pad = np.full((ny + 2 * reach, nx), 255, np.int32)
    pad[reach:reach + ny] = g
    best = np.full((ny, nx), 10 ** 6, np.int32)
    for k in range(-reach, reach + 1):
        rows = pad[reach + k:reach + k + ny]
        np.minimum(best, rows * rows + k * k if shape == "disc" else np.maximum(rows, abs(k)), out=best)
    return np.where(best <= p_max, best, FAR).astype(np.uint16)


def host_field(occ, shape, p_max):
    try:
        from scipy import ndimage
    except ImportError:
        return numpy_field(occ, shape, p_max)
    if not (occ == 0).any():
        return np.full(occ.shape, FAR, np.uint16)
    if shape == "disc":
        d = ndimage.distance_transform_edt(occ != 0)
        c = np.rint(d * d).astype(np.int64)
    else:
        c = ndimage.distance_transform_cdt(occ != 0, metric="chessboard").astype(np.int64)
    return np.where(c <= p_max, c, FAR).astype(np.uint16)


def host_route_name():
    try:
        import scipy
        return "scipy.ndimage %s" % scipy.__version__
    except ImportError:
        return "numpy"


def run_map(vhp, name, occ, p_maxes, rounds, log):
    import torch
    ny, nx = occ.shape
    ctx, other = vhp.Context(0), vhp.Context(0)
    d_occ = torch.from_numpy(occ).cuda()
    d_field = torch.empty((ny, nx), dtype=torch.int16, device="cuda")
    ctx.set_map_device(d_occ.data_ptr(), nx, ny)
    floor_ms = 2.0 * nx * ny / (STREAM_TBS * 1e12) * 1e3
    log("%s, %d x %d, %.1f %% free; wall-clock ms around the call and its synchronise, median (min .. max) of %d alternating rounds; "
        "the floor of (a), 2 bytes a cell at %.1f TB/s, is %.4f ms" % (name, nx, ny, 100.0 * occ.mean(), rounds, STREAM_TBS, floor_ms))
    for shape, p_max in p_maxes:
        def field():
            t0 = time.perf_counter()
            ctx.map_clearance_device(d_field.data_ptr(), p=p_max, shape=shape)
            ctx.sync()
            return (time.perf_counter() - t0) * 1e3

        def inflate():
            other.set_map_device(d_occ.data_ptr(), nx, ny)
            t0 = time.perf_counter()
            other.inflate_map(p=p_max, shape=shape)
            return (time.perf_counter() - t0) * 1e3

        def host():
            t0 = time.perf_counter()
            host_field(occ, shape, p_max)
            return (time.perf_counter() - t0) * 1e3

        # the results first (this is also the warm-up)
        field()
        got = d_field.cpu().numpy().view(np.uint16)
        assert np.array_equal(got, host_field(occ, shape, p_max)), "the field differs from the host route's"
        inflate()
        assert np.array_equal((got > p_max).astype(np.uint8), other.map_occupancy()), "(field > p_max) differs from the inflated map"
        candidates = [("(a) field:   vhp_map_clearance_device", field, rounds), ("(b) inflate: vhp_inflate_map, the one mask of p_max", inflate, rounds),
                      ("(c) host:    %s" % host_route_name(), host, min(rounds, 3))]
        t = {cname: [] for cname, _, _ in candidates}
        for r in range(rounds):
            for cname, f, n in candidates:
                if r < n:
                    t[cname].append(f())
        m = {cname: float(np.median(v)) for cname, v in t.items()}
        a = m[candidates[0][0]]
        log(" %s p_max %d (reach %d), %.1f %% of the cells within p_max" % (shape, p_max, reach_of(shape, p_max), 100.0 * (got != FAR).mean()))
        for cname, _, n in candidates:
            log("  %-52s %s   %.2fx of (a)%s" % (cname, med(t[cname]), m[cname] / a, "" if n == rounds else "   (%d rounds)" % n))
        log("  (a) is %.1fx its floor (%.1f %% of it); one field costs what %.2f calls of (b) cost and holds the mask of every p <= p_max"
            % (a / floor_ms, 100.0 * floor_ms / a, a / m[candidates[1][0]]))


def run_stack(vhp, what, occ, origins, w, h, p_maxes, rounds, log):
    import torch
    ctx = vhp.Context(0)
    ctx.set_map(occ)
    n = len(origins)
    ctx.set_maps_windows(origins, w, h)
    d_field = torch.empty((n, h, w), dtype=torch.int16, device="cuda")
    floor_ms = 2.0 * n * w * h / (STREAM_TBS * 1e12) * 1e3
    log("%s; vhp_maps_clearance_device on all of them, one launch, wall-clock ms around the call and its synchronise, median (min .. max) of %d rounds; "
        "floor %.4f ms" % (what, rounds, floor_ms))
    for shape, p_max in p_maxes:
        def field():
            t0 = time.perf_counter()
            ctx.maps_clearance_device(d_field.data_ptr(), p=p_max, shape=shape)
            ctx.sync()
            return (time.perf_counter() - t0) * 1e3

        field()   # the result first (this is also the warm-up): a map of the middle of the stack against the host route on the map as cut
        k = n // 2
        assert np.array_equal(d_field[k].cpu().numpy().view(np.uint16), host_field(ctx.maps_occupancy(k, 1)[0], shape, p_max)), "map %d differs" % k
        t = [field() for _ in range(rounds)]
        log("  %-52s %s   %.1fx the floor" % ("%s p_max %d" % (shape, p_max), med(t), float(np.median(t)) / floor_ms))


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

    log("the clearance field on the device, the inflation of one footprint, and a host route (%s)" % vhp_amd.version())
    single = (("disc", 9), ("disc", 64), ("disc", 4096), ("square", 8))
    occ3, _ = synth.config_c3(1)
    occ5, _ = synth.config_c5(1)
    run_map(vhp_amd, "random-rectangle map (benchmark configuration 3)", occ3, single, a.rounds, log)
    run_map(vhp_amd, "random-rectangle map (benchmark configuration 5)", occ5, single, a.rounds, log)
    rng = np.random.default_rng(7)
    occ2k = (rng.random((2000, 2000)) >= 0.05).astype(np.uint8)
    run_stack(vhp_amd, "256 windows of 101^2 from a 2000^2 map with 5 % blocked cells", occ2k, rng.integers(-50, 1950, (256, 2)).astype(np.int32), 101, 101,
              (("disc", 9),), a.rounds, log)
    run_stack(vhp_amd, "16 copies of the 1000^2 random-rectangle map", occ3, np.zeros((16, 2), np.int32), 1000, 1000, (("disc", 9), ("disc", 64)), a.rounds, log)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
