"""Windows of the single map as the stack of maps, cut on the device (vhp_set_maps_windows), and the stack read back as bytes
(vhp_maps_occupancy): the unpack alone, the cut against numpy on the grid of sizes and origins of test_window_cut_cpu.py, more
windows than a grid dimension holds, and the stack's users on a cut stack -- sweeps and ray casts against the oracle on the numpy-cut
windows, the sweep's restriction property against the whole map, the planner against the same call on a stack made from bytes --,
then state and errors.  Every origin here, however far outside the grid, is defined behaviour."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import maps
import window_cases as wc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def vhp():
    import torch  # noqa: F401
    import vhp_amd
    return vhp_amd


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d cells differ, first at %r: %r vs %r" % (what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


# ---- 1. the unpack without the cut ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny", [(1, 1), (63, 65), (64, 64), (130, 3)])
def test_occupancy_round_trip(vhp, nx, ny):
    rng = np.random.default_rng(nx * 100 + ny)
    stack = (rng.random((3, ny, nx)) < 0.6).astype(np.uint8) * rng.integers(1, 256, (3, ny, nx)).astype(np.uint8)   # (free: any value but 0)
    stack[0, 0, 0], stack[2, -1, -1] = 0, 255
    c = vhp.Context(0)
    c.set_maps(stack)
    want = (stack != 0).astype(np.uint8)
    _same(c.maps_occupancy(), want, "%d x %d, all three" % (nx, ny))
    _same(c.maps_occupancy(1, 2), want[1:], "%d x %d, maps 1 and 2" % (nx, ny))
    _same(c.maps_occupancy(2), want[2:], "%d x %d, the last map" % (nx, ny))


# ---- 2. the cut against numpy --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ny", wc.MAP_SIDES)
@pytest.mark.parametrize("nx", wc.MAP_SIDES)
def test_cut_equals_numpy(vhp, nx, ny):
    import torch
    occ = wc.random_map(nx, ny, seed=1000 * nx + ny)
    ox, oy = wc.origins(nx), wc.origins(ny)
    origin_xy = np.array([(x, y) for y in oy for x in ox], np.int32)
    d_origin = torch.from_numpy(origin_xy).cuda()
    c = vhp.Context(0)
    c.set_map(occ)
    some_free = False
    for h in wc.WINDOW_SIDES:
        for w in wc.WINDOW_SIDES:
            want = wc.cut(occ, ox, oy, w, h).reshape(len(origin_xy), h, w)
            some_free |= bool(want.any())
            c.set_maps_windows(origin_xy, w, h)
            assert (c.n_maps, c.maps_nx, c.maps_ny) == (len(origin_xy), w, h)
            _same(c.maps_occupancy(), want, "%d x %d windows of the %d x %d map" % (w, h, nx, ny))
            c.set_maps_windows_device(d_origin.data_ptr(), len(origin_xy), w, h)
            _same(c.maps_occupancy(), want, "%d x %d windows of the %d x %d map, origins on the device" % (w, h, nx, ny))
    assert some_free


def test_occupancy_device_form(vhp):
    """the device form writes the bytes of its maps and nothing else"""
    import torch
    occ = wc.random_map(130, 65, seed=8)
    origin_xy = np.array([(-3, -2), (60, 10), (100, 40)], np.int32)
    c = vhp.Context(0)
    c.set_map(occ)
    c.set_maps_windows(origin_xy, 65, 33)
    want = wc.cut_list(occ, origin_xy, 65, 33)
    cells = 65 * 33
    buf = torch.full((5 + 2 * cells + 7,), 9, dtype=torch.uint8, device="cuda")
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    c.maps_occupancy_device(buf.data_ptr() + 5, first=1, n=2)
    torch.cuda.synchronize()
    c.set_stream(None)
    host = buf.cpu().numpy()
    assert (host[:5] == 9).all() and (host[5 + 2 * cells:] == 9).all()
    _same(host[5: 5 + 2 * cells].reshape(2, 33, 65), want[1:], "maps 1 and 2, device form")


# ---- 3. more windows than a grid dimension holds -------------------------------------------------------------------------------------
def test_many_windows(vhp):
    n = 65537
    occ = wc.random_map(70, 5, seed=3, blocked=0.3)
    rng = np.random.default_rng(4)
    origin_xy = np.stack([rng.integers(-3, 71, n), rng.integers(-2, 6, n)], axis=1).astype(np.int32)
    origin_xy[0], origin_xy[-1] = (1, 1), (66, 2)
    c = vhp.Context(0)
    c.set_map(occ)
    c.set_maps_windows(origin_xy, 3, 2)
    got = c.maps_occupancy()
    assert got.shape == (n, 2, 3)
    picks = [0, n - 1, 65535, 65536] + rng.integers(0, n, 50).tolist()
    want = wc.cut_list(occ, origin_xy[picks], 3, 2)
    _same(got[picks], want, "the picked windows")
    assert want[0].any() and want[1].any() and not want.all()
    _same(c.maps_occupancy(n - 1, 1), want[1:2], "the last window, asked for alone")


# ---- 4. the stack's users on both packed copies, against the oracle on the numpy-cut windows -----------------------------------------
@pytest.fixture(scope="module")
def parity_map():
    return maps.random_rect_map(100, 90, 14, 3, 20, 3, 20, 21)


@pytest.mark.parametrize("w,h,origins", [(1, 1, [(0, 0), (50, 40), (99, 89), (7, 80)]),
                                         (17, 64, [(-5, -20), (40, 10), (90, 50), (30, 26)]),
                                         (65, 33, [(-30, 70), (20, 20), (60, -10), (35, 57)])])
def test_oracle_parity_on_windows(vhp, oracle, parity_map, w, h, origins):
    occ = parity_map
    wins = wc.cut_list(occ, origins, w, h)
    # up to three free sources per window, in window coordinates
    src, idx = [], []
    for k, win in enumerate(wins):
        pts = maps.free_sources(win, min(3, int(win.sum())), 60 + k) if win.any() else []
        src += [(int(x), int(y)) for x, y in pts]
        idx += [k] * len(pts)
    assert len(set(idx)) >= 3, "pick windows with free cells"
    c = vhp.Context(0)
    c.set_map(occ)
    c.set_maps_windows(np.array(origins, np.int32), w, h)
    got64 = c.sweep_maps_batch(src, idx)
    got32 = c.sweep_maps_batch(src, idx, dtype=vhp.F32)
    rays = c.raycast_maps_batch(src, idx, dtype=vhp.U8)
    for i, ((sx, sy), k) in enumerate(zip(src, idx)):
        what = "source (%d, %d) of the %d x %d window at %r" % (sx, sy, w, h, origins[k])
        want = oracle.sweep_full(wins[k], sx, sy)
        _same(got64[i], want, "sweep, fp64: " + what)
        _same(got32[i], want.astype(np.float32), "sweep, fp32: " + what)
        _same(rays[i], oracle.raycast_all(wins[k], sx, sy).astype(np.uint8), "ray cast: " + what)


# ---- 5. the restriction property ---------------------------------------------------------------------------------------------------
def test_sweep_windows_equals_the_whole_map_within_range(vhp):
    r = 20
    occ = maps.random_rect_map(150, 131, 30, 3, 18, 3, 18, 17)
    occ[0, 0] = occ[130, 149] = occ[5, 148] = occ[129, 3] = 1
    sources = [(0, 0), (149, 130), (148, 5), (3, 129)] + [tuple(int(v) for v in p) for p in maps.free_sources(occ, 8, 23)]
    c = vhp.Context(0)
    c.set_map(occ)
    whole = c.sweep_batch(sources)
    local = c.sweep_windows(sources, r)
    assert local.shape == (len(sources), 2 * r + 1, 2 * r + 1) and (c.n_maps, c.maps_nx, c.maps_ny) == (len(sources), 2 * r + 1, 2 * r + 1)
    compared = lit = 0
    for i, (sx, sy) in enumerate(sources):
        # window cell (a, b) is the map's cell (sx - r + a, sy - r + b): local and absolute x, y >= 1, inside the grid
        a0, b0 = max(1, 1 - (sx - r)), max(1, 1 - (sy - r))
        a1, b1 = min(2 * r + 1, 150 - (sx - r)), min(2 * r + 1, 131 - (sy - r))
        got = local[i, b0:b1, a0:a1]
        want = whole[i, sy - r + b0: sy - r + b1, sx - r + a0: sx - r + a1]
        _same(np.ascontiguousarray(got), np.ascontiguousarray(want), "source (%d, %d)" % (sx, sy))
        compared += got.size
        lit += int((got > 0).sum())
    assert compared > len(sources) * r * r and lit > compared // 4


# ---- 6. the planner on windows -------------------------------------------------------------------------------------------------------
def _smallest_latency_side():
    """the smallest square side of two cells or more (a query needs a start and an end) at which tests/golden/kernel_choice.json gives
    one fp64 source on 256 CUs the latency sweep"""
    with open(os.path.join(HERE, "golden", "kernel_choice.json")) as f:
        plans = json.load(f)["plans"]
    sides = []
    for key, runs in plans.items():
        m = re.match(r"A (\d+)x(\d+) cus256 f64 ", key)
        if m and m.group(1) == m.group(2) and int(m.group(1)) >= 2 and runs.split()[0].startswith("4"):
            sides.append(int(m.group(1)))
    return min(sides)


@pytest.mark.parametrize("side", [64, _smallest_latency_side()])
def test_planner_on_windows(vhp, side):
    """4 windows, a query in each: the maps batch on the cut stack against the same call on set_maps of the numpy-cut windows.  Both
    sides take the latency sweep (the table gives it to every small square grid), so both read diagonal maps built from their stack."""
    occ = maps.random_rect_map(200, 180, 40, 3, 16, 3, 16, 31)
    origins = [(-side // 4, 20), (60, 50), (200 - side // 2, 180 - side // 2), (120, 10)]
    wins = wc.cut_list(occ, origins, side, side)
    queries = []
    rng = np.random.default_rng(80 + side)
    for win in wins:   # (a start and another cell as the end, both free in their window)
        free = np.argwhere(win != 0)
        (sy, sx), (ey, ex) = free[rng.choice(len(free), 2, replace=False)]
        queries.append((int(sx), int(sy), int(ex), int(ey)))
    idx = [0, 1, 2, 3]
    results = []
    for cut_on_device in (True, False):
        c = vhp.Context(0)
        if cut_on_device:
            c.set_map(occ)
            c.set_maps_windows(np.array(origins, np.int32), side, side)
        else:
            c.set_maps(wins)
        paths = c.planner_solve_maps_batch(queries, idx, 0.25, 60, outputs="paths")
        assert c.last_sweep_kernel() == 4
        full = c.planner_solve_maps_batch(queries, idx, 0.25, 60)
        results.append((paths, full))
    (p_cut, f_cut), (p_ref, f_ref) = results
    assert any(r["status"] == vhp.VHP_OK and r["n_pivots"] >= 1 for r in f_ref)
    for q in range(4):
        what = "query %d %r in the %d x %d window at %r" % (q, queries[q], side, side, origins[q])
        for name in ("status", "n_pivots", "path_status", "length"):
            assert p_cut[q][name] == p_ref[q][name], (what, name, p_cut[q][name], p_ref[q][name])
        _same(p_cut[q]["path"], p_ref[q]["path"], what + ": path")
        assert f_cut[q]["status"] == f_ref[q]["status"] and f_cut[q]["n_pivots"] == f_ref[q]["n_pivots"], what
        _same(f_cut[q]["pivots"], f_ref[q]["pivots"], what + ": pivots")
        if f_ref[q]["came_from"] is None:
            assert f_cut[q]["came_from"] is None, what
        else:
            _same(f_cut[q]["came_from"], f_ref[q]["came_from"], what + ": labels")


# ---- 7. state and errors -------------------------------------------------------------------------------------------------------------
def test_state_and_errors(vhp):
    lib = vhp.load_library()
    occ = maps.random_rect_map(120, 97, 14, 3, 20, 3, 20, 5)
    origin_xy = np.array([(0, 0), (30, 20), (70, 40), (-10, 60)], np.int32)
    out = np.zeros(4 * 64 * 64, np.uint8)
    c = vhp.Context(0)
    # nothing set
    assert lib.vhp_set_maps_windows(c.h, origin_xy.ctypes.data, 4, 64, 64) == vhp.VHP_ERR_NO_MAP
    assert lib.vhp_set_maps_windows_device(c.h, origin_xy.ctypes.data, 4, 64, 64) == vhp.VHP_ERR_NO_MAP
    assert lib.vhp_maps_occupancy(c.h, 0, 1, out.ctypes.data) == vhp.VHP_ERR_NO_MAP
    assert lib.vhp_maps_occupancy_device(c.h, 0, 1, out.ctypes.data) == vhp.VHP_ERR_NO_MAP
    c.set_map(occ)
    assert lib.vhp_maps_occupancy(c.h, 0, 1, out.ctypes.data) == vhp.VHP_ERR_NO_MAP   # (a single map is no stack)
    # arguments
    for w, h in ((0, 64), (64, 0), (-1, 64)):
        assert lib.vhp_set_maps_windows(c.h, origin_xy.ctypes.data, 4, w, h) == vhp.VHP_ERR_ARG
    assert lib.vhp_set_maps_windows(c.h, origin_xy.ctypes.data, 0, 64, 64) == vhp.VHP_ERR_ARG
    assert lib.vhp_set_maps_windows(c.h, None, 4, 64, 64) == vhp.VHP_ERR_ARG
    assert lib.vhp_set_maps_windows_device(c.h, None, 4, 64, 64) == vhp.VHP_ERR_ARG
    for w, h in ((8192 + 1, 64), (64, 8192 + 1)):   # (VHP_MAX_SIDE + 1)
        assert lib.vhp_set_maps_windows(c.h, origin_xy.ctypes.data, 4, w, h) == vhp.VHP_ERR_TOO_LARGE
    assert lib.vhp_maps_occupancy(c.h, 0, 1, out.ctypes.data) == vhp.VHP_ERR_NO_MAP   # (a refused call sets no stack)
    with pytest.raises(vhp.VhpError) as e:
        c.set_maps_windows(origin_xy, 0, 5)
    assert e.value.code == vhp.VHP_ERR_ARG and c.n_maps == 0
    # a stack of windows, a maps batch on it
    c.set_maps_windows(origin_xy, 64, 64)
    want = wc.cut_list(occ, origin_xy, 64, 64)
    _same(c.maps_occupancy(), want, "the first stack")
    for first, n in ((-1, 1), (4, 1), (0, 5), (3, 2), (0, 0), (0, -1)):
        assert lib.vhp_maps_occupancy(c.h, first, n, out.ctypes.data) == vhp.VHP_ERR_ARG, (first, n)
        assert lib.vhp_maps_occupancy_device(c.h, first, n, out.ctypes.data) == vhp.VHP_ERR_ARG, (first, n)
    assert lib.vhp_maps_occupancy(c.h, 0, 1, None) == vhp.VHP_ERR_ARG
    pts = maps.free_sources(want[1], 2, 12)
    c.planner_solve_maps_batch([tuple(int(v) for v in pts[0]) + tuple(int(v) for v in pts[1])], [1], 0.25, 40)
    assert lib.vhp_planner_maps_batch_results(c.h, 0, None, None, None, None) == vhp.VHP_OK
    # the stack is a copy: another single map leaves it as it is
    c.set_map(maps.random_rect_map(50, 40, 6, 3, 9, 3, 9, 2))
    _same(c.maps_occupancy(), want, "the first stack after set_map of another map")
    # fewer and smaller windows: a new stack, of the new single map, and the maps batch's results are gone
    occ2 = maps.random_rect_map(50, 40, 6, 3, 9, 3, 9, 2)
    c.set_maps_windows(origin_xy[:2], 33, 17)
    assert (c.n_maps, c.maps_nx, c.maps_ny) == (2, 33, 17)
    _same(c.maps_occupancy(), wc.cut_list(occ2, origin_xy[:2], 33, 17), "the second stack")
    assert lib.vhp_maps_occupancy(c.h, 2, 1, out.ctypes.data) == vhp.VHP_ERR_ARG
    assert lib.vhp_planner_maps_batch_results(c.h, 0, None, None, None, None) == vhp.VHP_ERR_ARG
    assert c.planner_maps_batch_group() == 0


def test_plain_solve_survives_set_maps_windows(vhp):
    occ = maps.random_rect_map(120, 97, 14, 3, 20, 3, 20, 5)
    c = vhp.Context(0)
    c.set_map(occ)
    start, end = (tuple(int(v) for v in p) for p in maps.free_sources(occ, 2, 9))
    want = c.planner_solve(start, end, 0.25, 60)
    assert want["status"] == vhp.VHP_OK
    path = c.planner_path()
    assert path["status"] == vhp.VHP_OK and len(path["path"]) >= 2
    c.sweep_batch([start])
    ms = c.last_elapsed_ms()
    c.set_maps_windows(np.array([(3, 4), (50, 60)], np.int32), 40, 30)
    assert c.last_elapsed_ms() == ms   # (not timed)
    # the plain solve's device results and its path are still there, and so is the single map
    p = [C.c_void_p() for _ in range(4)]
    assert c.lib.vhp_planner_results_device(c.h, *[C.byref(q) for q in p]) == vhp.VHP_OK
    after = c.planner_path()
    assert after["status"] == vhp.VHP_OK and after["length"] == path["length"] and after["path"].tolist() == path["path"].tolist()
    again = c.planner_solve(start, end, 0.25, 60)
    for name in ("came_from", "vis_global", "vis_local", "pivots"):
        assert again[name].tobytes() == want[name].tobytes(), name
