"""Obstacles grown by a robot's footprint on the device (vhp_inflate_map, vhp_inflate_maps) and the single map read back as bytes
(vhp_map_occupancy): the inflation against numpy (inflate_cases.inflate, written from the definition) on both packed copies, the
read-back alone, ranges of a stack and more maps than a grid dimension holds, the order of inflating and cutting windows, every
consumer of the single map after an inflation against the same call after set_map of numpy's inflation, the fleet recipe of
include/vhp.h on the maps batch, then state and errors.  Every comparison is of bytes."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import inflate_cases as ic
import maps
import window_cases as wc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE_NAMES = {ic.DISC: "disc", ic.SQUARE: "square", ic.DIAMOND: "diamond"}


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


def _some_free(occ, n, seed):
    """up to n free cells of occ as (x, y)"""
    free = np.argwhere(occ != 0)
    if not len(free):
        return []
    pick = np.random.default_rng(seed).choice(len(free), min(n, len(free)), replace=False)
    return [(int(free[i][1]), int(free[i][0])) for i in pick]


# ---- 1. the inflation against numpy, on the single map ---------------------------------------------------------------------------
@pytest.mark.parametrize("ny", ic.GPU_SIDES[1])
@pytest.mark.parametrize("nx", ic.GPU_SIDES[0])
def test_inflate_map_equals_numpy(vhp, nx, ny):
    occ = wc.random_map(nx, ny, seed=1000 * nx + ny, blocked=0.03)
    occ[ny // 2, nx // 2] = 0   # (at least one obstacle, whatever the side)
    c, ref = vhp.Context(0), vhp.Context(0)
    changed = rays_differ = False
    for shape, p in ic.GPU_FOOTPRINTS:
        for border in (False, True):
            what = "%d x %d, %s p %d, border %r" % (nx, ny, SHAPE_NAMES[shape], p, border)
            want = ic.inflate(occ, shape, p, border)
            c.set_map(occ)
            c.inflate_map(p=p, shape=SHAPE_NAMES[shape], border=border)
            assert (c.nx, c.ny) == (nx, ny)
            _same(c.map_occupancy(), want, what + ": the row-packed copy")   # (vhp_map_occupancy unpacks the rows)
            changed |= not np.array_equal(want, occ)
            # the column-packed copy: ray casts read rows for y-major rays and columns for x-major ones
            src = _some_free(want, 3, seed=p + 7)
            if src:
                ref.set_map(want)
                rays = c.raycast_batch(src, dtype=vhp.U8)
                _same(rays, ref.raycast_batch(src, dtype=vhp.U8), what + ": ray casts from %r" % (src,))
                if not np.array_equal(want, occ):
                    ref.set_map(occ)
                    rays_differ |= rays.tobytes() != ref.raycast_batch(src, dtype=vhp.U8).tobytes()
    assert changed == (nx * ny > 1), "a map on which no footprint changes anything shows nothing"
    if nx >= 63 and ny >= 64:
        assert rays_differ, "ray casts that never see the inflation show nothing"


# ---- 2. the read-back alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny", [(1, 1), (63, 65), (130, 3)])
def test_map_occupancy_normalises(vhp, nx, ny):
    rng = np.random.default_rng(nx * 100 + ny)
    occ = (rng.random((ny, nx)) < 0.6).astype(np.uint8) * rng.integers(1, 256, (ny, nx)).astype(np.uint8)   # (free: any value but 0)
    occ[-1, -1] = 255
    c = vhp.Context(0)
    c.set_map(occ)
    _same(c.map_occupancy(), (occ != 0).astype(np.uint8), "%d x %d" % (nx, ny))
    occ[-1, -1] = 0
    c.set_map(occ)
    _same(c.map_occupancy(), (occ != 0).astype(np.uint8), "%d x %d, the last cell blocked" % (nx, ny))


def test_map_occupancy_device_form(vhp):
    """the device form writes the nx * ny bytes of the map and nothing around them"""
    import torch
    occ = wc.random_map(130, 65, seed=8, blocked=0.3)
    c = vhp.Context(0)
    c.set_map(occ)
    cells = 130 * 65
    buf = torch.full((5 + cells + 7,), 9, dtype=torch.uint8, device="cuda")
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    c.map_occupancy_device(buf.data_ptr() + 5)
    torch.cuda.synchronize()
    c.set_stream(None)
    host = buf.cpu().numpy()
    assert (host[:5] == 9).all() and (host[5 + cells:] == 9).all()
    _same(host[5: 5 + cells].reshape(65, 130), occ, "device form")


# ---- 3. ranges of a stack ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", [False, True])
def test_inflate_maps_range(vhp, border):
    stack = np.stack([wc.random_map(65, 33, seed=40 + k, blocked=0.03) for k in range(5)])
    c = vhp.Context(0)
    c.set_maps(stack)
    c.inflate_maps(1, 3, radius=2, border=border)
    want = stack.copy()
    want[1:4] = ic.inflate_stack(stack[1:4], ic.DISC, 4, border)
    assert not np.array_equal(want[1:4], stack[1:4])
    got = c.maps_occupancy()
    _same(got[[0, 4]], stack[[0, 4]], "maps 0 and 4, outside the range")
    _same(got, want, "the stack after inflate_maps(1, 3)")
    # an overlapping range composes: numpy applied twice
    c.inflate_maps(3, radius=1, shape="square", border=border)
    want[3:5] = ic.inflate_stack(want[3:5], ic.SQUARE, 1, border)
    _same(c.maps_occupancy(), want, "the stack after inflate_maps(3, 2) on top")
    # the column-packed copies went along: ray casts on maps 0, 2, 3 and 4
    ref = vhp.Context(0)
    ref.set_maps(want)
    src, idx = [], []
    for k in (0, 2, 3, 4):
        pts = _some_free(want[k], 2, seed=k)
        src += pts
        idx += [k] * len(pts)
    assert len(set(idx)) >= 3
    _same(c.raycast_maps_batch(src, idx, dtype=vhp.U8), ref.raycast_maps_batch(src, idx, dtype=vhp.U8), "ray casts on the inflated stack")


def test_inflate_many_maps(vhp):
    n = 65537
    rng = np.random.default_rng(4)
    stack = (rng.random((n, 2, 3)) >= 0.2).astype(np.uint8)
    stack[0], stack[-1] = [[1, 1, 1], [1, 1, 0]], [[0, 1, 1], [1, 1, 1]]
    c = vhp.Context(0)
    c.set_maps(stack)
    c.inflate_maps(p=1)
    got = c.maps_occupancy()
    assert got.shape == (n, 2, 3)
    picks = [0, 65535, 65536, n - 1] + rng.integers(0, n, 50).tolist()
    want = ic.inflate_stack(stack[picks], ic.DISC, 1)
    _same(got[picks], want, "the picked maps")
    assert want[0].tolist() == [[1, 1, 0], [1, 0, 0]] and want[3].tolist() == [[0, 0, 1], [0, 1, 1]]


# ---- 4. the order of inflating and cutting ----------------------------------------------------------------------------------------------
def test_inflate_then_cut(vhp):
    occ = wc.random_map(130, 65, seed=11, blocked=0.03)
    origins = np.array([(-3, -2), (100, 40), (60, -5), (-10, 50), (120, 60), (30, 20)], np.int32)   # over every edge and corner, and inside
    c = vhp.Context(0)
    c.set_map(occ)
    c.inflate_map(radius=2)
    c.set_maps_windows(origins, 40, 30)
    grown = ic.inflate(occ, ic.DISC, 4)
    _same(c.maps_occupancy(), wc.cut_list(grown, origins, 40, 30), "windows of the inflated map")
    _same(c.map_occupancy(), grown, "the inflated map itself")


def test_cut_then_inflate_is_another_thing(vhp):
    """the rule of include/vhp.h: an obstacle one cell outside a window grows into the window of the inflated map, and an inflated
    window knows nothing of it"""
    occ = np.ones((40, 40), np.uint8)
    occ[20, 10] = 0
    origin = np.array([(11, 10)], np.int32)   # the window's column 0 is the map's column 11
    a, b = vhp.Context(0), vhp.Context(0)
    a.set_map(occ)
    a.inflate_map(radius=1)
    a.set_maps_windows(origin, 20, 20)
    b.set_map(occ)
    b.set_maps_windows(origin, 20, 20)
    b.inflate_maps(radius=1)
    first, second = a.maps_occupancy()[0], b.maps_occupancy()[0]
    _same(first, wc.cut_list(ic.inflate(occ, ic.DISC, 1), origin, 20, 20)[0], "inflate, then cut")
    _same(second, ic.inflate(wc.cut_list(occ, origin, 20, 20)[0], ic.DISC, 1), "cut, then inflate")
    assert first[10, 0] == 0 and second[10, 0] == 1 and second.all()


# ---- 5. every consumer of the single map after an inflation ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def consumer_map():
    occ = maps.random_rect_map(150, 131, 30, 3, 18, 3, 18, 17)
    return occ, ic.inflate(occ, ic.DISC, 4)


def _two_contexts(vhp, occ, grown):
    a, b = vhp.Context(0), vhp.Context(0)
    a.set_map(occ)
    a.inflate_map(radius=2)
    b.set_map(grown)
    return a, b


def test_sweeps_after_inflate(vhp, consumer_map):
    occ, grown = consumer_map
    a, b = _two_contexts(vhp, occ, grown)
    src = _some_free(grown, 5, seed=3)
    for dtype in (vhp.F64, vhp.F32):
        got, want = a.sweep_batch(src, dtype=dtype), b.sweep_batch(src, dtype=dtype)
        _same(got, want, "sweep_batch, dtype %d" % dtype)
        assert a.last_sweep_kernel() == b.last_sweep_kernel()
    # and they are sweeps of the inflated map, not of the one before
    b.set_map(occ)
    assert b.sweep_batch(src, dtype=vhp.F32).tobytes() != got.tobytes()


def _compare_solves(vhp, a, b, start, end, what):
    ra, rb = a.planner_solve(start, end, 0.25, 60), b.planner_solve(start, end, 0.25, 60)
    assert ra["status"] == rb["status"] == vhp.VHP_OK, (what, ra["status"], rb["status"])
    assert ra["n_pivots"] == rb["n_pivots"], what
    for name in ("pivots", "came_from", "vis_global", "vis_local"):
        _same(ra[name], rb[name], what + ": " + name)
    pa, pb = a.planner_path(), b.planner_path()
    assert pa["status"] == pb["status"] == vhp.VHP_OK and pa["length"] == pb["length"], what
    _same(pa["path"], pb["path"], what + ": path")
    return ra, pa


def test_planner_after_inflate(vhp, consumer_map):
    occ, grown = consumer_map
    a, b = _two_contexts(vhp, occ, grown)
    start, end = _some_free(grown, 2, seed=9)
    r, path = _compare_solves(vhp, a, b, start, end, "solve %r -> %r" % (start, end))
    assert r["n_pivots"] >= 1 and len(path["path"]) >= 2
    assert a.last_sweep_kernel() == b.last_sweep_kernel()
    # a start that the inflation has blocked
    lost = np.argwhere((occ != 0) & (grown == 0))
    assert len(lost)
    sy, sx = (int(v) for v in lost[len(lost) // 2])
    for ctx in (a, b):
        assert ctx.planner_solve((sx, sy), end, 0.25, 60)["status"] == vhp.VHP_ERR_START_OCCUPIED


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


def test_planner_reads_rebuilt_diagonal_maps(vhp):
    """at a side where one source takes the latency sweep the solve reads the diagonal maps, which vhp_inflate_map has to rebuild"""
    side = _smallest_latency_side()
    occ = np.ones((side, side), np.uint8)
    occ[side // 2, side // 2 - 1] = 0
    occ[side // 2 - 1, side // 2 - 1] = 0
    grown = ic.inflate(occ, ic.DISC, 1)
    assert grown[0, 0] and grown[-1, -1] and not np.array_equal(grown, occ)
    a, b = vhp.Context(0), vhp.Context(0)
    a.set_map(occ)
    a.inflate_map(radius=1)
    b.set_map(grown)
    _compare_solves(vhp, a, b, (0, 0), (side - 1, side - 1), "the %d x %d solve" % (side, side))
    assert a.last_sweep_kernel() == 4 and b.last_sweep_kernel() == 4
    # and the fields are those of the inflated map, not of the one before
    b.set_map(occ)
    before = b.planner_solve((0, 0), (side - 1, side - 1), 0.25, 60)
    after = a.planner_solve((0, 0), (side - 1, side - 1), 0.25, 60)
    assert before["vis_global"].tobytes() != after["vis_global"].tobytes()


# ---- 6. the fleet recipe: robots of three sizes on one map, one maps batch --------------------------------------------------------------
def test_fleet_of_three_sizes(vhp):
    occ = np.ones((48, 64), np.uint8)
    occ[0:40, 30:33] = 0      # a wall from the top, open for 8 rows at the bottom ...
    occ[20:25, 30:33] = 1     # ... with a gap of 5 cells in it
    classes = ((ic.DISC, 0), (ic.DISC, 4), (ic.SQUARE, 3))   # a point, a disc of radius 2 (the gap is 1 cell to it), a square that no longer fits
    want = np.stack([ic.inflate(occ, s, p) for s, p in classes])
    assert want[1, 22, 31] == 1 and not want[2, 20:25, 31].any() and want[2, 44:, 31].all()
    c = vhp.Context(0)
    c.set_map(occ)
    c.set_maps_windows(np.zeros((3, 2), np.int32), 64, 48)
    for k, (s, p) in enumerate(classes):
        c.inflate_maps(k, 1, p=p, shape=SHAPE_NAMES[s])
    _same(c.maps_occupancy(), want, "the three classes' maps")
    queries = [(10, 22, 55, 22)] * 3
    got = c.planner_solve_maps_batch(queries, [0, 1, 2], 0.25, 60, outputs="paths")
    ref = vhp.Context(0)
    ref.set_maps(want)
    exp = ref.planner_solve_maps_batch(queries, [0, 1, 2], 0.25, 60, outputs="paths")
    for q in range(3):
        for name in ("status", "n_pivots", "path_status", "length"):
            assert got[q][name] == exp[q][name], (q, name, got[q][name], exp[q][name])
        _same(got[q]["path"], exp[q]["path"], "class %d: path" % q)
    assert got[0]["status"] == vhp.VHP_OK and got[0]["path_status"] == vhp.VHP_OK and len(got[0]["path"]) >= 2
    others = [q for q in (1, 2) if got[q]["status"] != got[0]["status"] or got[q]["path"].tobytes() != got[0]["path"].tobytes()]
    assert others, "inflation that changes no route shows nothing"


# ---- 7. state and errors -------------------------------------------------------------------------------------------------------------
def test_errors(vhp):
    lib = vhp.load_library()
    occ = maps.random_rect_map(120, 97, 14, 3, 20, 3, 20, 5)
    out = np.zeros(120 * 97, np.uint8)
    c = vhp.Context(0)
    # nothing set
    assert lib.vhp_inflate_map(c.h, 0, 1, 0) == vhp.VHP_ERR_NO_MAP
    assert lib.vhp_inflate_maps(c.h, 0, 1, 0, 1, 0) == vhp.VHP_ERR_NO_MAP
    assert lib.vhp_map_occupancy(c.h, out.ctypes.data) == vhp.VHP_ERR_NO_MAP
    assert lib.vhp_map_occupancy_device(c.h, out.ctypes.data) == vhp.VHP_ERR_NO_MAP
    c.set_map(occ)
    assert lib.vhp_inflate_maps(c.h, 0, 1, 0, 1, 0) == vhp.VHP_ERR_NO_MAP   # (a single map is no stack)
    stack = np.stack([wc.random_map(40, 30, seed=k, blocked=0.1) for k in range(4)])
    c.set_maps(stack)
    start, end = (tuple(int(v) for v in p) for p in maps.free_sources(occ, 2, 9))
    assert c.planner_solve(start, end, 0.25, 60)["status"] == vhp.VHP_OK
    path = c.planner_path()
    assert path["status"] == vhp.VHP_OK
    # arguments: every refusal leaves the map, the stack and the plain solve's path as they were
    bad = ((3, 1, 0), (-1, 1, 0), (0, -1, 0), (0, 4225, 0), (1, 65, 0), (2, 65, 0), (0, 1, 2), (0, 1, 3), (0, 1, -1))   # (shape, p, flags)
    for shape, p, flags in bad:
        assert lib.vhp_inflate_map(c.h, shape, p, flags) == vhp.VHP_ERR_ARG, (shape, p, flags)
        assert lib.vhp_inflate_maps(c.h, 0, 4, shape, p, flags) == vhp.VHP_ERR_ARG, (shape, p, flags)
    n = 4
    for first, count in ((-1, 1), (n, 1), (0, n + 1), (0, 0), (3, 2), (0, -1)):
        assert lib.vhp_inflate_maps(c.h, first, count, 0, 1, 0) == vhp.VHP_ERR_ARG, (first, count)
    assert lib.vhp_map_occupancy(c.h, None) == vhp.VHP_ERR_ARG
    assert lib.vhp_map_occupancy_device(c.h, None) == vhp.VHP_ERR_ARG
    with pytest.raises(vhp.VhpError) as e:
        c.inflate_map(p=4225)
    assert e.value.code == vhp.VHP_ERR_ARG
    with pytest.raises(vhp.VhpError) as e:
        c.inflate_maps(2, 3, p=1)
    assert e.value.code == vhp.VHP_ERR_ARG and c.n_maps == 4
    _same(c.map_occupancy(), (occ != 0).astype(np.uint8), "the map after the refused calls")
    _same(c.maps_occupancy(), stack, "the stack after the refused calls")
    after = c.planner_path()
    assert after["status"] == vhp.VHP_OK and after["length"] == path["length"] and after["path"].tolist() == path["path"].tolist()
    # the largest footprints are taken
    for shape, p in ((0, 4224), (1, 64), (2, 64)):
        assert lib.vhp_inflate_map(c.h, shape, p, 1) == vhp.VHP_OK
        assert not c.map_occupancy().any()   # (120 x 97 with a blocked border: nothing within 64 cells of an edge is left)


def test_state_after_inflate_map(vhp):
    occ = maps.random_rect_map(120, 97, 14, 3, 20, 3, 20, 5)
    stack = np.stack([wc.random_map(40, 30, seed=k, blocked=0.1) for k in range(3)])
    c = vhp.Context(0)
    c.set_map(occ)
    c.set_maps(stack)
    start, end = (tuple(int(v) for v in p) for p in maps.free_sources(ic.inflate(occ, ic.DISC, 1), 2, 9))
    assert c.planner_solve(start, end, 0.25, 60)["status"] == vhp.VHP_OK
    pts = _some_free(stack[1], 2, seed=1)
    c.planner_solve_maps_batch([pts[0] + pts[1]], [1], 0.25, 40)
    c.set_option("field_stride", 120 * 97 + 64)
    assert c.field_stride == 120 * 97 + 64
    c.sweep_batch([start])
    for p in (1, 0):   # (p = 0 changes no cell and does to the state what any p does)
        ms = c.last_elapsed_ms()
        c.inflate_map(p=p)
        assert c.last_elapsed_ms() == ms   # (not timed)
        assert c.field_stride == 0
        # the plain solve's results are gone, as after set_map ...
        ptrs = [C.c_void_p() for _ in range(4)]
        assert c.lib.vhp_planner_results_device(c.h, *[C.byref(q) for q in ptrs]) == vhp.VHP_ERR_ARG
        with pytest.raises(vhp.VhpError):
            c.planner_path()
        # ... the stack and its maps batch are not
        _same(c.maps_occupancy(), stack, "the stack after inflate_map")
        assert c.lib.vhp_planner_maps_batch_results(c.h, 0, None, None, None, None) == vhp.VHP_OK
        _same(c.map_occupancy(), ic.inflate(occ, ic.DISC, 1), "the map after inflate_map(p=%d)" % p)
        # (field_stride is 0 in the library too: device-form fields are packed, as on a fresh context)
        assert c.planner_solve(start, end, 0.25, 60)["status"] == vhp.VHP_OK
        c.set_option("field_stride", 120 * 97 + 64)
    import torch
    grown = ic.inflate(occ, ic.DISC, 1)
    fresh = vhp.Context(0)
    fresh.set_map(grown)
    src = np.array(_some_free(grown, 2, seed=2), np.int32)
    d_src = torch.from_numpy(src).cuda()
    outs = []
    c.inflate_map(p=0)   # (drops the stride set at the end of the loop)
    for ctx in (c, fresh):
        buf = torch.full((2 * 120 * 97 + 64,), -1.0, dtype=torch.float64, device="cuda")
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.sweep_batch_device(d_src.data_ptr(), 2, buf.data_ptr())
        ctx.sync()
        ctx.set_stream(None)
        outs.append(buf.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes() and (outs[0][-64:] == -1.0).all()


def test_state_after_inflate_maps(vhp):
    occ = maps.random_rect_map(120, 97, 14, 3, 20, 3, 20, 5)
    stack = np.stack([wc.random_map(40, 30, seed=k, blocked=0.1) for k in range(3)])
    c = vhp.Context(0)
    c.set_map(occ)
    c.set_maps(stack)
    start, end = (tuple(int(v) for v in p) for p in maps.free_sources(occ, 2, 9))
    want = c.planner_solve(start, end, 0.25, 60)
    assert want["status"] == vhp.VHP_OK
    path = c.planner_path()
    pts = _some_free(ic.inflate(stack[1], ic.DISC, 1), 2, seed=1)
    query = [pts[0] + pts[1]]
    first = c.planner_solve_maps_batch(query, [1], 0.25, 40, outputs="paths")   # (builds the stack's diagonal maps where it takes the latency sweep)
    assert c.planner_maps_batch_group() >= 1
    c.set_option("field_stride", 120 * 97 + 64)
    c.sweep_batch([start])
    for p in (1, 0):
        ms = c.last_elapsed_ms()
        c.inflate_maps(1, 1, p=p)
        assert c.last_elapsed_ms() == ms and c.field_stride == 120 * 97 + 64 and c.n_maps == 3
        # the maps batch's results are gone ...
        assert c.lib.vhp_planner_maps_batch_results(c.h, 0, None, None, None, None) == vhp.VHP_ERR_ARG
        assert c.planner_maps_batch_group() == 0
        # ... the single map and the plain solve are not
        _same(c.map_occupancy(), (occ != 0).astype(np.uint8), "the single map after inflate_maps")
        after = c.planner_path()
        assert after["status"] == vhp.VHP_OK and after["length"] == path["length"] and after["path"].tolist() == path["path"].tolist()
        # a maps batch on the inflated map reads diagonal maps built from it: the same as on a stack set from bytes
        grown = stack.copy()
        grown[1] = ic.inflate(stack[1], ic.DISC, 1)
        ref = vhp.Context(0)
        ref.set_maps(grown)
        got, exp = (x.planner_solve_maps_batch(query, [1], 0.25, 40, outputs="paths") for x in (c, ref))
        assert c.last_sweep_kernel() == ref.last_sweep_kernel()
        assert got[0]["status"] == exp[0]["status"] and got[0]["length"] == exp[0]["length"]
        _same(got[0]["path"], exp[0]["path"], "the maps batch after inflate_maps(p=%d)" % p)
    assert first[0]["status"] == vhp.VHP_OK
    again = c.planner_solve(start, end, 0.25, 60)
    for name in ("came_from", "vis_global", "vis_local", "pivots"):
        assert again[name].tobytes() == want[name].tobytes(), name


def test_one_context_reused(vhp):
    """inflate, a set_map of another size, inflate again: the same bytes as fresh contexts (the scratch of a larger map behind a
    smaller one, and the other way round)"""
    big = wc.random_map(130, 129, seed=1, blocked=0.02)
    small = wc.random_map(63, 5, seed=2, blocked=0.05)
    c = vhp.Context(0)
    for occ, (shape, p, border) in ((big, (ic.DISC, 8, False)), (small, (ic.SQUARE, 2, True)), (big, (ic.DIAMOND, 3, True)), (small, (ic.DISC, 4096, False))):
        c.set_map(occ)
        c.inflate_map(p=p, shape=SHAPE_NAMES[shape], border=border)
        fresh = vhp.Context(0)
        fresh.set_map(occ)
        fresh.inflate_map(p=p, shape=SHAPE_NAMES[shape], border=border)
        want = ic.inflate(occ, shape, p, border)
        _same(c.map_occupancy(), want, "the reused context")
        _same(fresh.map_occupancy(), want, "the fresh context")
        # twice on one map composes
        c.inflate_map(p=1)
        _same(c.map_occupancy(), ic.inflate(want, ic.DISC, 1), "inflated twice")
