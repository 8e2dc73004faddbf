"""The kernels on the inputs the other parity tests filter out, through the C ABI against the oracle, bit for bit: sources on
blocked cells (corner, border, interior, a free cell walled in on all 8 sides), the same source more than once in one batch,
maps that are all blocked, all free, or free only at the source, and occupancy bytes other than 1 for a free cell (the kernels
test `!= 0`; the reference's isFree too).  Every batch runs through each batch kernel (vhp_set_option "kernel" 1, 3, 4), in fp64
and fp32, on a width of every build (a multiple of 8, an even non-multiple of 8, an odd one, and sides above 1024: several
workgroups per unit), through the host and the device entry points; device outputs start as NaN, so every cell must be
written.  The CPU simulators get the same inputs in tests/test_pool_sim.py and tests/test_lat_sim.py."""
import numpy as np
import pytest

import maps
from edge_inputs import edge_map, whole_maps

pytestmark = pytest.mark.gpu

# (nx, ny): the pool sweep's build for multiples of 8 / its ANYW build; the latency sweep's odd-pitch build; several workgroups per unit
GRIDS = [(200, 163), (202, 163), (101, 101), (1104, 1030)]
DTYPES = {"f64": np.float64, "f32": np.float32}


@pytest.fixture(scope="module")
def vhp():
    import torch  # noqa: F401
    import vhp_amd
    return vhp_amd


def _assert_same(got, want, what):
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
        y, x = bad[0][-2:]
        raise AssertionError("%s: %d cells differ, first at (x=%d,y=%d): got %r want %r" % (what, len(bad), x, y, got[tuple(bad[0])], want[tuple(bad[0])]))


_WANT = {}


def _oracle_fields(oracle, occ, src, key):
    """the oracle's fields of a batch (one sweep per distinct source; cached per map)"""
    if key not in _WANT:
        per = {}
        for sx, sy in map(tuple, src.tolist()):
            if (sx, sy) not in per:
                per[(sx, sy)] = oracle.sweep_full(occ, sx, sy)
        _WANT[key] = np.stack([per[tuple(s)] for s in src.tolist()])
    return _WANT[key]


def _run_all_entries(vhp, c, occ, src, dtype, kernel, want, what):
    """the host entry point, the device one into a packed buffer and into one padded by field_stride: every field against `want`"""
    import torch
    ny, nx = occ.shape
    vdt = vhp.F64 if dtype == "f64" else vhp.F32
    tdt = torch.float64 if dtype == "f64" else torch.float32
    want = want.astype(DTYPES[dtype])
    got = c.sweep_batch(src, dtype=vdt)
    assert c.last_sweep_kernel() == kernel, (what, c.last_sweep_kernel())
    for k, (sx, sy) in enumerate(src):
        _assert_same(got[k], want[k], "%s host, source %d (%d,%d)" % (what, k, sx, sy))
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    d_src = torch.from_numpy(np.ascontiguousarray(src, np.int32)).cuda()
    cells = nx * ny
    for pad in (0, 5):
        stride = cells + pad
        c.set_option("field_stride", stride if pad else 0)
        buf = torch.full((len(src) * stride,), float("nan"), dtype=tdt, device="cuda")
        c.sweep_batch_device(d_src.data_ptr(), len(src), buf.data_ptr(), dtype=vdt)
        c.sync()
        assert c.last_sweep_kernel() == kernel, (what, c.last_sweep_kernel())
        out = buf.cpu().numpy().reshape(len(src), stride)
        assert np.isnan(out[:, cells:]).all(), "%s: padding written" % what
        for k, (sx, sy) in enumerate(src):
            _assert_same(out[k, :cells].reshape(ny, nx), want[k], "%s device stride +%d, source %d (%d,%d)" % (what, pad, k, sx, sy))
    c.set_option("field_stride", 0)
    c.set_stream(0)


@pytest.mark.parametrize("nx,ny", GRIDS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kernel", [1, 3, 4])
def test_blocked_and_repeated_sources(vhp, oracle, kernel, dtype, nx, ny):
    occ, src = edge_map(nx, ny, nx * 3 + ny)
    want = _oracle_fields(oracle, occ, src, ("edge", nx, ny))
    c = vhp.Context(0)
    c.set_map(occ)
    c.set_option("kernel", kernel)
    _run_all_entries(vhp, c, occ, src, dtype, kernel, want, "%dx%d %s kernel %d" % (nx, ny, dtype, kernel))


@pytest.mark.parametrize("nx,ny", [(200, 163), (101, 101)])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kernel", [1, 3, 4])
def test_whole_map_cases(vhp, oracle, kernel, dtype, nx, ny):
    for name, occ, src in whole_maps(nx, ny):
        want = _oracle_fields(oracle, occ, src, (name, nx, ny))
        c = vhp.Context(0)
        c.set_map(occ)
        c.set_option("kernel", kernel)
        _run_all_entries(vhp, c, occ, src, dtype, kernel, want, "%dx%d %s, %s kernel %d" % (nx, ny, name, dtype, kernel))


def test_auto_selected_large_batch_with_blocked_and_repeated_sources(vhp, oracle):
    # more than 32 sources on 1000^2: the library picks the kernel and launch shape the benchmark runs
    occ = maps.random_rect_map(1000, 1000, 50, 20, 100, 20, 100, 1)
    free = maps.free_sources(occ, 40, 3)
    blocked = np.argwhere(occ == 0)[:: max(1, int((occ == 0).sum()) // 6)][:6][:, ::-1]
    src = np.concatenate([free[:20], blocked, free[:3], free[20:], free[5:6], blocked[:2]]).astype(np.int32)
    assert len(src) > 32 and (occ[src[:, 1], src[:, 0]] == 0).sum() >= 8
    want = _oracle_fields(oracle, occ, src, ("auto", 1000, 1000))
    c = vhp.Context(0)
    c.set_map(occ)
    for dtype in ("f64", "f32"):
        got = c.sweep_batch(src, dtype=vhp.F64 if dtype == "f64" else vhp.F32)
        assert c.last_sweep_kernel() in (1, 3, 4)
        for k, (sx, sy) in enumerate(src):
            _assert_same(got[k], want[k].astype(DTYPES[dtype]), "1000^2 auto (kernel %d) %s, source %d (%d,%d)" % (c.last_sweep_kernel(), dtype, k, sx, sy))


# ---- occupancy bytes other than 1 for a free cell --------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[2, 128, 255])
def byte_map(request, oracle):
    """(free byte, the map with that byte for free cells, the same map in 0/1, a batch with blocked and repeated sources)"""
    occ01, src = edge_map(202, 163, 77)
    raw = (occ01 * np.uint8(request.param)).astype(np.uint8)
    return request.param, raw, occ01, src


def _set(vhp, c, raw, how):
    import torch
    if how == "host":
        c.set_map(raw)
    else:
        d = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
        c.set_map_device(d.data_ptr(), raw.shape[1], raw.shape[0])
        torch.cuda.synchronize()
        c._keep = d


@pytest.mark.parametrize("how", ["host", "device"])
def test_occupancy_bytes_batch_kernels(vhp, oracle, byte_map, how):
    byte, raw, occ01, src = byte_map
    want = _oracle_fields(oracle, occ01, src, ("bytes01",))
    for k, (sx, sy) in enumerate(src):
        assert oracle.sweep_full(raw, int(sx), int(sy)).tobytes() == want[k].tobytes(), "the oracle reads byte %d as free" % byte
    for kernel in (1, 3, 4):
        c = vhp.Context(0)
        _set(vhp, c, raw, how)
        c.set_option("kernel", kernel)
        for dtype in ("f64", "f32"):
            got = c.sweep_batch(src, dtype=vhp.F64 if dtype == "f64" else vhp.F32)
            assert c.last_sweep_kernel() == kernel
            for k, (sx, sy) in enumerate(src):
                _assert_same(got[k], want[k].astype(DTYPES[dtype]), "free byte %d via %s map, kernel %d %s, source %d (%d,%d)" % (byte, how, kernel, dtype, k, sx, sy))


@pytest.mark.parametrize("how", ["host", "device"])
def test_occupancy_bytes_queue_offset_variant_raycast(vhp, oracle, byte_map, how):
    byte, raw, occ01, src = byte_map
    c = vhp.Context(0)
    _set(vhp, c, raw, how)
    got = c.sweep_batch(src, variant=vhp.SWEEP_QUEUE)
    for k, (sx, sy) in enumerate(src):
        want = oracle.sweep_queue(occ01, int(sx), int(sy))
        assert oracle.sweep_queue(raw, int(sx), int(sy)).tobytes() == want.tobytes()
        _assert_same(got[k], want, "queue variant, free byte %d via %s map, source %d (%d,%d)" % (byte, how, k, sx, sy))
    few = src[:5]
    got = c.sweep_batch_offset(few, 1.0)
    for k, (sx, sy) in enumerate(few):
        want = oracle.sweep_full_offset(occ01, int(sx), int(sy), 1.0)
        assert oracle.sweep_full_offset(raw, int(sx), int(sy), 1.0).tobytes() == want.tobytes()
        _assert_same(got[k], want, "offset sweep, free byte %d via %s map, source %d" % (byte, how, k))
    got = c.sweep_batch_variant(few, 0.9, 1.5)
    for k, (sx, sy) in enumerate(few):
        want = oracle.sweep_matlab(occ01, int(sx), int(sy), 0.9, 1.5)
        assert oracle.sweep_matlab(raw, int(sx), int(sy), 0.9, 1.5).tobytes() == want.tobytes()
        _assert_same(got[k], want, "MATLAB variant, free byte %d via %s map, source %d" % (byte, how, k))
    for sx, sy in few[[0, 2, 3]]:
        want = oracle.raycast_all(occ01, int(sx), int(sy))
        assert oracle.raycast_all(raw, int(sx), int(sy)).tobytes() == want.tobytes()
        _assert_same(c.raycast_all(int(sx), int(sy)), want, "raycast_all, free byte %d via %s map, source (%d,%d)" % (byte, how, sx, sy))


def test_occupancy_byte_255_planner(vhp, oracle):
    # start and end on 255-valued cells: not START_OCCUPIED, and the oracle's solve on the same map
    occ01 = maps.random_rect_map(160, 131, 22, 4, 30, 4, 30, 1)
    start, end = (2, 2), (150, 120)
    occ01[start[1], start[0]] = occ01[end[1], end[0]] = 1
    raw = occ01 * np.uint8(255)
    c = vhp.Context(0)
    c.set_map(raw)
    got = c.planner_solve(start, end, 0.25, 60)
    want = oracle.solve(occ01, start, end, 0.25, 60)
    assert got["status"] != vhp.VHP_ERR_START_OCCUPIED and got["status"] != vhp.VHP_ERR_END_OCCUPIED, got["status"]
    assert oracle.solve(raw, start, end, 0.25, 60)["pivots"].tolist() == want["pivots"].tolist()
    assert got["status"] == want["status"] and got["n_pivots"] == want["n_pivots"], (got["status"], want["status"], got["n_pivots"], want["n_pivots"])
    assert got["pivots"].tolist() == want["pivots"].tolist()
    for name in ("came_from", "vis_global", "vis_local"):
        _assert_same(got[name], want[name], "planner on 255-valued free cells: " + name)


@pytest.mark.parametrize("nx,ny", [(120, 97), (101, 101)])
def test_queue_variant_blocked_and_repeated_sources(vhp, oracle, nx, ny):
    occ, src = edge_map(nx, ny, nx + 5)
    c = vhp.Context(0)
    c.set_map(occ)
    got = c.sweep_batch(src, variant=vhp.SWEEP_QUEUE)
    for k, (sx, sy) in enumerate(src):
        _assert_same(got[k], oracle.sweep_queue(occ, int(sx), int(sy)), "queue variant %dx%d, source %d (%d,%d)" % (nx, ny, k, sx, sy))
