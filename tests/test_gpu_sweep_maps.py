"""The sweep over a stack of maps (vhp_set_maps + vhp_sweep_maps_batch): field i is computeVisibility from source i on its own map,
bit for bit what vhp_set_map(that map) + vhp_sweep_batch gives and what the CPU oracle gives -- in both dtypes, in every front-sweep
shape the options can force, in the device form with strides and offsets --, a rejected source or map index is reported like a
source outside the grid, and the stack leaves the single map, the planner's state and the timing bookkeeping as they should be."""
import ctypes as C

import numpy as np
import pytest
from importlib import import_module

pytestmark = pytest.mark.gpu

synth = import_module("visibility-heuristic-path-planner_amd.synth")


@pytest.fixture(scope="module")
def vhp():
    import torch  # noqa: F401  (first, so the extension shares torch's HIP runtime)
    import vhp_amd
    return vhp_amd


def _stack(n_maps, nx, ny, seed, nb=None, wmax=None):
    nb = nb if nb is not None else max(4, nx * ny // 500)
    wmax = wmax if wmax is not None else max(4, min(nx, ny) // 5)
    return np.stack([synth.random_rect_map(nx, ny, nb, 2, wmax, 2, wmax, seed=seed + 17 * k) for k in range(n_maps)])


def _spread_sources(occ, n, seed, used_maps):
    """n sources over the maps in `used_maps`, with repeats, edges and corners (on free or blocked cells alike)"""
    _, ny, nx = occ.shape
    rng = np.random.default_rng(seed)
    special = [(0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1), (0, ny // 2), (nx - 1, ny // 3), (nx // 2, 0), (nx // 3, ny - 1)]
    src, idx = [], []
    for i in range(n):
        k = int(used_maps[i % len(used_maps)]) if i < 2 * len(used_maps) else int(rng.choice(used_maps))
        if i % 7 == 3:
            x, y = special[(i // 7) % len(special)]
        elif i % 11 == 5 and src:
            x, y = src[-1]   # the same position again, on another map
        else:
            x, y = int(rng.integers(nx)), int(rng.integers(ny))
        src.append((x, y))
        idx.append(k)
    return np.array(src, np.int32), np.array(idx, np.int32)


def _assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        y, x = bad[0]
        raise AssertionError("%s: %d cells differ, first (x=%d,y=%d): %r vs %r" % (what, len(bad), x, y, got[y, x], want[y, x]))


def _single_map_fields(vhp, occ, src, idx, dtype, opts):
    """what set_map(map k) + sweep_batch with "kernel" = 1 and the same options gives, field by field"""
    c = vhp.Context(0)
    out = np.empty((len(src),) + occ.shape[1:], np.float64 if dtype == vhp.F64 else np.float32)
    for k in sorted(set(idx.tolist())):
        c.set_map(occ[k])
        c.set_option("kernel", 1)
        for key, v in opts.items():
            c.set_option(key, v)
        sel = np.nonzero(idx == k)[0]
        out[sel] = c.sweep_batch(src[sel], dtype=dtype)
        assert c.last_sweep_kernel() == 1
    return out


def _maps_ctx(vhp, occ, opts=None):
    c = vhp.Context(0)
    c.set_maps(occ)
    for key, v in (opts or {}).items():
        c.set_option(key, v)
    return c


def test_oracle_parity_101(vhp, oracle):
    occ = _stack(24, 101, 101, seed=11)
    src, idx = _spread_sources(occ, 200, seed=5, used_maps=np.arange(20))   # (maps 20..23: no source)
    c = _maps_ctx(vhp, occ)
    got64 = c.sweep_maps_batch(src, idx)
    got32 = c.sweep_maps_batch(src, idx, dtype=vhp.F32)
    assert got64.shape == (200, 101, 101) and got32.dtype == np.float32
    for i, ((sx, sy), k) in enumerate(zip(src.tolist(), idx.tolist())):
        want = oracle.sweep_full(occ[k], sx, sy)
        _assert_same(got64[i], want, "source %d (%d,%d) on map %d" % (i, sx, sy, k))
        _assert_same(got32[i], want.astype(np.float32), "fp32 source %d (%d,%d) on map %d" % (i, sx, sy, k))


@pytest.mark.parametrize("nx,ny", [(97, 103), (250, 130)])
def test_oracle_parity_other_sizes(vhp, oracle, nx, ny):
    occ = _stack(5, nx, ny, seed=nx + ny)
    src, idx = _spread_sources(occ, 24, seed=nx, used_maps=np.arange(5))
    c = _maps_ctx(vhp, occ)
    for dtype in (vhp.F64, vhp.F32):
        got = c.sweep_maps_batch(src, idx, dtype=dtype)
        for i, ((sx, sy), k) in enumerate(zip(src.tolist(), idx.tolist())):
            want = oracle.sweep_full(occ[k], sx, sy)
            _assert_same(got[i], want if dtype == vhp.F64 else want.astype(np.float32), "%dx%d source %d on map %d" % (nx, ny, i, k))


SHAPES = [dict(rows_per_lane=1), dict(rows_per_lane=2), dict(rows_per_lane=4), dict(strips=1), dict(strips=4), dict(strips=8),
          dict(multi_round=1), dict(multi_round=1, rows_per_lane=2), dict(pack=1, strips=8, rows_per_lane=1), dict(slide=0), dict(slide=1)]


@pytest.mark.parametrize("opts", SHAPES, ids=lambda o: ",".join("%s=%d" % kv for kv in o.items()))
def test_equal_to_the_single_map_path(vhp, opts):
    occ = _stack(6, 101, 101, seed=3)
    src, idx = _spread_sources(occ, 48, seed=len(opts) * 7 + sum(opts.values()), used_maps=np.arange(6))
    c = _maps_ctx(vhp, occ, opts)
    for dtype in (vhp.F64, vhp.F32) if "rows_per_lane" not in opts or opts["rows_per_lane"] == 1 else (vhp.F64,):
        got = c.sweep_maps_batch(src, idx, dtype=dtype)
        assert c.last_sweep_kernel() == 1
        want = _single_map_fields(vhp, occ, src, idx, dtype, opts)
        for i in range(len(src)):
            _assert_same(got[i], want[i], "%r dtype %d source %d on map %d" % (opts, dtype, i, idx[i]))


def test_equal_to_the_single_map_path_multi_round(vhp):
    # a front longer than one workgroup's W*64*R = 64 rows: the multi-round build with its boundary scratch
    occ = _stack(3, 700, 500, seed=9, nb=60, wmax=60)
    src, idx = _spread_sources(occ, 6, seed=2, used_maps=np.arange(3))
    opts = dict(rows_per_lane=1, strips=1)
    c = _maps_ctx(vhp, occ, opts)
    got = c.sweep_maps_batch(src, idx)
    want = _single_map_fields(vhp, occ, src, idx, vhp.F64, opts)
    for i in range(len(src)):
        _assert_same(got[i], want[i], "700x500 R=1 W=1 source %d on map %d" % (i, idx[i]))


def test_oracle_parity_1000(vhp, oracle):
    occ = _stack(3, 1000, 1000, seed=21, nb=200, wmax=60)
    src = np.concatenate([synth.free_sources(occ[k], 3, seed=40 + k) for k in range(3)])
    idx = np.repeat(np.arange(3, dtype=np.int32), 3)
    got = _maps_ctx(vhp, occ).sweep_maps_batch(src, idx)
    for i, ((sx, sy), k) in enumerate(zip(src.tolist(), idx.tolist())):
        _assert_same(got[i], oracle.sweep_full(occ[k], sx, sy), "1000^2 source %d on map %d" % (i, k))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_device_form_stride_and_offset(vhp, dtype):
    import torch
    occ = _stack(8, 101, 101, seed=31)
    src, idx = _spread_sources(occ, 40, seed=8, used_maps=np.arange(8))
    dt, dv = (torch.float64, vhp.F64) if dtype == "f64" else (torch.float32, vhp.F32)
    c = _maps_ctx(vhp, occ)
    want = c.sweep_maps_batch(src, idx, dtype=dv)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    d_src = torch.from_numpy(src).cuda()
    d_idx = torch.from_numpy(idx).cuda()
    cells = 101 * 101
    # packed, NaN everywhere first: every cell is written
    d_out = torch.full((len(src), 101, 101), float("nan"), dtype=dt, device="cuda")
    c.sweep_maps_batch_device(d_src.data_ptr(), d_idx.data_ptr(), len(src), d_out.data_ptr(), dtype=dv)
    c.sync()
    got = d_out.cpu().numpy()
    assert not np.isnan(got).any()
    for i in range(len(src)):
        _assert_same(got[i], want[i], "device %s source %d" % (dtype, i))
    # a stride of its own and a start 3 elements into the buffer
    stride, off = cells + 37, 3
    buf = torch.full((off + len(src) * stride,), float("nan"), dtype=dt, device="cuda")
    c.set_option("field_stride", stride)
    c.sweep_maps_batch_device(d_src.data_ptr(), d_idx.data_ptr(), len(src), buf.data_ptr() + off * buf.element_size(), dtype=dv)
    c.sync()
    b = buf.cpu().numpy()
    assert np.isnan(b[:off]).all()
    for i in range(len(src)):
        lo = off + i * stride
        _assert_same(b[lo:lo + cells].reshape(101, 101), want[i], "strided device %s source %d" % (dtype, i))
        assert np.isnan(b[lo + cells:lo + stride]).all(), "source %d wrote past its field" % i
    # a stride below a field
    c.set_option("field_stride", cells - 1)
    rc = c.lib.vhp_sweep_maps_batch_device(c.h, C.c_void_p(d_src.data_ptr()), C.c_void_p(d_idx.data_ptr()), len(src), dv, C.c_void_p(buf.data_ptr()))
    assert rc == vhp.VHP_ERR_ARG
    # an element pointer that is not aligned to its type
    c.set_option("field_stride", 0)
    rc = c.lib.vhp_sweep_maps_batch_device(c.h, C.c_void_p(d_src.data_ptr()), C.c_void_p(d_idx.data_ptr()), len(src), dv, C.c_void_p(buf.data_ptr() + 2))
    assert rc == vhp.VHP_ERR_ARG


def test_rejected_sources_and_map_indices(vhp):
    import torch
    occ = _stack(4, 101, 101, seed=41)
    src, idx = _spread_sources(occ, 12, seed=4, used_maps=np.arange(4))
    bad_src, bad_idx = src.copy(), idx.copy()
    bad_idx[2] = -1
    bad_idx[5] = 4          # n_maps
    bad_src[7] = (101, 3)   # outside the grid
    bad_src[9] = (5, -1)
    rejected = {2, 5, 7, 9}
    c = _maps_ctx(vhp, occ)
    want = c.sweep_maps_batch(src, idx)
    out = np.full((len(src), 101, 101), 7.0)
    rc = c.lib.vhp_sweep_maps_batch(c.h, bad_src.ctypes.data, bad_idx.ctypes.data, len(src), vhp.F64, out.ctypes.data)
    assert rc == vhp.VHP_ERR_SOURCE_OOB
    for i in range(len(src)):
        if i in rejected:
            assert not out[i].any(), "rejected source %d: field not zero" % i
        else:
            _assert_same(out[i], want[i], "host form, source %d beside rejected ones" % i)
    assert c.lib.vhp_sync(c.h) == vhp.VHP_OK   # (the flag was consumed by the call)
    # device form: the rejected fields are not written, vhp_sync reports it
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    d_out = torch.full((len(src), 101, 101), float("nan"), dtype=torch.float64, device="cuda")
    d_src, d_idx = torch.from_numpy(bad_src).cuda(), torch.from_numpy(bad_idx).cuda()
    c.sweep_maps_batch_device(d_src.data_ptr(), d_idx.data_ptr(), len(src), d_out.data_ptr())
    assert c.lib.vhp_sync(c.h) == vhp.VHP_ERR_SOURCE_OOB
    assert c.lib.vhp_sync(c.h) == vhp.VHP_OK
    got = d_out.cpu().numpy()
    for i in range(len(src)):
        if i in rejected:
            assert np.isnan(got[i]).all(), "rejected source %d: field written" % i
        else:
            _assert_same(got[i], want[i], "device form, source %d beside rejected ones" % i)


def test_argument_errors(vhp):
    occ = _stack(2, 33, 17, seed=1)
    src = np.array([[1, 1]], np.int32)
    idx = np.array([0], np.int32)
    out = np.zeros((1, 17, 33))
    c = vhp.Context(0)
    lib, h = c.lib, c.h
    # before any stack: no map (a single map does not count)
    assert lib.vhp_sweep_maps_batch(h, src.ctypes.data, idx.ctypes.data, 1, vhp.F64, out.ctypes.data) == vhp.VHP_ERR_NO_MAP
    c.set_map(occ[0])
    assert lib.vhp_sweep_maps_batch(h, src.ctypes.data, idx.ctypes.data, 1, vhp.F64, out.ctypes.data) == vhp.VHP_ERR_NO_MAP
    assert lib.vhp_sweep_maps_batch_device(h, src.ctypes.data, idx.ctypes.data, 1, vhp.F64, out.ctypes.data) == vhp.VHP_ERR_NO_MAP
    p = occ.ctypes.data
    assert lib.vhp_set_maps(h, p, 0, 33, 17) == vhp.VHP_ERR_ARG
    assert lib.vhp_set_maps(h, p, -1, 33, 17) == vhp.VHP_ERR_ARG
    assert lib.vhp_set_maps(h, None, 2, 33, 17) == vhp.VHP_ERR_ARG
    assert lib.vhp_set_maps(h, p, 2, 0, 17) == vhp.VHP_ERR_ARG
    assert lib.vhp_set_maps(h, p, 2, 33, 0) == vhp.VHP_ERR_ARG
    assert lib.vhp_set_maps(h, p, 1, 8193, 1) == vhp.VHP_ERR_TOO_LARGE
    assert lib.vhp_set_maps(h, p, 1, 1, 8193) == vhp.VHP_ERR_TOO_LARGE
    assert lib.vhp_set_maps_device(h, None, 2, 33, 17) == vhp.VHP_ERR_ARG
    assert lib.vhp_set_maps_device(h, p, 0, 33, 17) == vhp.VHP_ERR_ARG
    assert lib.vhp_set_maps(None, p, 2, 33, 17) == vhp.VHP_ERR_ARG
    c.set_maps(occ)
    assert lib.vhp_sweep_maps_batch(h, None, idx.ctypes.data, 1, vhp.F64, out.ctypes.data) == vhp.VHP_ERR_ARG
    assert lib.vhp_sweep_maps_batch(h, src.ctypes.data, None, 1, vhp.F64, out.ctypes.data) == vhp.VHP_ERR_ARG
    assert lib.vhp_sweep_maps_batch(h, src.ctypes.data, idx.ctypes.data, 1, vhp.F64, None) == vhp.VHP_ERR_ARG
    assert lib.vhp_sweep_maps_batch(h, src.ctypes.data, idx.ctypes.data, -1, vhp.F64, out.ctypes.data) == vhp.VHP_ERR_ARG
    assert lib.vhp_sweep_maps_batch(h, src.ctypes.data, idx.ctypes.data, 1, 7, out.ctypes.data) == vhp.VHP_ERR_ARG
    assert lib.vhp_sweep_maps_batch(h, src.ctypes.data, idx.ctypes.data, 0, vhp.F64, out.ctypes.data) == vhp.VHP_OK
    assert lib.vhp_sweep_maps_batch_device(h, None, idx.ctypes.data, 1, vhp.F64, out.ctypes.data) == vhp.VHP_ERR_ARG
    assert lib.vhp_sweep_maps_batch_device(h, src.ctypes.data, None, 1, vhp.F64, out.ctypes.data) == vhp.VHP_ERR_ARG
    assert lib.vhp_sweep_maps_batch_device(h, src.ctypes.data, idx.ctypes.data, 1, vhp.F64, None) == vhp.VHP_ERR_ARG
    # a failed vhp_set_maps leaves no stack
    assert lib.vhp_set_maps(h, p, 1, 8193, 1) == vhp.VHP_ERR_TOO_LARGE
    assert lib.vhp_set_maps(h, p, 2, 33, 17) == vhp.VHP_OK
    assert lib.vhp_sweep_maps_batch(h, src.ctypes.data, idx.ctypes.data, 1, vhp.F64, out.ctypes.data) == vhp.VHP_OK


def test_one_map_equals_sweep_batch(vhp):
    occ = synth.random_rect_map(101, 101, 25, 2, 20, 2, 20, seed=1)
    src = synth.free_sources(occ, 16, seed=3)
    c = vhp.Context(0)
    c.set_map(occ)
    c.set_option("kernel", 1)
    want = c.sweep_batch(src)
    c.set_maps(occ[None])
    got = c.sweep_maps_batch(src, np.zeros(len(src), np.int32))
    for i in range(len(src)):
        _assert_same(got[i], want[i], "n_maps = 1, source %d" % i)


def test_stack_leaves_the_single_map_and_the_planner_alone(vhp):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def fetch(p, shape, dtype):
        a = np.empty(shape, dtype)
        assert hip.hipMemcpy(a.ctypes.data, p, a.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        return a

    occ = synth.random_rect_map(160, 122, 20, 3, 24, 3, 24, seed=2)
    ny, nx = occ.shape
    src = synth.free_sources(occ, 6, seed=5)
    c = vhp.Context(0)
    c.set_map(occ)
    before = c.sweep_batch(src)
    (sx, sy), (ex, ey) = src[0].tolist(), src[1].tolist()
    rc, n_piv, ptr = c.planner_solve_device((sx, sy), (ex, ey), 0.1, 100)
    assert rc in (vhp.VHP_OK, vhp.VHP_ERR_MAX_ITER) and ptr
    read = lambda q: [fetch(q["labels"], (ny, nx), np.uint32), fetch(q["vis_global"], (ny, nx), np.float64),
                      fetch(q["vis_local"], (ny, nx), np.float64), fetch(q["pivots"], (n_piv + 1, 2), np.int32)]
    plan_before = read(ptr)
    stack = _stack(5, 101, 101, seed=51)
    s_src, s_idx = _spread_sources(stack, 20, seed=6, used_maps=np.arange(5))
    c.set_maps(stack)
    fields = c.sweep_maps_batch(s_src, s_idx)
    _assert_same(c.sweep_batch(src), before, "sweep_batch after set_maps")
    p = [C.c_void_p() for _ in range(4)]
    assert c.lib.vhp_planner_results_device(c.h, *[C.byref(v) for v in p]) == vhp.VHP_OK
    after = read(dict(labels=p[0].value, vis_global=p[1].value, vis_local=p[2].value, pivots=p[3].value))
    for a, b in zip(plan_before, after):
        assert a.tobytes() == b.tobytes()
    # ... and set_map leaves the stack alone
    c.set_map(synth.random_rect_map(90, 70, 10, 2, 10, 2, 10, seed=8))
    _assert_same(c.sweep_maps_batch(s_src, s_idx), fields, "sweep_maps_batch after set_map")


def test_bookkeeping(vhp):
    occ = _stack(3, 101, 101, seed=61)
    src, idx = _spread_sources(occ, 12, seed=9, used_maps=np.arange(3))
    c = vhp.Context(0)
    c.set_map(occ[0])
    c.set_option("kernel", 3)   # (ignored by the stack's sweep)
    c.sweep_batch(src[:4])
    assert c.last_sweep_kernel() == 3
    c.set_maps(occ)
    c.timing(True)
    c.sweep_maps_batch(src, idx)
    assert c.last_sweep_kernel() == 1
    assert c.last_elapsed_ms() > 0
    ms = c.timing_collect()
    assert len(ms) == 1 and ms[0] > 0
    c.timing(False)
