"""Ray casting for batches of sources on the device (vhp_raycast_[maps_]batch[_device], vhp_line_of_sight[_device]): every field byte
for byte the oracle's raycast_all -- F32 and U8 that expectation cast --, the device forms on torch tensors into NaN / 0xFF-filled
outputs.  Grids, maps and sources: tests/raycast_cases.py (tests/test_raycast_cpu.py holds the same walk to the oracle on the CPU)."""
import ctypes as C

import numpy as np
import pytest

import maps
import raycast_cases as cases

pytestmark = pytest.mark.gpu

NP = {0: np.float64, 1: np.float32, 2: np.uint8}


@pytest.fixture(scope="module")
def vhp():
    import torch  # noqa: F401  (first, so the extension shares torch's HIP runtime)
    import vhp_amd
    return vhp_amd


_memo = {}


def expected(oracle, occ, sources):
    """float64 [n, ny, nx]: the oracle's field per source (computed once per map and source)."""
    out = np.empty((len(sources),) + occ.shape, np.float64)
    for k, (x, y) in enumerate(sources):
        key = (occ.shape, occ.tobytes(), int(x), int(y))
        if key not in _memo:
            _memo[key] = oracle.raycast_all(occ, int(x), int(y))
        out[k] = _memo[key]
    return out


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(~((got == want) | (np.isnan(got.astype(np.float64)) & np.isnan(want.astype(np.float64)))))
        raise AssertionError("%s: %d elements differ, first at %r: %r vs %r" % (what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def untouched(a, dtype):
    return bool(np.all(a == 255)) if dtype == 2 else bool(np.all(np.isnan(a)))


def device_call(vhp, c, sources, shape, dtype, map_index=None, offset=0, n_src=None, sync=True):
    """The device form into a NaN / 0xFF-filled tensor, the fields starting `offset` elements into it: (fields as numpy, the status of
    the call or of vhp_sync).  The elements around the fields must come back as they were."""
    import torch
    tdt = {0: torch.float64, 1: torch.float32, 2: torch.uint8}[dtype]
    src = np.ascontiguousarray(sources, np.int32).reshape(-1, 2)
    n = len(src) if n_src is None else n_src
    cells = shape[0] * shape[1]
    buf = torch.full((n * cells + offset + 16,), 255 if dtype == 2 else float("nan"), dtype=tdt, device="cuda")
    d_src = torch.from_numpy(src).cuda()
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    at = buf.data_ptr() + offset * buf.element_size()
    if map_index is None:
        rc = c.lib.vhp_raycast_batch_device(c.h, C.c_void_p(d_src.data_ptr()), n, dtype, C.c_void_p(at))
    else:
        d_idx = torch.from_numpy(np.ascontiguousarray(map_index, np.int32)).cuda()
        rc = c.lib.vhp_raycast_maps_batch_device(c.h, C.c_void_p(d_src.data_ptr()), C.c_void_p(d_idx.data_ptr()), n, dtype, C.c_void_p(at))
    if rc == vhp.VHP_OK and sync:
        rc = c.lib.vhp_sync(c.h)
    torch.cuda.synchronize()
    c.set_stream(None)
    host = buf.cpu().numpy()
    assert untouched(host[:offset], dtype) and untouched(host[offset + n * cells:], dtype), "stores outside the fields"
    return host[offset: offset + n * cells].reshape((n,) + shape), rc


@pytest.mark.parametrize("nx,ny,seed", cases.GRIDS)
def test_grids_every_dtype_host_and_device(vhp, oracle, nx, ny, seed):
    occ = cases.grid_map(nx, ny, seed)
    sources = cases.sources_for(occ)
    want = expected(oracle, occ, sources)
    if seed is not None:
        for k, (x, y) in enumerate(sources):
            if occ[y, x]:
                assert 0.0 in want[k] and 1.0 in want[k], "source %r would pass on all-ones" % ((x, y),)
        assert not want[-1].any()   # the blocked source: an all-zero field
    c = vhp.Context(0)
    c.set_map(occ)
    for dtype in (vhp.F64, vhp.F32, vhp.U8):
        same(c.raycast_batch(sources, dtype), want.astype(NP[dtype]), "%d x %d host form, dtype %d" % (nx, ny, dtype))
        # (fields that start 3 elements into the buffer: with the odd cell counts, fields on every alignment of their element)
        got, rc = device_call(vhp, c, sources, occ.shape, dtype, offset=3)
        assert rc == vhp.VHP_OK
        same(got, want.astype(NP[dtype]), "%d x %d device form, dtype %d" % (nx, ny, dtype))


def test_blocked_cells_in_plain_sight_stay_one(vhp, oracle):
    occ = np.ones((5, 5), np.uint8)
    occ[4, 4] = occ[0, 2] = 0   # a corner and a border cell, nothing behind either
    c = vhp.Context(0)
    c.set_map(occ)
    want = expected(oracle, occ, [(0, 2), (4, 4)])
    assert want[0].all() and not want[1].any()
    same(c.raycast_batch([(0, 2), (4, 4)]), want, "5 x 5")
    c.set_map(np.zeros((1, 1), np.uint8))
    assert c.raycast_batch([(0, 0)], vhp.U8).tolist() == [[[1]]]


@pytest.mark.parametrize("n_src", [0, 1, 3, 64])
def test_batch_sizes(vhp, oracle, n_src):
    nx, ny, seed = cases.RECT[2]
    occ = cases.rect_map(nx, ny, seed)
    sources = maps.free_sources(occ, 64, 11)[:n_src]
    want = expected(oracle, occ, sources)
    c = vhp.Context(0)
    c.set_map(occ)
    got = c.raycast_batch(sources)
    assert got.shape == (n_src, ny, nx)
    same(got, want, "host form")
    # (n_src = 0 with real pointers: VHP_OK, nothing launched, nothing written)
    got, rc = device_call(vhp, c, sources if n_src else [(0, 0)], occ.shape, vhp.F32, n_src=n_src)
    assert rc == vhp.VHP_OK
    same(got, want.astype(np.float32), "device form")


def test_70000_sources_pass_the_grid_limit(vhp, oracle):
    occ = np.ones((3, 3), np.uint8)
    occ[1, 2] = 0
    nine = [(x, y) for y in range(3) for x in range(3)]
    fields = expected(oracle, occ, nine).astype(np.uint8)
    assert len({f.tobytes() for f in fields}) > 3
    pick = (np.arange(70000) * 7 + np.arange(70000) // 9) % 9
    c = vhp.Context(0)
    c.set_map(occ)
    same(c.raycast_batch(np.array(nine, np.int32)[pick], vhp.U8), fields[pick], "70000 sources")


def test_offsets_past_2_to_the_32(vhp, oracle):
    """540 fields of 8 MB: byte offsets pass 2^31 at field 268 and 2^32 at field 536."""
    import torch
    occ, _ = maps.config_c3(1)
    sources = maps.free_sources(occ, 540, 13)
    c = vhp.Context(0)
    c.set_map(occ)
    out = torch.full((540, 1000, 1000), float("nan"), dtype=torch.float64, device="cuda")
    d_src = torch.from_numpy(sources).cuda()
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    c.raycast_batch_device(d_src.data_ptr(), 540, out.data_ptr())
    c.sync()
    c.set_stream(None)
    for k in (0, 268, 536, 539):
        same(out[k].cpu().numpy(), expected(oracle, occ, sources[k: k + 1])[0], "field %d" % k)


def test_rejected_sources_and_map_indices(vhp, oracle):
    nx, ny, seed = cases.RECT[0]
    occ = cases.rect_map(nx, ny, seed)
    stack = np.stack([occ, cases.rect_map(nx, ny, seed + 1)])
    good = maps.free_sources(occ, 4, 3)
    want = expected(oracle, occ, good)
    c = vhp.Context(0)
    c.set_map(occ)
    c.set_maps(stack)
    for bad in ((nx, 0), (0, ny), (-1, 5), (5, -1)):
        src = np.array([good[0], good[1], bad, good[3]], np.int32)
        out = np.full((4, ny, nx), 7, np.uint8)
        assert c.lib.vhp_raycast_batch(c.h, src.ctypes.data, 4, vhp.U8, out.ctypes.data) == vhp.VHP_ERR_SOURCE_OOB
        same(out[[0, 1, 3]], want[[0, 1, 3]].astype(np.uint8), "the other fields, host form, %r" % (bad,))
        assert not out[2].any()
        got, rc = device_call(vhp, c, src, occ.shape, vhp.F64)
        assert rc == vhp.VHP_ERR_SOURCE_OOB and untouched(got[2], vhp.F64)
        same(got[[0, 1, 3]], want[[0, 1, 3]], "the other fields, device form, %r" % (bad,))
        assert c.lib.vhp_sync(c.h) == vhp.VHP_OK   # (reported once)
    for bad in (-1, 2):
        idx = np.array([0, bad, 0, 0], np.int32)
        out = np.full((4, ny, nx), 7.0, np.float32)
        assert c.lib.vhp_raycast_maps_batch(c.h, good.ctypes.data, idx.ctypes.data, 4, vhp.F32, out.ctypes.data) == vhp.VHP_ERR_SOURCE_OOB
        same(out[[0, 2, 3]], want[[0, 2, 3]].astype(np.float32), "the other fields, maps host form, index %d" % bad)
        assert not out[1].any()
        got, rc = device_call(vhp, c, good, occ.shape, vhp.U8, map_index=idx)
        assert rc == vhp.VHP_ERR_SOURCE_OOB and untouched(got[1], vhp.U8)
        same(got[[0, 2, 3]], want[[0, 2, 3]].astype(np.uint8), "the other fields, maps device form, index %d" % bad)


def test_argument_errors(vhp):
    import torch
    occ = cases.rect_map(*cases.RECT[0])
    ny, nx = occ.shape
    src = np.array([[1, 1]], np.int32)
    idx = np.zeros(1, np.int32)
    out = np.zeros((ny, nx), np.float64)
    hit = np.zeros(2, np.int32)
    pair = np.array([1, 1, 2, 2], np.int32)
    c = vhp.Context(0)
    # no map, no stack
    assert c.lib.vhp_raycast_batch(c.h, src.ctypes.data, 1, vhp.F64, out.ctypes.data) == vhp.VHP_ERR_NO_MAP
    assert c.lib.vhp_raycast_batch_device(c.h, src.ctypes.data, 1, vhp.F64, out.ctypes.data) == vhp.VHP_ERR_NO_MAP
    assert c.lib.vhp_line_of_sight(c.h, pair.ctypes.data, 1, hit.ctypes.data) == vhp.VHP_ERR_NO_MAP
    assert c.lib.vhp_line_of_sight_device(c.h, pair.ctypes.data, 1, hit.ctypes.data) == vhp.VHP_ERR_NO_MAP
    c.set_map(occ)
    assert c.lib.vhp_raycast_maps_batch(c.h, src.ctypes.data, idx.ctypes.data, 1, vhp.F64, out.ctypes.data) == vhp.VHP_ERR_NO_MAP
    assert c.lib.vhp_raycast_maps_batch_device(c.h, src.ctypes.data, idx.ctypes.data, 1, vhp.F64, out.ctypes.data) == vhp.VHP_ERR_NO_MAP
    c.set_maps(occ[None])
    # dtypes: 3 is none of the ray casts', and 2 stays none of the sweeps'
    d_src = torch.from_numpy(src).cuda()
    d_idx = torch.from_numpy(idx).cuda()
    d_out = torch.zeros((ny, nx), dtype=torch.float64, device="cuda")
    for dtype in (3, -1):
        assert c.lib.vhp_raycast_batch(c.h, src.ctypes.data, 1, dtype, out.ctypes.data) == vhp.VHP_ERR_ARG
        assert c.lib.vhp_raycast_maps_batch(c.h, src.ctypes.data, idx.ctypes.data, 1, dtype, out.ctypes.data) == vhp.VHP_ERR_ARG
        assert c.lib.vhp_raycast_batch_device(c.h, C.c_void_p(d_src.data_ptr()), 1, dtype, C.c_void_p(d_out.data_ptr())) == vhp.VHP_ERR_ARG
        assert c.lib.vhp_raycast_maps_batch_device(c.h, C.c_void_p(d_src.data_ptr()), C.c_void_p(d_idx.data_ptr()), 1, dtype,
                                                   C.c_void_p(d_out.data_ptr())) == vhp.VHP_ERR_ARG
    assert c.lib.vhp_sweep_batch_device(c.h, C.c_void_p(d_src.data_ptr()), 1, vhp.SWEEP_FULL, vhp.U8, C.c_void_p(d_out.data_ptr())) == vhp.VHP_ERR_ARG
    assert c.lib.vhp_sweep_batch(c.h, src.ctypes.data, 1, vhp.SWEEP_FULL, vhp.U8, out.ctypes.data) == vhp.VHP_ERR_ARG
    assert c.lib.vhp_sweep_maps_batch(c.h, src.ctypes.data, idx.ctypes.data, 1, vhp.U8, out.ctypes.data) == vhp.VHP_ERR_ARG
    # null pointers, a negative count, a misaligned output
    assert c.lib.vhp_raycast_batch(c.h, None, 1, vhp.F64, out.ctypes.data) == vhp.VHP_ERR_ARG
    assert c.lib.vhp_raycast_batch(c.h, src.ctypes.data, -1, vhp.F64, out.ctypes.data) == vhp.VHP_ERR_ARG
    assert c.lib.vhp_raycast_maps_batch(c.h, src.ctypes.data, None, 1, vhp.F64, out.ctypes.data) == vhp.VHP_ERR_ARG
    assert c.lib.vhp_raycast_batch_device(c.h, C.c_void_p(d_src.data_ptr()), 1, vhp.F64, C.c_void_p(d_out.data_ptr() + 4)) == vhp.VHP_ERR_ARG
    assert c.lib.vhp_line_of_sight(c.h, None, 1, hit.ctypes.data) == vhp.VHP_ERR_ARG
    assert c.lib.vhp_line_of_sight(c.h, pair.ctypes.data, -1, hit.ctypes.data) == vhp.VHP_ERR_ARG
    assert c.lib.vhp_line_of_sight(c.h, pair.ctypes.data, 0, hit.ctypes.data) == vhp.VHP_OK
    assert c.lib.vhp_sync(c.h) == vhp.VHP_OK


def test_stack_of_maps(vhp, oracle):
    nx, ny, _ = cases.RECT[2]
    stack = np.stack([cases.rect_map(nx, ny, 20 + k) for k in range(4)])
    assert len({m.tobytes() for m in stack}) == 4
    on = np.array([(5 * k + 3) % 4 for k in range(12)], np.int32)
    per_map = [maps.free_sources(m, 12, 40 + k) for k, m in enumerate(stack)]
    sources = np.array([per_map[m][k] for k, m in enumerate(on)], np.int32)
    want = np.stack([expected(oracle, stack[m], sources[k: k + 1])[0] for k, m in enumerate(on)])
    c = vhp.Context(0)
    c.set_maps(stack)
    for dtype in (vhp.F64, vhp.U8):
        same(c.raycast_maps_batch(sources, on, dtype), want.astype(NP[dtype]), "maps host form, dtype %d" % dtype)
        got, rc = device_call(vhp, c, sources, (ny, nx), dtype, map_index=on)
        assert rc == vhp.VHP_OK
        same(got, want.astype(NP[dtype]), "maps device form, dtype %d" % dtype)
    single = vhp.Context(0)
    for m in range(4):
        single.set_map(stack[m])
        same(single.raycast_batch(sources[on == m]), want[on == m], "the single-map batch on map %d" % m)


def test_the_one_source_entry_point_is_unchanged(vhp, oracle):
    nx, ny, seed = cases.RECT[3]
    occ = cases.rect_map(nx, ny, seed)
    sources = cases.sources_for(occ)
    want = expected(oracle, occ, sources)
    c = vhp.Context(0)
    c.set_map(occ)
    batch = c.raycast_batch(sources)
    for k, (x, y) in enumerate(sources):
        one = c.raycast_all(x, y)
        same(one, want[k], "raycast_all from %r" % ((x, y),))
        same(one, batch[k], "raycast_all against the batch from %r" % ((x, y),))


def test_line_of_sight(vhp, oracle):
    import torch
    nx, ny, seed = cases.RECT[3]
    occ = cases.rect_map(nx, ny, seed)
    sources = [cases.sources_for(occ)[k] for k in (0, 8, 9)]   # a corner, the centre, the cell beside an obstacle
    c = vhp.Context(0)
    c.set_map(occ)
    fields = c.raycast_batch(sources)
    yy, xx = np.mgrid[0:ny, 0:nx]
    for k, (sx, sy) in enumerate(sources):
        pairs = np.stack([np.full(nx * ny, sx), np.full(nx * ny, sy), xx.ravel(), yy.ravel()], axis=1).astype(np.int32)
        want = cases.hits_from(occ, sx, sy)
        got = c.line_of_sight(pairs).reshape(ny, nx, 2)
        same(got, want, "hits from %r" % ((sx, sy),))
        assert (got[..., 0] >= 0).any() and (got[..., 0] == -1).any()
        assert got[sy, sx].tolist() == [-1, -1] or not occ[sy, sx]
        # the union relation gives the batch's field, and the oracle's
        same(cases.field_from_hits(got), fields[k], "union of the hits from %r" % ((sx, sy),))
        same(fields[k], expected(oracle, occ, [(sx, sy)])[0], "field from %r" % ((sx, sy),))
        # the device form into a filled tensor
        d_pairs = torch.from_numpy(pairs).cuda()
        d_hit = torch.full((nx * ny, 2), -9, dtype=torch.int32, device="cuda")
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        c.line_of_sight_device(d_pairs.data_ptr(), len(pairs), d_hit.data_ptr())
        c.sync()
        c.set_stream(None)
        same(d_hit.cpu().numpy().reshape(ny, nx, 2), want, "device form from %r" % ((sx, sy),))
    # equal ends are clear, on a free cell; the start is tested, so not on a blocked one with another target
    by, bx = (int(v) for v in np.argwhere(occ == 0)[0])
    fx, fy = sources[1]
    assert c.line_of_sight([(fx, fy, fx, fy), (bx, by, bx, by), (bx, by, fx, fy)]).tolist() == [[-1, -1], [-1, -1], [bx, by]]
    # an end outside the grid: (-2, -2), the status, the other pairs answered
    pairs = np.array([(fx, fy, fx, fy), (nx, 0, 1, 1), (1, 1, 0, ny), (-1, 0, 0, 0), (bx, by, fx, fy)], np.int32)
    hit = np.zeros((5, 2), np.int32)
    assert c.lib.vhp_line_of_sight(c.h, pairs.ctypes.data, 5, hit.ctypes.data) == vhp.VHP_ERR_SOURCE_OOB
    assert hit.tolist() == [[-1, -1], [-2, -2], [-2, -2], [-2, -2], [bx, by]]
    assert c.lib.vhp_sync(c.h) == vhp.VHP_OK


def test_one_context_reused(vhp, oracle):
    """A large call, a small one, a large one, the map changed in between: what fresh contexts give, and the oracle."""
    a = cases.rect_map(*cases.RECT[3])
    b = cases.tiny_map(7, 1)
    d = cases.rect_map(65, 63, 9)
    stack = np.stack([d, cases.rect_map(65, 63, 10)])
    steps = [(a, maps.free_sources(a, 64, 5), vhp.F64), (b, np.array([(0, 0)], np.int32), vhp.U8), (d, maps.free_sources(d, 48, 6), vhp.F32),
             (b, np.array([(6, 0), (1, 0)], np.int32), vhp.F64), (a, maps.free_sources(a, 9, 8), vhp.U8)]
    c = vhp.Context(0)
    for stage, (occ, sources, dtype) in enumerate(steps):
        ny, nx = occ.shape
        c.set_map(occ)
        fresh = vhp.Context(0)
        fresh.set_map(occ)
        want = expected(oracle, occ, sources).astype(NP[dtype])
        same(c.raycast_batch(sources, dtype), want, "stage %d, host form" % stage)
        same(fresh.raycast_batch(sources, dtype), want, "stage %d, fresh context" % stage)
        got, rc = device_call(vhp, c, sources, occ.shape, dtype)
        assert rc == vhp.VHP_OK
        same(got, want, "stage %d, device form" % stage)
        pairs = np.array([(x, y, nx - 1 - x, ny - 1 - y) for x, y in sources[: 1 + 40 * ((stage + 1) % 2)]], np.int32)
        same(c.line_of_sight(pairs), fresh.line_of_sight(pairs), "stage %d, line of sight" % stage)
        if stage == 2:
            c.set_maps(stack)
            fresh.set_maps(stack)
            on = np.arange(len(sources), dtype=np.int32) % 2
            same(c.raycast_maps_batch(sources, on, dtype), fresh.raycast_maps_batch(sources, on, dtype), "stage 2, maps batch")
        assert c.last_elapsed_ms() > 0.0
