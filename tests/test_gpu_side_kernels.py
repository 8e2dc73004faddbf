"""The entry points beside the tuned sweeps and the planner, on the GPU, past the sizes at which their loops first repeat -- byte for
byte against the oracle or numpy (inputs: side_kernel_shapes.py; that they are past those sizes: test_side_kernel_shapes.py).

  A  vhp_sweep_batch / vhp_sweep_maps_batch with more than 1 GiB of fields: the second slice of stage_slices;
  B  the queue variant: a second slice of its own launch loop, fp32, and the device entry point (NaN-filled buffer, field_stride,
     a source outside the grid);
  C  the union kernel over more cells than one pass of its capped grid, fields and partials, and fields a stride apart;
  D  vhp_variant_sweep / vhp_offset_sweep with fronts longer than the workgroup, dynamic LDS either side of 64 KB and at the side
     limit of 4096, the refusal above it, the argument checks;
  E  vhp_planner_solve_variant: every status, ties of its pick across lanes, wavefronts and the final scan, a side above 1024.

Device outputs start as NaN (-7 for int32), so a cell nobody wrote fails."""
import numpy as np
import pytest

import side_kernel_shapes as shapes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vhp():
    import torch  # noqa: F401  (first, so the extension shares torch's HIP runtime)
    import vhp_amd
    return vhp_amd


def _types(vhp, dtype):
    import torch
    return (vhp.F64, torch.float64, np.float64) if dtype == "f64" else (vhp.F32, torch.float32, np.float32)


def _context(vhp, occ):
    import torch
    c = vhp.Context(0)
    c.set_map(np.array(occ))
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


def _assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, "%s: %s %r, want %s %r" % (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() != want.tobytes():
        differ = got != want
        if not differ.any():  # (NaN in both, or zeros of either sign)
            differ = got.view(np.uint8).reshape(got.shape + (-1,)) != want.view(np.uint8).reshape(want.shape + (-1,))
            differ = differ.any(axis=-1)
        first = tuple(int(v) for v in np.argwhere(differ)[0])
        raise AssertionError("%s: %d cells differ, first at [y, x] = %r: got %r want %r" % (what, int(differ.sum()), first, got[first], want[first]))


def _raises(vhp, code, call, *args, **kw):
    with pytest.raises(vhp.VhpError) as e:
        call(*args, **kw)
    assert e.value.code == code, "status %d, want %d" % (e.value.code, code)


# ---- A. host staging past one slice ---------------------------------------------------------------------------------------------

def test_sweep_batch_stages_a_second_slice(vhp, oracle):
    occ, src = shapes.stage_batch()
    want = shapes.stage_oracle_fields(oracle)
    # csrc/vhp_capi.hip stage_slices: slices of (1 << 30) / field sources
    assert len(src) * shapes.STAGE_FIELD_BYTES > 2**30 and len(src) > shapes.STAGE_SLICE
    c = vhp.Context(0)
    c.set_map(np.array(occ))
    got = c.sweep_batch(src)
    kernel = c.last_sweep_kernel()
    assert got.nbytes == len(src) * shapes.STAGE_FIELD_BYTES
    for k, (x, y) in enumerate(src):
        _assert_same(got[k], want[(int(x), int(y))], "source %d (%d,%d) of %d, kernel %d of the last slice" % (k, x, y, len(src), kernel))
    del got


def test_sweep_maps_batch_stages_a_second_slice(vhp, oracle):
    occ, src, idx = shapes.stage_maps_batch()
    want = shapes.stage_maps_oracle_fields(oracle)
    assert len(src) * shapes.STAGE_FIELD_BYTES > 2**30 and len(src) > shapes.STAGE_SLICE
    c = vhp.Context(0)
    c.set_maps(np.array(occ))
    got = c.sweep_maps_batch(src, idx)
    kernel = c.last_sweep_kernel()
    for k, ((x, y), m) in enumerate(zip(src, idx)):
        _assert_same(got[k], want[(int(m), int(x), int(y))], "source %d (%d,%d) on map %d, kernel %d of the last slice" % (k, x, y, m, kernel))
    del got


# ---- B. the queue variant -------------------------------------------------------------------------------------------------------

def test_queue_variant_launches_a_second_slice(vhp, oracle):
    occ, src = shapes.queue_batch()
    want = shapes.queue_oracle_fields(oracle)
    # csrc/vhp_queue.hip.h launch_queue_sweep_impl: (1 << 30) / (cells * 33 + 64) sources per launch
    assert len(src) > 2**30 // (33 * occ.size + 64)
    c = vhp.Context(0)
    c.set_map(np.array(occ))
    got = c.sweep_batch(src, variant=vhp.SWEEP_QUEUE)
    for k, (x, y) in enumerate(src):
        _assert_same(got[k], want[(int(x), int(y))], "queue variant, source %d (%d,%d) of %d" % (k, x, y, len(src)))
    del got


def test_queue_variant_fp32(vhp, oracle):
    occ, src = shapes.queue_small()
    want = shapes.queue_small_oracle_fields(oracle)
    c = vhp.Context(0)
    c.set_map(np.array(occ))
    got = c.sweep_batch(src, variant=vhp.SWEEP_QUEUE, dtype=vhp.F32)
    for k, (x, y) in enumerate(src):
        _assert_same(got[k], want[(int(x), int(y))].astype(np.float32), "queue variant fp32, source %d (%d,%d)" % (k, x, y))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_queue_variant_device_entry_point(vhp, oracle, dtype):
    import torch
    occ, src = shapes.queue_small()
    want = shapes.queue_small_oracle_fields(oracle)
    vdt, tdt, ndt = _types(vhp, dtype)
    n, cells = len(src), occ.size
    c = _context(vhp, occ)
    d_src = torch.from_numpy(np.array(src)).cuda()

    def launch(d_sources):
        d_out = torch.full((n,) + occ.shape, float("nan"), dtype=tdt, device="cuda")
        c.sweep_batch_device(d_sources.data_ptr(), n, d_out.data_ptr(), variant=vhp.SWEEP_QUEUE, dtype=vdt)
        return d_out

    packed = launch(d_src)
    c.sync()
    packed = packed.cpu().numpy()
    for k, (x, y) in enumerate(src):
        _assert_same(packed[k], want[(int(x), int(y))].astype(ndt), "queue variant on a caller's buffer, %s, source %d (%d,%d)" % (dtype, k, x, y))

    c.set_option("field_stride", cells)   # the packed stride by its own name: accepted
    same = launch(d_src)
    c.sync()
    assert same.cpu().numpy().tobytes() == packed.tobytes()

    c.set_option("field_stride", cells + 5)   # the queue variant writes packed fields only
    d_out = torch.full((n * (cells + 5),), float("nan"), dtype=tdt, device="cuda")
    _raises(vhp, vhp.VHP_ERR_ARG, c.sweep_batch_device, d_src.data_ptr(), n, d_out.data_ptr(), variant=vhp.SWEEP_QUEUE, dtype=vdt)
    c.sync()
    assert bool(torch.isnan(d_out).all()), "a refused launch wrote into the caller's buffer"
    c.set_option("field_stride", 0)

    outside = np.array(src)
    outside[4] = (occ.shape[1], 3)   # one past the right edge
    got = launch(torch.from_numpy(outside).cuda())
    _raises(vhp, vhp.VHP_ERR_SOURCE_OOB, c.sync)
    c.sync()   # reported once
    got = got.cpu().numpy()
    for k, (x, y) in enumerate(src):
        w = np.zeros(occ.shape, ndt) if k == 4 else want[(int(x), int(y))].astype(ndt)
        _assert_same(got[k], w, "queue variant, source 4 outside the grid, %s, source %d" % (dtype, k))


# ---- C. the union past one pass of its grid, and field_stride -------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("grid", list(shapes.UNION_GRIDS))
def test_union_past_one_pass_of_its_grid(vhp, grid, dtype):
    import torch
    nx, ny = shapes.UNION_GRIDS[grid]
    vdt, tdt, ndt = _types(vhp, dtype)
    # csrc/vhp_union.hip.h launch_union: 16 workgroups of 256 threads per CU at the most, two cells a thread
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert nx * ny > 2 * shapes.UNION_CELLS_PER_CU_AND_PASS * n_cus, "%d CUs: %d cells are one pass" % (n_cus, nx * ny)
    f = shapes.union_fields(grid, ndt)
    wb, wa = shapes.union_want(grid, ndt)
    n = len(f)
    c = _context(vhp, np.ones((ny, nx), np.uint8))
    d = torch.from_numpy(np.array(f)).cuda()
    best = torch.full((ny, nx), float("nan"), dtype=tdt, device="cuda")
    arg = torch.full((ny, nx), -7, dtype=torch.int32, device="cuda")
    c.union_fields_device(d.data_ptr(), n, best.data_ptr(), arg.data_ptr(), first_index=shapes.UNION_FIRST_INDEX, dtype=vdt)
    torch.cuda.synchronize()
    _assert_same(best.cpu().numpy(), wb, "union of %d fields %s, %s: best" % (n, grid, dtype))
    _assert_same(arg.cpu().numpy(), wa, "union of %d fields %s, %s: arg" % (n, grid, dtype))
    # the same through partials in scrambled slots (tests/test_union.py), from fields that start off the 16-byte grid
    pb = torch.full((3, ny, nx), float("nan"), dtype=tdt, device="cuda")
    pa = torch.full((3, ny, nx), -7, dtype=torch.int32, device="cuda")
    raw = torch.empty(f.size + 1, dtype=tdt, device="cuda")
    off = raw[1:].view(f.shape)
    off.copy_(d)
    del d
    for slot, (lo, hi) in zip(shapes.UNION_SLOTS, shapes.UNION_CUTS):
        c.union_fields_device(off[lo:].data_ptr(), hi - lo, pb[slot].data_ptr(), pa[slot].data_ptr(), first_index=shapes.UNION_FIRST_INDEX + lo, dtype=vdt)
    best.fill_(float("nan"))
    arg.fill_(-7)
    c.union_partials_device(pb.data_ptr(), pa.data_ptr(), 3, best.data_ptr(), arg.data_ptr(), dtype=vdt)
    torch.cuda.synchronize()
    _assert_same(best.cpu().numpy(), wb, "union of 3 partials %s, %s: best" % (grid, dtype))
    _assert_same(arg.cpu().numpy(), wa, "union of 3 partials %s, %s: arg" % (grid, dtype))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_union_of_fields_a_stride_apart(vhp, dtype):
    import torch
    nx, ny = shapes.STRIDE_GRID
    cells = nx * ny
    vdt, tdt, ndt = _types(vhp, dtype)
    f = shapes.stride_fields(ndt)
    n = len(f)
    wb, wa = shapes._numpy_union(f, 3)
    c = _context(vhp, np.ones((ny, nx), np.uint8))
    best = torch.empty((ny, nx), dtype=tdt, device="cuda")
    arg = torch.empty((ny, nx), dtype=torch.int32, device="cuda")

    def union(d_fields):
        best.fill_(float("nan"))
        arg.fill_(-7)
        c.union_fields_device(d_fields.data_ptr(), n, best.data_ptr(), arg.data_ptr(), first_index=3, dtype=vdt)
        torch.cuda.synchronize()
        return best.cpu().numpy(), arg.cpu().numpy()

    for path, pad in shapes.STRIDE_PADS.items():
        assert ((cells + pad) % 2 == 0) == (path == "pairs")
        d = torch.from_numpy(shapes.padded(f, pad)).cuda()   # (+inf in the padding: a pad read as a cell wins its cell)
        c.set_option("field_stride", cells + pad)
        gb, ga = union(d)
        _assert_same(gb, wb, "fields %d apart (%s), %s: best" % (cells + pad, path, dtype))
        _assert_same(ga, wa, "fields %d apart (%s), %s: arg" % (cells + pad, path, dtype))
    c.set_option("field_stride", cells - 1)
    _raises(vhp, vhp.VHP_ERR_ARG, c.union_fields_device, d.data_ptr(), n, best.data_ptr(), arg.data_ptr(), first_index=3, dtype=vdt)
    # vhp_set_map takes the stride back to 0: packed fields again (in a buffer with room for a stride that stayed)
    c.set_option("field_stride", cells + 6)
    c.set_map(np.ones((ny, nx), np.uint8))
    assert c.field_stride == 0
    room = np.full(n * (cells + 6), np.inf, ndt)
    room[: n * cells] = f.reshape(-1)
    gb, ga = union(torch.from_numpy(room).cuda())
    _assert_same(gb, wb, "packed fields after set_map, %s: best" % dtype)
    _assert_same(ga, wa, "packed fields after set_map, %s: arg" % dtype)


# ---- D. the variant and offset sweeps above 1024 --------------------------------------------------------------------------------

def _lds_check(nx, ny):
    lds = shapes.variant_lds_bytes(nx, ny)
    if max(nx, ny) == 2729:
        assert lds <= shapes.LDS_DEFAULT_LIMIT < lds + 24
    if max(nx, ny) == 2730:
        assert lds - 24 <= shapes.LDS_DEFAULT_LIMIT < lds
    if max(nx, ny) == shapes.VARIANT_MAX_SIDE:
        assert lds == 98328
    assert min(nx, ny) > shapes.VARIANT_THREADS   # a corner source's longest fronts take a second pass of the workgroup


@pytest.mark.parametrize("alpha,fac", shapes.VARIANT_PARAMS)
@pytest.mark.parametrize("nx,ny", shapes.VARIANT_GRIDS)
def test_variant_sweep_above_1024(vhp, oracle, nx, ny, alpha, fac):
    _lds_check(nx, ny)
    occ, src = shapes.variant_case(nx, ny)
    c = vhp.Context(0)
    c.set_map(np.array(occ))
    got = c.sweep_batch_variant(src, alpha, fac)
    for k, (x, y) in enumerate(src):
        want = oracle.sweep_matlab(np.array(occ), int(x), int(y), alpha, fac)
        _assert_same(got[k], want, "variant sweep %dx%d alpha %g fac %g, source (%d,%d)" % (nx, ny, alpha, fac, x, y))


@pytest.mark.parametrize("offset", shapes.OFFSETS)
@pytest.mark.parametrize("nx,ny", shapes.VARIANT_GRIDS)
def test_offset_sweep_above_1024(vhp, oracle, nx, ny, offset):
    _lds_check(nx, ny)
    occ, src = shapes.variant_case(nx, ny)
    c = vhp.Context(0)
    c.set_map(np.array(occ))
    got = c.sweep_batch_offset(src, offset)
    for k, (x, y) in enumerate(src):
        want = oracle.sweep_full_offset(np.array(occ), int(x), int(y), offset)
        _assert_same(got[k], want, "offset sweep %dx%d offset %g, source (%d,%d)" % (nx, ny, offset, x, y))
        if offset == 0.0:   # include/vhp.h: offset 0 is computeVisibility() as the tuned kernels compute it
            _assert_same(got[k], oracle.sweep_full(np.array(occ), int(x), int(y)), "offset 0 against the plain sweep, %dx%d source (%d,%d)" % (nx, ny, x, y))


def test_variant_entry_points_refuse_a_side_above_4096(vhp, oracle):
    for occ in shapes.too_large_maps():
        ny, nx = occ.shape
        assert max(nx, ny) > shapes.VARIANT_MAX_SIDE
        src = np.array([(nx // 2, ny // 2)], np.int32)
        c = vhp.Context(0)
        c.set_map(np.array(occ))
        _raises(vhp, vhp.VHP_ERR_TOO_LARGE, c.sweep_batch_variant, src, 1.0, 1.0)
        _raises(vhp, vhp.VHP_ERR_TOO_LARGE, c.sweep_batch_offset, src, 0.0)
        _raises(vhp, vhp.VHP_ERR_TOO_LARGE, c.planner_solve_variant, (nx // 2, ny // 2), (0, 0), 0.5, 1.0, 5)
        got = c.sweep_batch(src)   # the context sweeps on
        _assert_same(got[0], oracle.sweep_full(np.array(occ), nx // 2, ny // 2), "sweep_batch on %dx%d after the refusals" % (nx, ny))


def test_variant_entry_points_check_their_arguments(vhp):
    occ, src = shapes.queue_small()
    ny, nx = occ.shape
    c = vhp.Context(0)
    c.set_map(np.array(occ))
    for fac in (0.0, -1.0, float("nan")):
        _raises(vhp, vhp.VHP_ERR_ARG, c.sweep_batch_variant, src, 1.0, fac)
    for offset in (-1.0, float("nan")):
        _raises(vhp, vhp.VHP_ERR_ARG, c.sweep_batch_offset, src, offset)
    none = np.zeros((0, 2), np.int32)
    assert c.sweep_batch_variant(none, 1.0, 1.0).shape == (0, ny, nx)
    assert c.sweep_batch_offset(none, 1.0).shape == (0, ny, nx)
    for bad in ((nx, 3), (-1, 3), (3, ny), (3, -1)):
        batch = np.array([src[0], bad], np.int32)
        _raises(vhp, vhp.VHP_ERR_SOURCE_OOB, c.sweep_batch_variant, batch, 1.0, 1.0)
        _raises(vhp, vhp.VHP_ERR_SOURCE_OOB, c.sweep_batch_offset, batch, 1.0)


# ---- E. the variant planner -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", shapes.PLANNER_NAMES)
def test_variant_planner(vhp, oracle, name):
    occ, start, end, thr, alpha, max_iter = shapes.planner_cases()[name]
    want = shapes.planner_want(oracle, name)
    c = vhp.Context(0)
    c.set_map(np.array(occ))
    got = c.planner_solve_variant(start, end, thr, alpha, max_iter)
    assert got["status"] == want["status"], "%s: status %d, want %d" % (name, got["status"], want["status"])
    assert got["waypoints"].tolist() == want["waypoints"].tolist(), name
    for key in ("label", "map_builder", "local"):   # (after VHP_ERR_NOTHING_LIT and VHP_ERR_MAX_ITER too)
        _assert_same(got[key], want[key], "%s: %s" % (name, key))


def test_variant_planner_refuses_points_outside_the_grid(vhp):
    occ = shapes.planner_cases()["max_iter 0"][0]
    ny, nx = occ.shape
    c = vhp.Context(0)
    c.set_map(np.array(occ))
    for bad in ((nx, 5), (-1, 5), (5, ny), (5, -1)):
        assert c.planner_solve_variant(bad, (5, 5), 0.5, 1.0, 5)["status"] == vhp.VHP_ERR_START_OOB, bad
        assert c.planner_solve_variant((5, 5), bad, 0.5, 1.0, 5)["status"] == vhp.VHP_ERR_END_OOB, bad
