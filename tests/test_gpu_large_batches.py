"""Batches past one pass of the sweeps' launch-order pre-kernels, on the GPU, bit for bit against the oracle (large_batch_shapes.py).

  * the pool sweep's vhp_pool_order at the last size of its LDS body (1024 sources, order_units_lds with eight units a thread), at
    the first of its global-memory body (1025, order_units: blocks[] staged through line_base, order[], scans with more than 8
    entries a thread), and with three sources outside the map among 1031 (records with -1); each launched twice on one context and
    scratch (the epoch and the queue word start over), in both dtypes, on a width that is a multiple of 8 and on one that is not;
    and the static round off, on and snaking on the global body;
  * the front sweep's vhp_order_units with 257 and 1025 sources (four units a source: two and five passes of its 1024 threads),
    also packing short quadrants, and over a stack of maps with 1025 sources;
  * the latency sweep at its last batch size, 256 sources, and the fall-back one above.

Every launch is the device form into fields prefilled with NaN: an accepted field has none left, a rejected one nothing else."""
import numpy as np
import pytest

import large_batch_shapes as shapes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vhp():
    import torch  # noqa: F401  (first, so the extension shares torch's HIP runtime)
    import vhp_amd
    return vhp_amd


def _types(vhp, dtype):
    import torch
    return (vhp.F64, torch.float64, np.float64) if dtype == "f64" else (vhp.F32, torch.float32, np.float32)


def _context(vhp, occ, **options):
    import torch
    c = vhp.Context(0)
    c.set_map(np.array(occ))
    for key, v in options.items():
        c.set_option(key, v)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


def _launch(vhp, c, d_src, n, occ, dtype, rejects=False):
    """One device-form sweep into NaN-filled fields; returns them on the host."""
    import torch
    vdt, tdt, _ = _types(vhp, dtype)
    d_out = torch.full((n,) + occ.shape, float("nan"), dtype=tdt, device="cuda")
    c.sweep_batch_device(d_src.data_ptr(), n, d_out.data_ptr(), dtype=vdt)
    if rejects:  # the launch runs, and the sync behind it names the bad source
        with pytest.raises(vhp.VhpError) as e:
            c.sync()
        assert e.value.code == vhp.VHP_ERR_SOURCE_OOB
    else:
        c.sync()
    return d_out.cpu().numpy()


def _assert_fields(got, src, outside, want_of, ndt, what):
    """Field k equals want_of(k) cast to ndt bit for bit and holds no NaN; the fields of `outside` are all NaN still."""
    assert got.dtype == ndt and len(got) == len(src)
    for k in range(len(src)):
        if k in outside:
            assert np.isnan(got[k]).all(), "%s: the field of source %d (rejected) was written" % (what, k)
            continue
        assert not np.isnan(got[k]).any(), "%s: source %d (%d,%d): cells left unwritten" % (what, k, src[k][0], src[k][1])
        w = want_of(k).astype(ndt)
        if got[k].tobytes() != w.tobytes():
            bad = np.argwhere(got[k] != w)
            y, x = bad[0]
            raise AssertionError("%s, source %d (%d,%d): %d cells differ, first at (x=%d,y=%d): got %r want %r" % (
                what, k, src[k][0], src[k][1], len(bad), x, y, got[k][y, x], w[y, x]))


def _single_map_want(oracle, grid, src):
    want = shapes.oracle_fields(oracle, grid)
    return lambda k: want[(int(src[k][0]), int(src[k][1]))]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("grid", list(shapes.GRIDS))
@pytest.mark.parametrize("name", list(shapes.POOL))
def test_pool_sweep_either_side_of_1024_sources(vhp, oracle, name, grid, dtype):
    import torch
    n, with_outside = shapes.POOL[name]
    occ, src, outside = shapes.batch(grid, n, with_outside)
    assert shapes.ORDER_BODY[name] == ("order_units_lds" if n <= 1024 else "order_units")
    c = _context(vhp, occ, kernel=3)
    d_src = torch.from_numpy(np.array(src)).cuda()
    first = _launch(vhp, c, d_src, n, occ, dtype, rejects=bool(outside))
    assert c.last_sweep_kernel() == 3
    _assert_fields(first, src, outside, _single_map_want(oracle, grid, src), _types(vhp, dtype)[2], "%s %s %s" % (name, grid, dtype))
    again = _launch(vhp, c, d_src, n, occ, dtype, rejects=bool(outside))
    assert c.last_sweep_kernel() == 3
    assert again.tobytes() == first.tobytes(), "%s %s %s: a second launch on the same scratch differs" % (name, grid, dtype)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_pool_sweep_static_round_off_and_snaking_on_the_global_path(vhp, oracle, dtype):
    import torch
    occ, src, _ = shapes.batch("w8", 1025)
    c = _context(vhp, occ, kernel=3)
    d_src = torch.from_numpy(np.array(src)).cuda()
    default = _launch(vhp, c, d_src, len(src), occ, dtype)
    _assert_fields(default, src, (), _single_map_want(oracle, "w8", src), _types(vhp, dtype)[2], "1025 sources, default, %s" % dtype)
    for mode in (0, 2):
        c.set_option("pool_static_round", mode)
        got = _launch(vhp, c, d_src, len(src), occ, dtype)
        assert c.last_sweep_kernel() == 3
        assert got.tobytes() == default.tobytes(), "pool_static_round = %d, %s: not the default's bytes" % (mode, dtype)


# (pack: short quadrants share a workgroup, which the one-round shape of 8 strips offers -- the shape test_gpu_sweep_maps.py packs)
FRONT = [(257, {}), (1025, {}), (1025, dict(pack=1, strips=8, rows_per_lane=1))]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n,options", FRONT, ids=lambda v: ("packed" if v else "plain") if isinstance(v, dict) else str(v))
def test_front_sweep_past_one_pass_of_its_order_kernel(vhp, oracle, n, options, dtype):
    import torch
    occ, src, _ = shapes.batch("w8", n)
    c = _context(vhp, occ, kernel=1, **options)
    d_src = torch.from_numpy(np.array(src)).cuda()
    got = _launch(vhp, c, d_src, n, occ, dtype)
    assert c.last_sweep_kernel() == 1
    _assert_fields(got, src, (), _single_map_want(oracle, "w8", src), _types(vhp, dtype)[2], "front sweep, %d sources %r %s" % (n, options, dtype))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_stack_of_maps_with_1025_sources(vhp, oracle, dtype):
    import torch
    occ, src, idx = shapes.maps_batch()
    want = shapes.maps_oracle_fields(oracle)
    n = len(src)
    vdt, tdt, ndt = _types(vhp, dtype)
    c = vhp.Context(0)
    c.set_maps(np.array(occ))
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    d_src = torch.from_numpy(np.array(src)).cuda()
    # every source on its own map; then two map indices outside the stack, one either side of the pre-kernel's first pass
    bad_idx = np.array(idx)
    bad_idx[9], bad_idx[1024] = -1, occ.shape[0]
    for indices, rejected in ((np.array(idx), ()), (bad_idx, (9, 1024))):
        d_idx = torch.from_numpy(indices).cuda()
        d_out = torch.full((n,) + occ.shape[1:], float("nan"), dtype=tdt, device="cuda")
        c.sweep_maps_batch_device(d_src.data_ptr(), d_idx.data_ptr(), n, d_out.data_ptr(), dtype=vdt)
        assert c.lib.vhp_sync(c.h) == (vhp.VHP_ERR_SOURCE_OOB if rejected else vhp.VHP_OK)
        assert c.lib.vhp_sync(c.h) == vhp.VHP_OK
        assert c.last_sweep_kernel() == 1
        _assert_fields(d_out.cpu().numpy(), src, rejected, lambda k: want[(int(idx[k]), int(src[k][0]), int(src[k][1]))], ndt,
                       "stack of maps, %s, rejected %r" % (dtype, rejected))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", [256, 257])
def test_latency_sweep_at_its_last_batch_size_and_the_fall_back_above(vhp, oracle, n, dtype):
    import torch
    occ, src, _ = shapes.batch("w8", n)
    c = _context(vhp, occ, kernel=4)
    d_src = torch.from_numpy(np.array(src)).cuda()
    got = _launch(vhp, c, d_src, n, occ, dtype)
    # (vhp_choice.hpp use_lat: asked for by name, the latency sweep takes up to 256 sources)
    assert (c.last_sweep_kernel() == 4) == (n <= 256), c.last_sweep_kernel()
    _assert_fields(got, src, (), _single_map_want(oracle, "w8", src), _types(vhp, dtype)[2], "kernel 4, %d sources, %s" % (n, dtype))
