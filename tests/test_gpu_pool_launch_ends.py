"""The two ends of a pool-sweep launch on the GPU: the order pre-kernel's records (vhp_pool_order) and the sweep kernel's first
round, on the batches of pool_launch_ends_shapes.py, and vhp_timing's events around them.

Each batch is launched twice on one context, with vhp_timing off and then on: both results equal the oracle bit for bit (so they
equal each other), and the timed launch reports one finite, positive time that does not exceed the wall time of the launch."""
import math
import time

import numpy as np
import pytest

import pool_launch_ends_shapes as shapes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vhp():
    import torch  # noqa: F401
    import vhp_amd
    return vhp_amd


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", list(shapes.SHAPES))
def test_pool_launch_ends_bit_exact_with_timing_off_and_on(vhp, oracle, name, dtype):
    import torch
    occ, src, outside = shapes.batch(name)
    want = shapes.oracle_fields(oracle, name)
    n, ny, nx = len(src), occ.shape[0], occ.shape[1]
    vdt, tdt, ndt = (vhp.F64, torch.float64, np.float64) if dtype == "f64" else (vhp.F32, torch.float32, np.float32)
    c = vhp.Context(0)
    c.set_map(np.array(occ))
    c.set_option("kernel", 3)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    d_src = torch.from_numpy(np.array(src)).cuda()
    results = []
    for timed in (False, True):
        d_out = torch.full((n, ny, nx), float("nan"), dtype=tdt, device="cuda")
        torch.cuda.synchronize()
        c.timing(timed)
        t0 = time.perf_counter()
        c.sweep_batch_device(d_src.data_ptr(), n, d_out.data_ptr(), dtype=vdt)
        if outside:  # the error flag as ever: the launch runs, and the sync behind it names the bad source
            with pytest.raises(vhp.VhpError) as e:
                c.sync()
            assert e.value.code == vhp.VHP_ERR_SOURCE_OOB
        else:
            c.sync()
        wall_ms = (time.perf_counter() - t0) * 1e3
        assert c.last_sweep_kernel() == 3
        ms = c.timing_collect()
        c.timing(False)
        if timed:
            assert len(ms) == 1
            print("%s %s: launch %.4f ms by its events, %.4f ms wall" % (name, dtype, float(ms[0]), wall_ms))
            assert math.isfinite(float(ms[0])) and 0.0 < float(ms[0]) <= wall_ms
        else:
            assert len(ms) == 0
        results.append(d_out.cpu().numpy())
    for got, what in zip(results, ("timing off", "timing on")):
        for k in range(n):
            if k in outside:   # a rejected source's field is left as it was
                assert np.isnan(got[k]).all(), "%s %s, %s: the field of source %d (outside the map) was written" % (name, dtype, what, k)
                continue
            w = want[k].astype(ndt)
            if got[k].tobytes() != w.tobytes():
                bad = np.argwhere(~((got[k] == w) | (np.isnan(got[k]) & np.isnan(w))))
                y, x = bad[0]
                raise AssertionError("%s %s, %s, source %d (%d,%d): %d cells differ, first at (x=%d,y=%d): got %r want %r" % (
                    name, dtype, what, k, src[k][0], src[k][1], len(bad), x, y, got[k][y, x], w[y, x]))
    assert results[0].tobytes() == results[1].tobytes()
