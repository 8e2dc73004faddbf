"""Pool-sweep and latency-sweep launches time themselves by the stamps their own kernels write (csrc/vhp_stamps.hpp): no event is
recorded around them.  On the batches of pool_launch_ends_shapes.py -- the smallest that take each path of a pool launch's two ends --
and on three latency-sweep launches (no pre-kernel, the order pre-kernel, two workgroups per unit): the fields equal the oracle bit
for bit in buffers prefilled with NaN, vhp_last_elapsed_ms and vhp_timing_collect report finite, positive times within the host's wall
time around launch and sync, a ring of two slots takes two of five timed launches and leaves the rest to event pairs, and the
bookkeeping survives other kernels, other streams, other contexts, a union and vhp_probe_stores in between.

A stamped launch is told from one timed by events by what the two calls report for it: the same float, bit for bit (one slot serves
both), where the event pair inside ev0 / ev1 reads less than they do."""
import math
import time

import numpy as np
import pytest

import maps
import pool_launch_ends_shapes as shapes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vhp():
    import torch  # noqa: F401
    import vhp_amd
    return vhp_amd


def _dtypes(vhp, dtype):
    import torch
    return (vhp.F64, torch.float64, np.float64) if dtype == "f64" else (vhp.F32, torch.float32, np.float32)


def _context(vhp, occ, kernel, **options):
    import torch
    c = vhp.Context(0)
    c.set_map(np.array(occ))
    c.set_option("kernel", kernel)
    for k, v in options.items():
        c.set_option(k, v)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


def _launch(vhp, c, d_src, n, d_out, vdt, outside=()):
    """One launch into d_out (prefilled with NaN) and the sync behind it; the host's wall time around both, in ms."""
    import torch
    d_out.fill_(float("nan"))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c.sweep_batch_device(d_src.data_ptr(), n, d_out.data_ptr(), dtype=vdt)
    if outside:  # the error flag as ever: the launch runs, and the sync behind it names the bad source
        with pytest.raises(vhp.VhpError) as e:
            c.sync()
        assert e.value.code == vhp.VHP_ERR_SOURCE_OOB
    else:
        c.sync()
    return (time.perf_counter() - t0) * 1e3


def _check_fields(got, want, src, outside, ndt, what):
    for k in range(len(src)):
        if k in outside:   # a rejected source's field is left as it was
            assert np.isnan(got[k]).all(), "%s: the field of source %d (outside the map) was written" % (what, k)
            continue
        w = want[k].astype(ndt)
        if got[k].tobytes() != w.tobytes():
            bad = np.argwhere(~((got[k] == w) | (np.isnan(got[k]) & np.isnan(w))))
            y, x = bad[0]
            raise AssertionError("%s, source %d (%d,%d): %d cells differ, first at (x=%d,y=%d): got %r want %r" % (
                what, k, src[k][0], src[k][1], len(bad), x, y, got[k][y, x], w[y, x]))


def _timed_off_and_on(vhp, c, kernel, occ, src, outside, want, dtype, what):
    """The assertions every stamped launch shape is held to."""
    import torch
    vdt, tdt, ndt = _dtypes(vhp, dtype)
    n, ny, nx = len(src), occ.shape[0], occ.shape[1]
    d_src = torch.from_numpy(np.array(src)).cuda()
    d_out = torch.empty((n, ny, nx), dtype=tdt, device="cuda")
    # timing off: slot 0 of the stamps serves vhp_last_elapsed_ms
    wall = _launch(vhp, c, d_src, n, d_out, vdt, outside)
    assert c.last_sweep_kernel() == kernel
    ms = c.last_elapsed_ms()
    print("%s: timing off %.4f ms, wall %.4f ms" % (what, ms, wall))
    assert math.isfinite(ms) and 0.0 < ms <= wall, (ms, wall)
    assert c.last_elapsed_ms() == ms   # (read once, the same answer ever after)
    assert len(c.timing_collect()) == 0
    _check_fields(d_out.cpu().numpy(), want, src, outside, ndt, what + ", timing off")
    # timing on, a ring of two slots, five launches before one collect: two by their stamps, three by the event fallback
    c.timing(True, prealloc=2)
    walls, lasts = [], []
    for k in range(5):
        walls.append(_launch(vhp, c, d_src, n, d_out, vdt, outside))
        lasts.append(c.last_elapsed_ms())
    got = d_out.cpu().numpy()
    times = [float(t) for t in c.timing_collect()]
    print("%s: timing on %s ms, last %s, wall %s" % (what, ["%.4f" % t for t in times], ["%.4f" % t for t in lasts], ["%.4f" % t for t in walls]))
    assert len(times) == 5
    for k in range(5):
        assert math.isfinite(times[k]) and 0.0 < times[k] <= walls[k], (k, times[k], walls[k])
        assert math.isfinite(lasts[k]) and 0.0 < lasts[k] <= walls[k], (k, lasts[k], walls[k])
    # the stamped ones: one slot serves both calls, the same float; the others: the pair lies inside ev0 / ev1
    assert times[0] == lasts[0] and times[1] == lasts[1], (times, lasts)
    for k in range(2, 5):
        assert times[k] <= lasts[k], (k, times, lasts)
    assert c.last_elapsed_ms() == lasts[4]
    assert len(c.timing_collect()) == 0   # a second collect returns none
    c.timing(False)
    _check_fields(got, want, src, outside, ndt, what + ", timing on")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["96_static_round", "9_fewer_units_than_groups", "96_anyw", "97_two_outside"])
def test_pool_sweep_stamps(vhp, oracle, name, dtype):
    occ, src, outside = shapes.batch(name)
    c = _context(vhp, occ, 3)
    _timed_off_and_on(vhp, c, 3, occ, src, outside, shapes.oracle_fields(oracle, name), dtype, "pool %s %s" % (name, dtype))


# name: (nx, ny, sources, options): eight workgroups and no pre-kernel (every workgroup leaves a begin stamp); 320 units on 256 CUs
# (vhp_lat_order runs first and leaves the one begin stamp); two workgroups per unit (the build whose bands read across workgroups)
LAT_CASES = {
    "one_source_no_pre_kernel": (72, 40, 1, {}),
    "40_sources_order_kernel": (136, 136, 40, {}),
    "two_workgroups_per_unit": (1040, 64, 1, {"lat_workgroups": 2}),
}
_lat = {}


def _lat_case(oracle, name):
    if name not in _lat:
        nx, ny, n, _ = LAT_CASES[name]
        occ = maps.random_rect_map(nx, ny, 8, 2, max(nx // 6, 3), 2, max(ny // 6, 3), nx + ny + n)
        src = maps.free_sources(occ, n, nx + n).copy()
        occ.setflags(write=False)
        src.setflags(write=False)
        _lat[name] = (occ, src, {k: oracle.sweep_full(np.array(occ), int(sx), int(sy)) for k, (sx, sy) in enumerate(src)})
    return _lat[name]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", list(LAT_CASES))
def test_latency_sweep_stamps(vhp, oracle, name, dtype):
    occ, src, want = _lat_case(oracle, name)
    c = _context(vhp, occ, 4, **LAT_CASES[name][3])
    _timed_off_and_on(vhp, c, 4, occ, src, (), want, dtype, "lat %s %s" % (name, dtype))


def test_pool_front_and_latency_launches_in_one_timed_sequence(vhp, oracle):
    import torch
    occ, src, _ = shapes.batch("96_static_round")
    want = shapes.oracle_fields(oracle, "96_static_round")
    n, ny, nx = len(src), occ.shape[0], occ.shape[1]
    c = _context(vhp, occ, 3)
    d_src = torch.from_numpy(np.array(src)).cuda()
    d_out = torch.empty((n, ny, nx), dtype=torch.float64, device="cuda")
    c.timing(True, prealloc=8)
    lasts, walls = [], []
    for kernel, n_k in ((3, n), (1, n), (4, 8), (3, n)):
        c.set_option("kernel", kernel)
        walls.append(_launch(vhp, c, d_src, n_k, d_out, vhp.F64))
        assert c.last_sweep_kernel() == kernel
        lasts.append(c.last_elapsed_ms())
        _check_fields(d_out[:n_k].cpu().numpy(), want, src[:n_k], (), np.float64, "kernel %d" % kernel)
    times = [float(t) for t in c.timing_collect()]
    print("pool, front, latency, pool: %s ms; last %s" % (["%.4f" % t for t in times], ["%.4f" % t for t in lasts]))
    # one entry per launch, oldest first: the stamped ones are what vhp_last_elapsed_ms said right behind them, the front sweep's
    # event pair lies inside its ev0 / ev1
    assert len(times) == 4
    assert (times[0], times[2], times[3]) == (lasts[0], lasts[2], lasts[3])
    assert 0.0 < times[1] <= lasts[1] <= walls[1]
    assert all(math.isfinite(t) and 0.0 < t <= w for t, w in zip(times, walls))
    assert len(c.timing_collect()) == 0


def test_union_behind_a_stamped_sweep_leaves_its_time(vhp):
    # tests/test_gpu_dist.py checks this on the default kernel (ev0 / ev1); here behind the pool sweep, whose time is in slot 0
    import torch
    occ = maps.random_rect_map(328, 300, 30, 3, 40, 3, 40, 5)
    src = maps.free_sources(occ, 8, 8)
    c = _context(vhp, occ, 3)
    out = torch.empty((len(src),) + occ.shape, dtype=torch.float64, device="cuda")
    d_src = torch.from_numpy(np.ascontiguousarray(src, np.int32)).cuda()
    c.sweep_batch_device(d_src.data_ptr(), len(src), out.data_ptr())
    assert c.last_sweep_kernel() == 3
    best = torch.empty(occ.shape, dtype=torch.float64, device="cuda")
    arg = torch.empty(occ.shape, dtype=torch.int32, device="cuda")
    c.union_fields_device(out.data_ptr(), len(src), best.data_ptr(), arg.data_ptr())   # (before the time is first asked for)
    ms = c.last_elapsed_ms()
    assert math.isfinite(ms) and ms > 0
    c.union_fields_device(out.data_ptr(), len(src), best.data_ptr(), arg.data_ptr())
    torch.cuda.synchronize()
    assert c.last_elapsed_ms() == ms
    assert np.array_equal(best.cpu().numpy(), out.cpu().numpy().max(axis=0))


def test_stamped_launches_on_two_streams(vhp, oracle):
    import torch
    name = "9_fewer_units_than_groups"
    occ, src, _ = shapes.batch(name)
    want = shapes.oracle_fields(oracle, name)
    n, ny, nx = len(src), occ.shape[0], occ.shape[1]
    c = _context(vhp, occ, 3)
    main, side = torch.cuda.current_stream(), torch.cuda.Stream()
    d_src = torch.from_numpy(np.array(src)).cuda()
    outs = [torch.full((n, ny, nx), float("nan"), dtype=torch.float64, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    # timing off: each launch's time is readable behind it, whichever stream it went out on
    for k, s in enumerate((main, side, main)):
        c.set_stream(s.cuda_stream)
        c.sweep_batch_device(d_src.data_ptr(), n, outs[k].data_ptr())
        ms = c.last_elapsed_ms()
        assert math.isfinite(ms) and ms > 0, (k, ms)
    torch.cuda.synchronize()
    for k in range(3):
        _check_fields(outs[k].cpu().numpy(), want, src, (), np.float64, "launch %d" % k)
    # timing on: three launches, none read until all are out
    c.timing(True, prealloc=4)
    for k, s in enumerate((main, side, main)):
        c.set_stream(s.cuda_stream)
        c.sweep_batch_device(d_src.data_ptr(), n, outs[k].data_ptr())
        torch.cuda.synchronize()   # (one scratch per context: the next launch must not overtake this one on the other stream)
    times = [float(t) for t in c.timing_collect()]
    assert len(times) == 3 and all(math.isfinite(t) and t > 0 for t in times), times
    assert c.last_elapsed_ms() == times[2]
    c.timing(False)


def test_two_contexts_collect_their_own(vhp):
    import torch
    ctxs, bufs = [], []
    for name in ("96_static_round", "9_fewer_units_than_groups"):
        occ, src, _ = shapes.batch(name)
        c = _context(vhp, occ, 3)
        c.timing(True, prealloc=4)
        ctxs.append(c)
        bufs.append((torch.from_numpy(np.array(src)).cuda(), len(src), torch.empty((len(src),) + occ.shape, dtype=torch.float64, device="cuda")))
    lasts = {0: [], 1: []}
    for k in (0, 1, 0):
        d_src, n, d_out = bufs[k]
        ctxs[k].sweep_batch_device(d_src.data_ptr(), n, d_out.data_ptr())
        lasts[k].append(ctxs[k].last_elapsed_ms())
    for k in (0, 1):
        times = [float(t) for t in ctxs[k].timing_collect()]
        assert times == lasts[k] and all(t > 0 for t in times), (k, times, lasts[k])
        assert len(ctxs[k].timing_collect()) == 0


def test_probe_stores_behind_a_stamped_sweep_leaves_nothing_timed(vhp):
    import torch
    occ, src, _ = shapes.batch("9_fewer_units_than_groups")
    c = _context(vhp, occ, 3)
    d_src = torch.from_numpy(np.array(src)).cuda()
    d_out = torch.empty((len(src),) + occ.shape, dtype=torch.float64, device="cuda")
    c.sweep_batch_device(d_src.data_ptr(), len(src), d_out.data_ptr())
    assert c.last_elapsed_ms() > 0
    buf = torch.empty((16, 1000, 1000), dtype=torch.float64, device="cuda")
    c.probe_stores(buf.data_ptr(), buf.numel() * 8)
    with pytest.raises(vhp.VhpError) as e:
        c.last_elapsed_ms()
    assert e.value.code == vhp.VHP_ERR_ARG and "nothing timed yet" in str(e.value)
    # ... and the next sweep is timed again
    c.sweep_batch_device(d_src.data_ptr(), len(src), d_out.data_ptr())
    assert c.last_elapsed_ms() > 0
