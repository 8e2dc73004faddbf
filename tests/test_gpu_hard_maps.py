"""Every sweep kernel and the planner on the hard maps (tests/hard_maps.py), on the GPU, bit for bit against the oracle.

The fields of these maps hold what rectangle and salt maps never do (tests/test_hard_maps.py asserts that they do): corridors whose
value decays to fp32-subnormal, to nothing in fp32, to fp64-subnormal and to an exact +0.0 by arithmetic alone -- strips that die by
decay and not behind a blocked cell, results that a flush-to-zero build would change --, and lattices whose lit cells are almost all
fractional, tens of thousands of them at or below the queue variant's 0.001.  All comparisons are byte equality; fp32 results are
compared with oracle.astype(float32).  Device outputs start as NaN (-7 for int32), so a cell nobody wrote fails.

Every (kernel, case) pair is supported (vhp_launch_plan.hpp lat_supported / pool_supported hold up to sides far above 1304), so no
pair is left out: a forced kernel that did not run fails its test."""
import numpy as np
import pytest

import hard_maps
from side_kernel_shapes import OFFSETS, VARIANT_PARAMS, _numpy_union
from test_gpu_planner import _assert_same_solution
from test_gpu_planner_batch import _assert_same as _assert_same_batch_result
from test_gpu_side_kernels import _assert_same

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
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    for k, v in options.items():
        c.set_option(k, v)
    return c


# ---- the sweeps: every case x dtype x launch -----------------------------------------------------------------------------------------

LAUNCHES = {   # vhp_set_option keys; "again": a second launch into the same buffer (the first one's tags and death records are stale by then)
    "auto": dict(kernel=0),
    "front": dict(kernel=1),
    "front_one_row_8_strips_slid": dict(kernel=1, rows_per_lane=1, strips=8, slide=1),
    "front_packed": dict(kernel=1, pack=1),
    "pool": dict(kernel=3),
    "lat": dict(kernel=4),
}


@pytest.mark.parametrize("launch", list(LAUNCHES))
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", hard_maps.CASE_NAMES)
def test_sweeps_on_hard_maps(vhp, oracle, record_property, name, dtype, launch):
    import torch
    occ, src = hard_maps.case(name)
    vdt, tdt, ndt = _types(vhp, dtype)
    want = hard_maps.fields(oracle, name).astype(ndt)
    options = LAUNCHES[launch]
    c = _context(vhp, occ, **options)
    d_src = torch.from_numpy(np.array(src)).cuda()
    out = torch.empty((len(src),) + occ.shape, dtype=tdt, device="cuda")
    kernel = None
    for rep in range(2):
        out.fill_(float("nan"))
        c.sweep_batch_device(d_src.data_ptr(), len(src), out.data_ptr(), dtype=vdt)
        c.sync()
        kernel = c.last_sweep_kernel()
        if options["kernel"]:
            assert kernel == options["kernel"], "%s: kernel %d was asked for, %d ran" % (name, options["kernel"], kernel)
        got = out.cpu().numpy()
        for k, (sx, sy) in enumerate(src):
            _assert_same(got[k], want[k], "%s %s %s (kernel %d), launch %d, source (%d,%d)" % (name, dtype, launch, kernel, rep, sx, sy))
        if kernel not in (3, 4):
            break
    if launch == "auto":
        record_property("kernel", kernel)
        print("kernel=0 on %s %s: kernel %d" % (name, dtype, kernel))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_host_entry_on_star328_lo(vhp, oracle, dtype):
    occ, src = hard_maps.case("star328_lo")
    vdt, _, ndt = _types(vhp, dtype)
    want = hard_maps.fields(oracle, "star328_lo").astype(ndt)
    c = vhp.Context(0)
    c.set_map(np.array(occ))
    got = c.sweep_batch(src, dtype=vdt)
    for k, (sx, sy) in enumerate(src):
        _assert_same(got[k], want[k], "star328_lo %s, host entry, source (%d,%d)" % (dtype, sx, sy))


# ---- a stack of maps, given as bytes and cut as windows --------------------------------------------------------------------------------

def _stack():
    """three 328 x 300 maps, and sources interleaved across them: (sources int32 [n, 2], map index int32 [n])"""
    salt = hard_maps.salt_walled(328, 300, 3, 0.15)
    salt_src = np.array([(160, 150), (0, 0), (327, 0), (0, 299), (327, 299), (167, 147), (164, 0)], np.int32)
    salt[salt_src[:, 1], salt_src[:, 0]] = 1
    per_map = [hard_maps.case("star328_lo"), hard_maps.case("dots3x5"), (salt, salt_src)]
    stack = np.stack([np.array(occ) for occ, _ in per_map])
    src, idx = [], []
    for k in range(max(len(s) for _, s in per_map)):
        for m, (_, s) in enumerate(per_map):
            if k < len(s):
                src.append(tuple(int(v) for v in s[k]))
                idx.append(m)
    return stack, np.array(src, np.int32), np.array(idx, np.int32)


@pytest.fixture(scope="module")
def stack_case(oracle):
    stack, src, idx = _stack()
    want = [oracle.sweep_full(stack[m], int(x), int(y)) for (x, y), m in zip(src, idx)]
    return stack, src, idx, want


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("how", ["bytes", "windows"])
def test_stack_of_hard_maps(vhp, stack_case, how, dtype):
    """how = windows: the same stack cut on the device from one 984 x 300 map that holds the three side by side.  (A window's first row
    and column are what the sweep of the whole map does not give, include/vhp.h; against the oracle on the window itself, as here,
    every cell is compared.)"""
    import torch
    stack, src, idx, want = stack_case
    vdt, tdt, ndt = _types(vhp, dtype)
    c = vhp.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    if how == "bytes":
        c.set_maps(stack)
    else:
        c.set_map(np.ascontiguousarray(np.concatenate(list(stack), axis=1)))
        c.set_maps_windows(np.array([(0, 0), (328, 0), (656, 0)], np.int32), 328, 300)
    assert (c.n_maps, c.maps_nx, c.maps_ny) == (3, 328, 300)
    d_src, d_idx = torch.from_numpy(src).cuda(), torch.from_numpy(idx).cuda()
    out = torch.empty((len(src), 300, 328), dtype=tdt, device="cuda")
    for rep in range(2):
        out.fill_(float("nan"))
        c.sweep_maps_batch_device(d_src.data_ptr(), d_idx.data_ptr(), len(src), out.data_ptr(), dtype=vdt)
        c.sync()
        got = out.cpu().numpy()
        for i, ((sx, sy), m) in enumerate(zip(src, idx)):
            _assert_same(got[i], want[i].astype(ndt), "stack as %s, %s (kernel %d), launch %d, source (%d,%d) on map %d" % (
                how, dtype, c.last_sweep_kernel(), rep, sx, sy, m))


# ---- the queue variant and its v > 0.001 ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["dots3x5", "dots2x2", "star401", "salt333"])
def test_queue_variant_on_hard_maps(vhp, oracle, name, dtype):
    import torch
    occ, src = hard_maps.case(name)
    vdt, tdt, ndt = _types(vhp, dtype)
    c = _context(vhp, occ)
    d_src = torch.from_numpy(np.array(src)).cuda()
    out = torch.full((len(src),) + occ.shape, float("nan"), dtype=tdt, device="cuda")
    c.sweep_batch_device(d_src.data_ptr(), len(src), out.data_ptr(), variant=vhp.SWEEP_QUEUE, dtype=vdt)
    c.sync()
    got = out.cpu().numpy()
    for k, (sx, sy) in enumerate(src):
        want = oracle.sweep_queue(np.array(occ), int(sx), int(sy))
        _assert_same(got[k], want.astype(ndt), "queue variant on %s, %s, source (%d,%d)" % (name, dtype, sx, sy))


# ---- the MATLAB-flavoured and the offset sweep ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("alpha,fac", VARIANT_PARAMS)
@pytest.mark.parametrize("name", ["dots3x5", "star_q1"])
def test_variant_sweep_on_hard_maps(vhp, oracle, name, alpha, fac):
    occ, src = hard_maps.case(name)
    c = vhp.Context(0)
    c.set_map(np.array(occ))
    got = c.sweep_batch_variant(src, alpha, fac)
    for k, (x, y) in enumerate(src):
        want = oracle.sweep_matlab(np.array(occ), int(x), int(y), alpha, fac)
        _assert_same(got[k], want, "variant sweep on %s alpha %g fac %g, source (%d,%d)" % (name, alpha, fac, x, y))


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("name", ["dots3x5", "star_q1"])
def test_offset_sweep_on_hard_maps(vhp, oracle, name, offset):
    occ, src = hard_maps.case(name)
    c = vhp.Context(0)
    c.set_map(np.array(occ))
    got = c.sweep_batch_offset(src, offset)
    for k, (x, y) in enumerate(src):
        want = oracle.sweep_full_offset(np.array(occ), int(x), int(y), offset)
        _assert_same(got[k], want, "offset sweep on %s offset %g, source (%d,%d)" % (name, offset, x, y))
        if offset == 0.0:   # include/vhp.h: offset 0 is computeVisibility() as the tuned kernels compute it
            _assert_same(got[k], hard_maps.fields(oracle, name)[k], "offset 0 against the plain sweep, %s source (%d,%d)" % (name, x, y))


# ---- the union: maxima among subnormals and fp32-flushed zeros -----------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_union_of_star328_lo_fields(vhp, oracle, dtype):
    import torch
    occ, src = hard_maps.case("star328_lo")
    vdt, tdt, ndt = _types(vhp, dtype)
    want = hard_maps.fields(oracle, "star328_lo").astype(ndt)
    wb, wa = _numpy_union(want, 0)
    c = _context(vhp, occ)
    d_src = torch.from_numpy(np.array(src)).cuda()
    swept = torch.full((len(src),) + occ.shape, float("nan"), dtype=tdt, device="cuda")
    c.sweep_batch_device(d_src.data_ptr(), len(src), swept.data_ptr(), dtype=vdt)
    for what, d_fields in (("swept fields", swept), ("the oracle's fields", torch.from_numpy(want).cuda())):
        best = torch.full(occ.shape, float("nan"), dtype=tdt, device="cuda")
        arg = torch.full(occ.shape, -7, dtype=torch.int32, device="cuda")
        c.union_fields_device(d_fields.data_ptr(), len(src), best.data_ptr(), arg.data_ptr(), dtype=vdt)
        c.sync()
        assert np.array_equal(best.cpu().numpy(), wb) and np.array_equal(arg.cpu().numpy(), wa), what
        _assert_same(best.cpu().numpy(), wb, "union of %s, %s: best" % (what, dtype))
        _assert_same(arg.cpu().numpy(), wa, "union of %s, %s: arg" % (what, dtype))


# ---- the planner ---------------------------------------------------------------------------------------------------------------------

THRESHOLDS = (0.5, 1e-3, 1e-30, 1e-320, 0.0, 1.0)   # (1e-320: a subnormal threshold)
PLANNER_MAPS = {"star401": 40, "dots3x5_333": 40, "star1304": 12}   # case: max_iter


def _ends(oracle, name):
    """The far corner, and -- beyond what a lit corner asks of the loop -- the darkest free cell of the start's own field away from the
    first row and column (those are never lit): an end the loop has to work for at the larger thresholds."""
    occ, src = hard_maps.case(name)
    ny, nx = occ.shape
    f = np.where(np.array(occ) != 0, hard_maps.fields(oracle, name)[0], np.inf)
    f[0, :] = f[:, 0] = np.inf
    y, x = np.unravel_index(int(np.argmin(f)), f.shape)
    return [(nx - 1, ny - 1), (int(x), int(y))]


def _queries(oracle, name):
    start = tuple(int(v) for v in hard_maps.case(name)[1][0])
    ends = _ends(oracle, name)
    if name == "star1304":   # (the darkest cell at three thresholds only: an oracle solve of 12 iterations there takes a second)
        pairs = [(ends[0], t) for t in THRESHOLDS] + [(ends[1], t) for t in (0.5, 1e-320, 0.0)]
    else:
        pairs = [(e, t) for e in ends for t in THRESHOLDS]
    return [start + e for e, _ in pairs], [t for _, t in pairs]


@pytest.mark.parametrize("name", list(PLANNER_MAPS))
def test_planner_on_hard_maps(vhp, oracle, name):
    """planner_solve against the oracle, then the same queries as one planner_solve_batch against the plain solves.  At thresholds at
    or below the corridors' values the labels and the heap's arg-min depend on cells that hold 1e-40 or 1e-320, and on the two
    alternating local fields being zero where a dead strip stored nothing."""
    occ, _ = hard_maps.case(name)
    occ = np.array(occ)
    max_iter = PLANNER_MAPS[name]
    queries, thr = _queries(oracle, name)
    c = vhp.Context(0)
    c.set_map(occ)
    plain, statuses = [], set()
    for (sx, sy, ex, ey), t in zip(queries, thr):
        got = c.planner_solve((sx, sy), (ex, ey), t, max_iter)
        want = oracle.solve(occ, (sx, sy), (ex, ey), t, max_iter)
        assert got["status"] in (vhp.VHP_OK, vhp.VHP_ERR_MAX_ITER, vhp.VHP_ERR_NOTHING_LIT)
        _assert_same_solution(got, want, "%s (%d,%d) -> (%d,%d) thr %g" % (name, sx, sy, ex, ey, t))
        plain.append(got)
        statuses.add(got["status"])
    print("%s: statuses %r, pivots %r, sweep kernel %d" % (name, sorted(statuses), [r["n_pivots"] for r in plain], c.last_sweep_kernel()))
    batch = c.planner_solve_batch(queries, thr, max_iter)
    for q, r in enumerate(batch):
        _assert_same_batch_result(r, plain[q], "%s batch query %d %r thr %g" % (name, q, queries[q], thr[q]), vhp)


def test_planner_maps_batch_on_hard_maps(vhp, oracle):
    """planner_solve_maps_batch on a stack of star401 and a 401 x 401 lattice: each query equals the plain solve on its map."""
    star = np.array(hard_maps.case("star401")[0])
    dots = hard_maps.dot_lattice(401, 401, 3, 5)
    dots[200, 200] = dots[400, 400] = 1
    stack = np.stack([star, dots])
    ends = _ends(oracle, "star401")
    queries, idx, thr = [], [], []
    for t in THRESHOLDS:
        queries += [(200, 200) + ends[0], (200, 200) + ends[1], (200, 200, 400, 400)]
        idx += [0, 0, 1]
        thr += [t] * 3
    c = vhp.Context(0)
    c.set_maps(stack)
    batch = c.planner_solve_maps_batch(queries, idx, thr, 40)
    for m in (0, 1):
        c.set_map(stack[m])
        for q in range(len(queries)):
            if idx[q] == m:
                what = "maps batch query %d %r on map %d thr %g" % (q, queries[q], m, thr[q])
                plain = c.planner_solve(queries[q][:2], queries[q][2:], thr[q], 40)
                _assert_same_batch_result(batch[q], plain, what, vhp)
                _assert_same_solution(plain, oracle.solve(stack[m], queries[q][:2], queries[q][2:], thr[q], 40), what + ", plain solve vs oracle")
