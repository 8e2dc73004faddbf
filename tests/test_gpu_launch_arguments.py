"""A launch's arguments belong to the launch.  One context carries the options that the planner loops and the host-buffer sweeps must
not see -- "field_stride" (nx * ny + 24) and vhp_timing -- through every planner solve and sweep in turn, on a 100 x 98 map and a stack
of three such maps.  Every solve gives the bytes of the same call on a fresh context with default options; the host-buffer sweeps
return packed fields; per-launch timing times the three batch-sweep launches and none of the planner loops'; and the last call, a
device sweep of three sources, still writes its fields "field_stride" apart (the library has no getter: that launch is how the option
reads back) and leaves the pads alone.  Once with the kernel the library chooses (the latency sweep at this size: vhp_last_sweep_kernel
4 after every solve) and once with option kernel = 1, where the planners fall back to their front sweeps."""
import numpy as np
import pytest

import maps
from test_gpu_planner_batch import _assert_same, _free_pairs

pytestmark = pytest.mark.gpu

NX, NY, PAD = 100, 98, 24
MAX_ITER = 40
MAP_IDX = [2, 0, 1]
SENTINEL = -7.0
# vhp_timing entries of one sequence: one launch each by sweep_batch, sweep_maps_batch (three fields are one slice) and
# sweep_batch_device; the planner loops' launches take no event pairs.  A property of the code, the same for every kernel.
TIMED_BY_THE_SWEEPS = 3


@pytest.fixture(scope="module")
def vhp():
    import torch  # noqa: F401
    import vhp_amd
    return vhp_amd


def _map(seed):
    return maps.random_rect_map(NX, NY, 14, 4, 24, 4, 24, seed)


@pytest.fixture(scope="module")
def case():
    occ = _map(3)
    stack = np.stack([_map(20 + k) for k in range(3)])
    q = _free_pairs(occ, 4, 5)
    stack_q = [_free_pairs(stack[m], 1, 30 + m)[0] for m in MAP_IDX]
    src = np.ascontiguousarray(maps.free_sources(occ, 3, 9), np.int32)
    stack_src = np.ascontiguousarray([stack_q[i][:2] for i in range(3)], np.int32)
    return dict(occ=occ, stack=stack, plain=q[0], batch=q[1:], thr=[0.25, 0.1, 0.5], stack_q=stack_q, src=src, stack_src=stack_src)


def _context(vhp, case):
    c = vhp.Context(0)
    c.set_map(case["occ"])
    c.set_maps(case["stack"])
    return c


def _calls(c, case):
    """the solves and host-buffer sweeps in the order of the issue; after each solve, the kernel that swept its iterations"""
    out, kernels = {}, []
    sx, sy, ex, ey = case["plain"]
    out["plain"] = c.planner_solve((sx, sy), (ex, ey), 0.25, MAX_ITER)
    kernels.append(c.last_sweep_kernel())
    out["spec"] = c.planner_solve_speculative((sx, sy), (ex, ey), 0.25, MAX_ITER, k=4)
    kernels.append(c.last_sweep_kernel())
    out["batch"] = c.planner_solve_batch(case["batch"], case["thr"], MAX_ITER)
    kernels.append(c.last_sweep_kernel())
    out["maps_batch"] = c.planner_solve_maps_batch(case["stack_q"], MAP_IDX, case["thr"], MAX_ITER)
    kernels.append(c.last_sweep_kernel())
    return out, kernels


def _sweeps(c, case):
    return c.sweep_batch(case["src"]), c.sweep_maps_batch(case["stack_src"], MAP_IDX)


@pytest.fixture(scope="module")
def fresh(vhp, case):
    """the same calls on a context with default options"""
    c = _context(vhp, case)
    out, kernels = _calls(c, case)
    assert kernels == [4, 4, 4, 4], kernels
    fields, stack_fields = _sweeps(c, case)
    c.close()
    return out, fields, stack_fields


@pytest.mark.parametrize("kernel", [0, 1])
def test_options_reach_only_the_launches_they_belong_to(vhp, case, fresh, kernel):
    import torch
    want, want_fields, want_stack_fields = fresh
    stride = NX * NY + PAD
    c = _context(vhp, case)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    c.set_option("field_stride", stride)
    c.set_option("kernel", kernel)
    c.timing(True)
    got, kernels = _calls(c, case)
    assert kernels == [kernel or 4] * 4, kernels
    assert len(c.timing_collect()) == 0   # (no planner loop is timed launch by launch)
    for name in ("plain", "spec"):
        _assert_same(got[name], want[name], "%s, kernel %d" % (name, kernel), vhp)
    for name in ("batch", "maps_batch"):
        for q in range(3):
            _assert_same(got[name][q], want[name][q], "%s query %d, kernel %d" % (name, q, kernel), vhp)
    assert got["plain"]["status"] in (vhp.VHP_OK, vhp.VHP_ERR_MAX_ITER), got["plain"]["status"]
    for name in ("came_from", "vis_global", "vis_local", "pivots"):   # (the exact speculative solve is the plain one)
        assert got["spec"][name].tobytes() == got["plain"][name].tobytes(), name

    fields, stack_fields = _sweeps(c, case)
    assert fields.shape == (3, NY, NX) and fields.tobytes() == want_fields.tobytes()
    assert stack_fields.shape == (3, NY, NX) and stack_fields.tobytes() == want_stack_fields.tobytes()

    d_src = torch.from_numpy(case["src"]).cuda()
    d_out = torch.full((3, stride), SENTINEL, dtype=torch.float64, device="cuda")
    c.sweep_batch_device(d_src.data_ptr(), 3, d_out.data_ptr())
    c.sync()
    out = d_out.cpu().numpy()
    assert out[:, : NX * NY].reshape(3, NY, NX).tobytes() == want_fields.tobytes()
    assert (out[:, NX * NY:] == SENTINEL).all()
    assert len(c.timing_collect()) == TIMED_BY_THE_SWEEPS
    c.close()
