"""What the map layer (csrc/vhp_maps.hip.h) shares between the calls on the packed maps, where one call's slip would show in another:
  1. the single map is packed by the stack's kernels as a stack of one: what set_map and set_maps(occ[None]) put on the device reads
     back as occ, and a ray cast (both packed copies) and a sweep on the single map are the oracle's, at the word edges of both sides;
  2. the host forms of the occupancy, clearance, ray-cast, line-of-sight and sweep calls all stage through one output scratch: one
     Context driven through them on a grid, a smaller one and the first again gives what fresh Contexts give;
  3. the sliced copy-out reaches its second slice in the clearance and occupancy calls (513 fields of 2 MiB, 1025 maps of 1 MiB),
     and the maps there are the ones asked for -- the stacks cut on the device, so nothing large is uploaded.
Every comparison is exact."""
import numpy as np
import pytest

import maps
import window_cases as wc

pytestmark = pytest.mark.gpu

SIDES = [(1, 1), (63, 2), (64, 1), (65, 3), (128, 64), (129, 65), (131, 77)]   # (nx, ny)
GRIDS = {"A": (96, 80, 31), "B": (131, 77, 47)}   # nx, ny, seed: tests/test_gpu_scratch_reuse.py's
BIG = 1024


@pytest.fixture(scope="module")
def vhp():
    import torch  # noqa: F401  (first, so the extension shares torch's HIP runtime)
    import vhp_amd
    return vhp_amd


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d elements differ, first at %r: %r vs %r" % (what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


# ---- 1. the single map through the stack packers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny", SIDES)
def test_single_map_is_a_stack_of_one(vhp, oracle, nx, ny):
    occ = wc.random_map(nx, ny, seed=1000 * nx + ny, blocked=1 / 3)
    free = (occ != 0).astype(np.uint8)
    what = "%d x %d" % (nx, ny)
    c = vhp.Context(0)
    c.set_map(occ)
    _same(c.map_occupancy(), free, what + ": the map of set_map")
    c.set_maps(occ[None])
    _same(c.maps_occupancy(), free[None], what + ": the stack of one")
    if (nx, ny) == (1, 1):
        return
    assert 0 < free.sum() < free.size, what
    src = maps.free_sources(occ, 3, 7)
    _same(c.raycast_batch(src), np.stack([oracle.raycast_all(occ, int(x), int(y)) for x, y in src]), what + ": ray cast")
    _same(c.sweep_batch(src), np.stack([oracle.sweep_full(occ, int(x), int(y)) for x, y in src]), what + ": sweep")


# ---- 2. one output scratch behind every host form ------------------------------------------------------------------------------------
def _pairs(occ):
    """five (x0, y0, x1, y1) between free cells"""
    p = maps.free_sources(occ, 10, 21)
    return np.ascontiguousarray(np.concatenate([p[:5], p[5:]], axis=1), np.int32)


def _calls(vhp, stack):
    """the sequence: (name, needs the stack set, the call on a context)"""
    occ = stack[0]
    src = maps.free_sources(occ, 3, 3)
    pairs = _pairs(occ)
    return [("sweep_batch of 3", False, lambda c: c.sweep_batch(src)),
            ("map_clearance", False, lambda c: c.map_clearance(radius=3)),
            ("set_maps", True, None),
            ("maps_occupancy", True, lambda c: c.maps_occupancy()),
            ("maps_clearance(1, 2)", True, lambda c: c.maps_clearance(1, 2, radius=3)),
            ("raycast_batch as uint8", True, lambda c: c.raycast_batch(src, vhp.U8)),
            ("line_of_sight of 5", True, lambda c: c.line_of_sight(pairs)),
            ("sweep_batch of 1", True, lambda c: c.sweep_batch(src[:1])),
            ("map_occupancy", True, lambda c: c.map_occupancy())]


def test_host_forms_share_one_output_scratch(vhp):
    stacks = {}
    for name, (nx, ny, seed) in GRIDS.items():
        stacks[name] = np.stack([maps.random_rect_map(nx, ny, 40, 3, 20, 3, 20, seed + 17 * k) for k in range(3)])
    fresh = {}
    c = vhp.Context(0)
    seen = set()
    for stage, name in enumerate("ABA"):
        stack = stacks[name]
        c.set_map(stack[0])
        for call, with_stack, run in _calls(vhp, stack):
            if run is None:
                c.set_maps(stack)
                continue
            if (name, call) not in fresh:
                f = vhp.Context(0)
                f.set_map(stack[0])
                if with_stack:
                    f.set_maps(stack)
                fresh[name, call] = run(f)
            got = run(c)
            _same(got, fresh[name, call], "stage %d, grid %s, %s" % (stage, name, call))
            seen.add(got.tobytes())
    assert len(seen) == 2 * 8   # (every call of a grid gives something of its own: none is compared with a stale copy of another's)


# ---- 3. the second slice of the shared copy-out --------------------------------------------------------------------------------------
def _origins(n):
    k = np.arange(n, dtype=np.int64)
    return np.ascontiguousarray(np.stack([(37 * k) % 301 - 150, (53 * k) % 211 - 105], axis=1), np.int32)


def _big_map():
    return wc.random_map(BIG, BIG, seed=1024, blocked=1 / 3)


def _cuts(occ, origins, picks):
    """the numpy cut of the picked windows, and that they are no near copies of one another: map 0 and every pair of neighbours
    among the picks differ in far more cells than a border holds"""
    cut = {k: wc.cut(occ, [origins[k, 0]], [origins[k, 1]], BIG, BIG)[0, 0] for k in picks}
    for a, b in [(picks[0], k) for k in picks[1:]] + list(zip(picks, picks[1:])):
        if a != b:
            assert (cut[a] != cut[b]).sum() > BIG * BIG // 10, (a, b)
    return cut


def test_clearance_second_slice(vhp):
    n = 513   # (2 MiB a field: a slice is 512 maps)
    occ, origins = _big_map(), _origins(n)
    picks = [0, 1, 511, 512]
    cut = _cuts(occ, origins, picks)
    c = vhp.Context(0)
    c.set_map(occ)
    c.set_maps_windows(origins, BIG, BIG)
    got = c.maps_clearance(p=9)
    assert got.shape == (n, BIG, BIG)
    ref = vhp.Context(0)
    for k in picks:
        ref.set_map(cut[k])
        _same(got[k], ref.map_clearance(p=9), "window %d" % k)
    del got


def test_occupancy_second_slice(vhp):
    n = 1025   # (1 MiB a map: a slice is 1024 maps)
    occ, origins = _big_map(), _origins(n)
    picks = [0, 1023, 1024]
    cut = _cuts(occ, origins, picks)
    c = vhp.Context(0)
    c.set_map(occ)
    c.set_maps_windows(origins, BIG, BIG)
    got = c.maps_occupancy()
    assert got.shape == (n, BIG, BIG)
    for k in picks:
        _same(got[k], cut[k], "window %d" % k)
    del got
