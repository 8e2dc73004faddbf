"""The clearance field on the device (vhp_map_clearance, vhp_maps_clearance and their _device forms): against numpy
(clearance_cases.clearance, written from the definition) at the word edges, around the kernel's tile height and over more than one
tile each way; against the inflation that is already on the device -- (field > p) must be vhp_map_occupancy after vhp_inflate_map(p)
--; on a stack of windows, a range of it and more maps than a grid dimension holds; the fleet recipe of INTEGRATION.md against the
inflation route; then state, errors and the agreement of the host and device forms.  Every comparison is exact."""
import os
import re

import numpy as np
import pytest

import clearance_cases as cc
import inflate_cases as ic
import maps
import window_cases as wc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE_NAMES = {ic.DISC: "disc", ic.SQUARE: "square", ic.DIAMOND: "diamond"}
P_MAX = ic.GPU_FOOTPRINTS + ((ic.DISC, 4224),)


def _tile_rows():
    """kClearanceTileRows, from the one place that defines it"""
    text = open(os.path.join(HERE, "..", "visibility-heuristic-path-planner_amd", "csrc", "vhp_clearance.hip.h")).read()
    found = re.findall(r"^constexpr int kClearanceTileRows = (\d+);", text, re.M)
    assert len(found) == 1
    return int(found[0])


TY = _tile_rows()


@pytest.fixture(scope="module")
def vhp():
    import torch  # noqa: F401
    import vhp_amd
    return vhp_amd


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d cells differ, first at %r: %r vs %r" % (what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def _against_numpy(vhp, occ, p_maxes):
    ny, nx = occ.shape
    c = vhp.Context(0)
    c.set_map(occ)
    fields = set()
    for shape, p_max in p_maxes:
        for border in (False, True):
            got = c.map_clearance(p=p_max, shape=SHAPE_NAMES[shape], border=border)
            _same(got, cc.clearance(occ, shape, p_max, border), "%d x %d, %s p_max %d, border %r" % (nx, ny, SHAPE_NAMES[shape], p_max, border))
            fields.add(got.tobytes())
    return fields


# ---- 1. against numpy --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ny", ic.GPU_SIDES[1])
@pytest.mark.parametrize("nx", ic.GPU_SIDES[0])
def test_map_clearance_equals_numpy(vhp, nx, ny):
    occ = wc.random_map(nx, ny, seed=1000 * nx + ny, blocked=0.03)
    occ[ny // 2, nx // 2] = 0   # (at least one obstacle, whatever the side)
    fields = _against_numpy(vhp, occ, P_MAX)
    if nx >= 63 and ny >= 64:
        # (p_max = 0 knows no border, and the two largest discs may agree on a map this small: at most three fields coincide)
        assert len(fields) >= 2 * len(P_MAX) - 3, "p_max and a border flag that change nothing show nothing"


@pytest.mark.parametrize("ny", [TY - 1, TY, TY + 1, 2 * TY + 1])
def test_heights_around_the_tile(vhp, ny):
    occ = wc.random_map(65, ny, seed=ny, blocked=0.01)
    occ[0, 64] = occ[ny - 1, 0] = 0
    _against_numpy(vhp, occ, P_MAX)


def test_more_than_one_tile_each_way(vhp):
    assert 200 > 64 and 200 > TY
    _against_numpy(vhp, wc.random_map(200, 200, seed=200, blocked=0.01), ((ic.DISC, 8),))


# ---- 2. against the inflation that is already on the device ------------------------------------------------------------------------
def test_field_above_p_is_the_inflated_map(vhp):
    nx, ny = 130, 129
    # (shape, p_max, the p compared): the disc to its largest reach, a square and a diamond
    todo = ((ic.DISC, 4096, (0, 1, 8, 4096)), (ic.SQUARE, 5, (3,)), (ic.DIAMOND, 4, (2,)))
    c, ref = vhp.Context(0), vhp.Context(0)
    names = set()
    for name, occ in ic.case_maps(nx, ny, seed=77):
        names.add(name.split("_")[0])
        c.set_map(occ)
        for border in (False, True):
            for shape, p_max, ps in todo:
                field = c.map_clearance(p=p_max, shape=SHAPE_NAMES[shape], border=border)
                for p in ps:
                    ref.set_map(occ)   # (a fresh state holding the same map)
                    ref.inflate_map(p=p, shape=SHAPE_NAMES[shape], border=border)
                    _same((field > p).astype(np.uint8), ref.map_occupancy(), "map %s, %s p %d of p_max %d, border %r" % (name, SHAPE_NAMES[shape], p, p_max, border))
    assert names == {"corner00", "corner10", "corner01", "corner11", "cell", "free", "blocked", "random"}


# ---- 3. the stack -------------------------------------------------------------------------------------------------------------------
def test_maps_clearance_on_windows(vhp):
    occ = wc.random_map(130, 65, seed=11, blocked=0.03)
    origins = np.array([(-3, -2), (100, 40), (60, -5), (-10, 50), (120, 60), (30, 20)], np.int32)   # over every edge and corner, and inside
    c = vhp.Context(0)
    c.set_map(occ)
    c.set_maps_windows(origins, 70, 30)
    stack = c.maps_occupancy()
    assert stack.shape == (6, 30, 70) and len({m.tobytes() for m in stack}) == 6
    for shape, p_max, border in ((ic.DISC, 8, False), (ic.DISC, 4096, True), (ic.DIAMOND, 3, False)):
        got = c.maps_clearance(p=p_max, shape=SHAPE_NAMES[shape], border=border)
        _same(got, cc.clearance(stack, shape, p_max, border), "the windows, %s p_max %d, border %r" % (SHAPE_NAMES[shape], p_max, border))
    _same(c.maps_clearance(2, 3, radius=2), cc.clearance(stack[2:5], ic.DISC, 4), "maps 2 .. 4")
    _same(c.maps_occupancy(), stack, "the stack after the calls")


def test_device_form_writes_exactly_its_range(vhp):
    import torch
    stack = np.stack([wc.random_map(65, 33, seed=40 + k, blocked=0.03) for k in range(5)])
    cells = 65 * 33
    c = vhp.Context(0)
    c.set_maps(stack)
    buf = torch.full((7 + 3 * cells + 9,), 0x5A5A, dtype=torch.int16, device="cuda")
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    c.maps_clearance_device(buf.data_ptr() + 2 * 7, 1, 3, radius=3, border=True)
    torch.cuda.synchronize()
    c.set_stream(None)
    host = buf.cpu().numpy().view(np.uint16)
    assert (host[:7] == 0x5A5A).all() and (host[7 + 3 * cells:] == 0x5A5A).all()
    want = cc.clearance(stack[1:4], ic.DISC, 9, True)
    assert not (want == 0x5A5A).any()
    _same(host[7:7 + 3 * cells].reshape(3, 33, 65), want, "maps 1 .. 3 through the device form")


def test_many_maps(vhp):
    n = 65537
    rng = np.random.default_rng(4)
    stack = (rng.random((n, 2, 3)) >= 0.2).astype(np.uint8)
    stack[0], stack[-1] = [[1, 1, 1], [1, 1, 0]], [[0, 1, 1], [1, 1, 1]]
    c = vhp.Context(0)
    c.set_maps(stack)
    got = c.maps_clearance(p=2)
    assert got.shape == (n, 2, 3)
    picks = [0, 65535, 65536, n - 1] + rng.integers(0, n, 200).tolist()
    _same(got[picks], cc.clearance(stack[picks], ic.DISC, 2), "the picked maps")
    F = cc.FAR
    assert got[0].tolist() == [[F, 2, 1], [F, 1, 0]] and got[-1].tolist() == [[0, 1, F], [1, 2, F]]


# ---- 4. the fleet recipe: K configuration-space maps from one field ------------------------------------------------------------------
def test_fleet_from_one_field(vhp):
    import torch
    occ = maps.random_rect_map(150, 131, 30, 3, 18, 3, 18, 17)
    ny, nx = occ.shape
    ps = (0, 4, 9)
    c = vhp.Context(0)
    c.set_map(occ)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    field = torch.empty((ny, nx), dtype=torch.int16, device="cuda")
    c.map_clearance_device(field.data_ptr(), p=max(ps))
    wide = field.to(torch.int32) & 0xFFFF                    # (uint16 read as such: VHP_CLEARANCE_FAR is above every p)
    masks = torch.stack([(wide > p).to(torch.uint8) for p in ps]).contiguous()
    c.set_maps_device(masks.data_ptr(), len(ps), nx, ny)
    got = c.maps_occupancy()
    c.set_stream(None)
    ref = vhp.Context(0)
    ref.set_map(occ)
    ref.set_maps_windows(np.zeros((len(ps), 2), np.int32), nx, ny)
    for k, p in enumerate(ps):
        ref.inflate_maps(k, 1, p=p)
    _same(got, ref.maps_occupancy(), "the three classes' maps")
    assert len({m.tobytes() for m in got}) == 3 and got[0].tobytes() == (occ != 0).astype(np.uint8).tobytes()


# ---- 5. state and errors --------------------------------------------------------------------------------------------------------------
def test_calls_change_no_state(vhp):
    occ = maps.random_rect_map(120, 97, 14, 3, 20, 3, 20, 5)
    stack = np.stack([wc.random_map(40, 30, seed=k, blocked=0.1) for k in range(3)])
    c = vhp.Context(0)
    c.set_map(occ)
    c.set_maps(stack)
    src = [tuple(int(v) for v in p) for p in maps.free_sources(occ, 3, 9)]
    before = c.sweep_batch(src)
    ms = c.last_elapsed_ms()
    assert ms > 0
    first = c.map_clearance(radius=8)
    c.maps_clearance(radius=2, border=True)
    assert c.last_elapsed_ms() == ms   # (not timed)
    _same(c.map_occupancy(), (occ != 0).astype(np.uint8), "the map after the calls")
    _same(c.maps_occupancy(), stack, "the stack after the calls")
    _same(c.sweep_batch(src), before, "the sweep after the calls")
    _same(c.map_clearance(radius=8), first, "the field, again")


def test_host_and_device_forms_agree(vhp):
    import torch
    occ = wc.random_map(130, 65, seed=8, blocked=0.02)
    stack = np.stack([wc.random_map(63, 20, seed=k, blocked=0.05) for k in range(4)])
    c = vhp.Context(0)
    c.set_map(occ)
    c.set_maps(stack)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    one = torch.zeros((65, 130), dtype=torch.int16, device="cuda")
    many = torch.zeros((4, 20, 63), dtype=torch.int16, device="cuda")
    c.map_clearance_device(one.data_ptr(), p=3, shape="square", border=True)
    c.maps_clearance_device(many.data_ptr(), radius=5)
    torch.cuda.synchronize()
    c.set_stream(None)
    _same(one.cpu().numpy().view(np.uint16), c.map_clearance(p=3, shape="square", border=True), "the single map")
    _same(many.cpu().numpy().view(np.uint16), c.maps_clearance(radius=5), "the stack")


def test_errors(vhp):
    import torch
    lib = vhp.load_library()
    occ = maps.random_rect_map(120, 97, 14, 3, 20, 3, 20, 5)
    out = np.full(120 * 97 * 4, 0x1234, np.uint16)
    d_out = torch.full((120 * 97 * 4 + 8,), 0x1234, dtype=torch.int16, device="cuda")
    c = vhp.Context(0)
    # nothing set
    assert lib.vhp_map_clearance(c.h, 0, 1, 0, out.ctypes.data) == vhp.VHP_ERR_NO_MAP
    assert lib.vhp_map_clearance_device(c.h, 0, 1, 0, d_out.data_ptr()) == vhp.VHP_ERR_NO_MAP
    assert lib.vhp_maps_clearance(c.h, 0, 1, 0, 1, 0, out.ctypes.data) == vhp.VHP_ERR_NO_MAP
    assert lib.vhp_maps_clearance_device(c.h, 0, 1, 0, 1, 0, d_out.data_ptr()) == vhp.VHP_ERR_NO_MAP
    c.set_map(occ)
    assert lib.vhp_maps_clearance(c.h, 0, 1, 0, 1, 0, out.ctypes.data) == vhp.VHP_ERR_NO_MAP   # (a single map is no stack)
    assert lib.vhp_maps_clearance_device(c.h, 0, 1, 0, 1, 0, d_out.data_ptr()) == vhp.VHP_ERR_NO_MAP
    stack = np.stack([wc.random_map(40, 30, seed=k, blocked=0.1) for k in range(4)])
    c.set_maps(stack)
    # the footprint and the flags, as vhp_inflate_map refuses them
    bad = ((3, 1, 0), (-1, 1, 0), (0, -1, 0), (0, 4225, 0), (1, 65, 0), (2, 65, 0), (0, 1, 2), (0, 1, 3), (0, 1, -1))   # (shape, p_max, flags)
    for shape, p_max, flags in bad:
        assert lib.vhp_map_clearance(c.h, shape, p_max, flags, out.ctypes.data) == vhp.VHP_ERR_ARG, (shape, p_max, flags)
        assert lib.vhp_map_clearance_device(c.h, shape, p_max, flags, d_out.data_ptr()) == vhp.VHP_ERR_ARG, (shape, p_max, flags)
        assert lib.vhp_maps_clearance(c.h, 0, 4, shape, p_max, flags, out.ctypes.data) == vhp.VHP_ERR_ARG, (shape, p_max, flags)
        assert lib.vhp_maps_clearance_device(c.h, 0, 4, shape, p_max, flags, d_out.data_ptr()) == vhp.VHP_ERR_ARG, (shape, p_max, flags)
    # the range, as vhp_maps_occupancy refuses it
    for first, count in ((-1, 1), (4, 1), (0, 5), (0, 0), (3, 2), (0, -1)):
        assert lib.vhp_maps_clearance(c.h, first, count, 0, 1, 0, out.ctypes.data) == vhp.VHP_ERR_ARG, (first, count)
        assert lib.vhp_maps_clearance_device(c.h, first, count, 0, 1, 0, d_out.data_ptr()) == vhp.VHP_ERR_ARG, (first, count)
    # null pointers, and a device pointer at an odd address
    assert lib.vhp_map_clearance(c.h, 0, 1, 0, None) == vhp.VHP_ERR_ARG
    assert lib.vhp_map_clearance_device(c.h, 0, 1, 0, None) == vhp.VHP_ERR_ARG
    assert lib.vhp_maps_clearance(c.h, 0, 1, 0, 1, 0, None) == vhp.VHP_ERR_ARG
    assert lib.vhp_maps_clearance_device(c.h, 0, 1, 0, 1, 0, None) == vhp.VHP_ERR_ARG
    assert lib.vhp_map_clearance_device(c.h, 0, 1, 0, d_out.data_ptr() + 1) == vhp.VHP_ERR_ARG
    assert lib.vhp_maps_clearance_device(c.h, 0, 1, 0, 1, 0, d_out.data_ptr() + 3) == vhp.VHP_ERR_ARG
    with pytest.raises(vhp.VhpError) as e:
        c.map_clearance(p=4225)
    assert e.value.code == vhp.VHP_ERR_ARG
    with pytest.raises(vhp.VhpError) as e:
        c.maps_clearance(2, 3, p=1)
    assert e.value.code == vhp.VHP_ERR_ARG
    # a refused call writes nothing
    torch.cuda.synchronize()
    c.sync()
    assert (out == 0x1234).all() and bool((d_out == 0x1234).all())
    # the largest p_max are taken
    for shape, p_max in ((0, 4224), (1, 64), (2, 64)):
        assert lib.vhp_map_clearance(c.h, shape, p_max, 1, out.ctypes.data) == vhp.VHP_OK
        _same(out[:120 * 97].reshape(97, 120), cc.clearance(occ, shape, p_max, True), "shape %d at its largest p_max" % shape)
    assert (out[120 * 97:] == 0x1234).all()
