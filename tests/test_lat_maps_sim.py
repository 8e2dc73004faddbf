"""The latency sweep on a stack of maps (csrc/vhp_band.hpp BandWorker, STACK build: vhp_lat_maps_sweep) on the CPU simulator, against
the oracle bit for bit.  Sources of one launch lie on different maps of a stack of three; every field must be the oracle's on its own
map.  The stack's diagonal maps, built from its row-packed words (diag_word_from_rows: vhp_pack_diag_stack), must be exactly the
words vhp_pack_diag builds from each map's bytes.  No GPU needed; the gfx950 build is checked in tests/test_gpu_planner_maps.py."""
import numpy as np
import pytest

import lat_maps_sim
import maps
from sim_lib import POOL_BACKWARD, POOL_BURSTS, POOL_GREEDY, POOL_POINTS_ALWAYS, POOL_POINTS_RANDOM, POOL_RANDOM, POOL_ROUND_ROBIN

SHAPES = [  # W sweepers per workgroup, policy
    (12, POOL_ROUND_ROBIN | POOL_POINTS_ALWAYS),
    (12, POOL_RANDOM | POOL_POINTS_RANDOM),
    (4, POOL_GREEDY | POOL_POINTS_ALWAYS),
    (3, POOL_BURSTS | POOL_POINTS_RANDOM),
    (2, POOL_BACKWARD | POOL_POINTS_ALWAYS),
]
# from test_lat_sim.py's list: even widths, odd widths (the ODD build), a strip of a few rows, a tall grid
SIZES = [(8, 8), (16, 3), (10, 9), (2, 5), (104, 77), (101, 101), (105, 78), (130, 131), (200, 163), (71, 300)]


def _stack(nx, ny, seed):
    """Three maps of nx x ny and a cell (sx, sy) that is free on all of them; map 1 is map 0 plus a wall two cells to the cell's
    right (a wall that exists only in map 1), which blocks what map 0 lets through."""
    m0 = maps.random_rect_map(nx, ny, max(3, min(30, nx * ny // 400)), 1, max(nx // 8, 2), 1, max(ny // 8, 2), seed)
    m2 = maps.random_rect_map(nx, ny, max(3, min(30, nx * ny // 300)), 1, max(nx // 6, 2), 1, max(ny // 6, 2), seed + 1000)
    sx, sy = max(0, nx // 2 - 2), ny // 2
    m0[sy, sx] = m2[sy, sx] = 1
    if sx + 2 < nx:
        m0[max(0, sy - 1): sy + 2, sx + 1: sx + 3] = 1   # (free in map 0 around the wall's place ...)
    m1 = m0.copy()
    if sx + 2 < nx:
        m1[max(0, sy - 1): sy + 2, sx + 2] = 0           # (... a wall of up to three cells in map 1)
    return np.stack([m0, m1, m2]), (sx, sy)


def _launch(stack, cell, seed):
    """Sources of one launch over all three maps: the cell on maps 0 and 1, free cells of each map, corners."""
    ny, nx = stack.shape[1:]
    src, idx = [cell, cell], [0, 1]
    for k in range(3):
        for p in maps.free_sources(stack[k], 2, seed + k):
            src.append((int(p[0]), int(p[1])))
            idx.append(k)
    for k, (x, y) in ((2, (0, 0)), (1, (nx - 1, ny - 1))):
        if stack[k, y, x]:
            src.append((x, y))
            idx.append(k)
    return np.array(src, np.int32), np.array(idx, np.int32)


def _check(oracle, stack, src, idx, what, **kw):
    got, st = lat_maps_sim.lat_maps_sweep(stack, src, idx, **kw)
    assert st["deadlock"] == 0, "%s: every wavefront waiting %r" % (what, st)
    assert st["err"] == 0, what
    for k, ((sx, sy), m) in enumerate(zip(src.tolist(), idx.tolist())):
        want = oracle.sweep_full(stack[m], int(sx), int(sy))
        if got[k].tobytes() != want.tobytes():
            bad = np.argwhere(~((got[k] == want) | (np.isnan(got[k]) & np.isnan(want))))
            y, x = bad[0]
            raise AssertionError("%s, source %d (%d,%d) on map %d: %d cells differ, first at (x=%d,y=%d): got %r want %r" % (
                what, k, sx, sy, m, len(bad), x, y, got[k][y, x], want[y, x]))
    return got


@pytest.mark.parametrize("nx,ny", SIZES)
@pytest.mark.parametrize("halves", [1, 2])
def test_lat_maps_sim_against_the_oracle(oracle, nx, ny, halves):
    stack, cell = _stack(nx, ny, nx * 7 + ny)
    src, idx = _launch(stack, cell, nx + ny)
    for W, policy in SHAPES:
        got = _check(oracle, stack, src, idx, "%dx%d halves=%d W=%d policy=%d" % (nx, ny, halves, W, policy), W=W, policy=policy,
                     seed=nx + W, halves=halves)
        if nx >= 8 and ny >= 8:   # (map 1's wall changes the field of the source at the same cell of map 0)
            assert got[0].tobytes() != got[1].tobytes(), "%dx%d: the wall of map 1 changed nothing" % (nx, ny)


def test_lat_maps_sim_tall_grid_two_workgroups(oracle):
    """A side above 1024 -- the MULTI build's own sizes, two workgroups per unit -- with sources on all three maps."""
    stack, cell = _stack(72, 1100, 5)
    src, idx = _launch(stack, cell, 9)
    for W, policy in SHAPES[:3]:
        _check(oracle, stack, src, idx, "72x1100 W=%d policy=%d" % (W, policy), W=W, policy=policy, seed=W, halves=2)


def test_lat_maps_sim_map_index_outside_the_stack_is_rejected(oracle):
    stack, cell = _stack(40, 33, 3)
    src = np.array([cell, cell, cell, cell], np.int32)
    idx = np.array([0, -1, 3, 2], np.int32)
    got, st = lat_maps_sim.lat_maps_sweep(stack, src, idx, W=4, policy=POOL_RANDOM | POOL_POINTS_RANDOM)
    assert st["deadlock"] == 0 and st["err"] == 1
    assert np.isnan(got[1]).all() and np.isnan(got[2]).all()   # (their units did nothing)
    for k in (0, 3):
        assert got[k].tobytes() == oracle.sweep_full(stack[idx[k]], *cell).tobytes()


@pytest.mark.parametrize("nx,ny", [(1, 1), (8, 1), (3, 7), (64, 64), (65, 63), (130, 131), (200, 163), (971, 65)])
def test_stack_diagonal_words_equal_vhp_pack_diag(nx, ny):
    stack = np.stack([maps.random_rect_map(nx, ny, max(2, nx * ny // 300), 1, max(nx // 5, 2), 1, max(ny // 5, 2), s) for s in (1, 2, 3)])
    stack[1] = 1 - stack[1]   # (a map with most cells blocked)
    from_rows, from_bytes = lat_maps_sim.stack_diag_words(stack)
    assert from_rows.tobytes() == from_bytes.tobytes()
    assert from_rows.any()
