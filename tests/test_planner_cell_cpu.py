"""One planner step's per-cell work (csrc/vhp_planner_cell.hpp: planner_unswept, eval_d_dev, planner_h, push_rank, key_less -- what the
epilogue kernels of the plain, batch and speculative solves call), built with the host compiler into tests/planner_cell_driver.cpp and
held to the CPU oracle's planner_step: the pick, the bits of its h, the labels and the union after the step, and the number of pushes.
No GPU.  The grids are the ones no GPU planner test used to reach: 1 x 1 up to 5 x 4, every pivot and every end, on and off the
border, so that the pivot-on-row-0-then-off-it sequence and push_rank's branch for empty quadrants are decided here, by the device's
own text, before a kernel runs.
The local field the driver is given holds 1.0 in every cell the pivot does not sweep (row 0 / column 0) -- what a field
that is not cleared between pivots may hold -- so that only planner_unswept keeps those cells out of the union, the labels and the heap.
The driver is built twice: plain, and with the address and undefined-behaviour sanitizers; every case runs through both."""
import functools
import struct

import numpy as np
import pytest

import edge_solves as es
import planner_cell_lib as pcl
from planner_cell_lib import compare as _compare, first_state as _first_state, run as _run
from schedule_model import first_touch_rank

GRIDS = ((1, 1), (1, 2), (2, 1), (2, 2), (1, 7), (7, 1), (3, 3), (2, 9), (9, 2), (5, 4))   # (nx, ny)
THRESHOLDS = (0.0, 0.5, 1.0)


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    return pcl.build_drivers(str(tmp_path_factory.mktemp("planner_cell_driver")))


def _maps_of(nx, ny):
    """the all-free grid, then each single cell blocked in turn"""
    free = np.ones((ny, nx), np.uint8)
    yield free
    for k in range(nx * ny):
        occ = free.copy()
        occ.reshape(-1)[k] = 0
        yield occ


@functools.lru_cache(maxsize=None)
def _first_steps(nx, ny):
    steps = []
    for occ in _maps_of(nx, ny):
        for thr in THRESHOLDS:
            for s in range(nx * ny):
                pivot = (s % nx, s // nx)
                came, vg, piv = _first_state(occ, pivot)
                for e in range(nx * ny):
                    steps.append((occ, pivot, (e % nx, e // nx), thr, 0, piv, came, vg))
    return steps


_results = {}


def _exhaustive(oracle, drivers, nx, ny):
    """(steps, results) of the first steps of a grid and of the second steps that follow them, computed once per process"""
    if (nx, ny) not in _results:
        first = _first_steps(nx, ny)
        got = _compare(oracle, drivers, first)
        second = []
        for (occ, pivot, end, thr, nb, piv, came, vg), (pick, rank, tied, status) in zip(first, got):
            if status == 0 and pick != pivot:
                came, vg = came.copy(), vg.copy()
                oracle.planner_step(occ, pivot, end, thr, 0, piv, came, vg)   # the state the oracle leaves
                second.append((occ, pick, end, thr, 1, np.array([pivot, pick], np.int32), came, vg))
        _results[(nx, ny)] = (first, got, second, _compare(oracle, drivers, second))
    return _results[(nx, ny)]


@pytest.mark.parametrize("nx,ny", GRIDS)
def test_first_and_second_steps(oracle, drivers, nx, ny):
    """every pivot, every end, every single blocked cell, three thresholds; then the step from every pick that is not the pivot"""
    first, got, second, got2 = _exhaustive(oracle, drivers, nx, ny)
    n = nx * ny
    assert len(first) == len(got) == (n + 1) * len(THRESHOLDS) * n * n
    assert len(second) == len(got2)
    on = lambda p: p[0] == 0 or p[1] == 0
    on_off = sum(1 for s in second if on(tuple(s[5][0])) and not on(s[1]))
    off_on = sum(1 for s in second if not on(tuple(s[5][0])) and on(s[1]))
    print("%d x %d: %d first steps, %d second steps, of them %d from a pivot on row 0 / column 0 to one off it and %d the reverse" % (
        nx, ny, len(first), len(second), on_off, off_on))
    if n > 1:
        assert len(second) >= 1
    # the sequence of the stale-field hazard: a pivot on row 0 / column 0 followed by one off it (a cell off both needs two rows and two
    # columns).  The reverse cannot be a pick: a pivot off row 0 and column 0 sweeps neither, so no cell of them is pushed.
    assert (on_off >= 1) == (nx > 1 and ny > 1)
    assert off_on == 0
    # threshold 1.0 on a blocked pivot lights nothing: the empty heap
    assert any(g[3] == 3 for g in got)


def test_blocked_pivot_map(oracle, drivers):
    """the 9 x 9 serpentine at threshold 0.0: `v >= 0` labels and pushes dark and blocked cells, and the pivots are blocked cells -- every
    step of the oracle's solve from each corner, with the state the oracle left"""
    occ = es.serpentine(9, 9)
    steps, n_blocked = [], 0
    for start, end in (((0, 0), (8, 8)), ((8, 8), (0, 0)), ((0, 8), (8, 0)), ((8, 0), (0, 8)), ((0, 0), (0, 8))):
        r = oracle.solve(occ, start, end, 0.0, 12)
        came, vg, _ = _first_state(occ, start)
        for nb in range(r["n_pivots"]):   # (the list's last entry was picked, or is `end`, and is not swept)
            piv = r["pivots"][: nb + 1]
            pivot = tuple(int(v) for v in piv[nb])
            steps.append((occ, pivot, end, 0.0, nb, piv.copy(), came.copy(), vg.copy()))
            n_blocked += int(occ[pivot[1], pivot[0]] == 0)
            oracle.planner_step(occ, pivot, end, 0.0, nb, piv, came, vg)
    assert len(steps) >= 20 and n_blocked >= 10, (len(steps), n_blocked)
    _compare(oracle, drivers, steps)


def test_ties_and_rank_branches(oracle, drivers):
    """at least 100 steps have two or more cells at the minimal h; among them each of push_rank's four branches holds the pick at least
    once, and pivots on each of the four borders occur"""
    tied = []
    for nx, ny in GRIDS:
        first, got, second, got2 = _exhaustive(oracle, drivers, nx, ny)
        tied += [(s[0].shape, s[1], g) for s, g in zip(first + second, got + got2) if g[3] == 0 and g[2] >= 2]
    assert len(tied) >= 100, len(tied)
    assert {g[1] >> 40 for _, _, g in tied} == {0, 1, 2, 3}
    assert any(p[0] == 0 for _, p, _ in tied) and any(p[1] == 0 for _, p, _ in tied)
    assert any(p[0] == nx - 1 and nx > 1 for (ny, nx), p, _ in tied) and any(p[1] == ny - 1 and ny > 1 for (ny, nx), p, _ in tied)
    # the branch for empty quadrants (dx == 0 && sx >= 1 is false): a pivot in column 0 whose pick lies straight below it
    assert any(p[0] == 0 and g[0][0] == 0 and g[0][1] < p[1] and g[1] >> 40 == 3 for _, p, g in tied)
    assert any(p[0] >= 1 and g[0][0] == p[0] and g[0][1] < p[1] and g[1] >> 40 == 2 for _, p, g in tied)


def test_python_copy_of_the_rank(drivers):
    """schedule_model.first_touch_rank, the formula test_schedule_model.py holds to the oracle, equals the device's push_rank on every
    (pivot, cell) of the grids above and of the serpentine's"""
    grids = GRIDS + ((9, 9),)
    lines = _run(drivers, "rank", b"".join(struct.pack("<2i", nx, ny) for nx, ny in grids), len(grids))
    for (nx, ny), line in zip(grids, lines):
        got = [int(v, 16) for v in line.split()]
        want = [first_touch_rank(nx, ny, sx, sy, x, y) for sy in range(ny) for sx in range(nx) for y in range(ny) for x in range(nx)]
        assert got == want, (nx, ny)
