"""Builds and runs tests/planner_cell_driver.cpp (one planner step's per-cell work, csrc/vhp_planner_cell.hpp, on the host) and holds its
output to the CPU oracle's planner_step -- TEST INFRASTRUCTURE ONLY (numpy, no GPU).  Shared by tests/test_planner_cell_cpu.py (exhaustive
small grids) and tests/test_edge_solves.py (every step of the edge solves).
The local field the driver is given holds STALE in every cell the pivot does not sweep (row 0 / column 0) -- what a field
that is not cleared between pivots may hold -- so that only planner_unswept keeps those cells out of the union, the labels and the heap."""
import functools
import os
import struct
import subprocess

import numpy as np

import cpu_driver
from oracle_lib import UNLABELLED
from schedule_model import first_touch_rank

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(HERE, "planner_cell_driver.cpp")
UNL32 = 0xFFFFFFFF
STALE = 1.0


def build_drivers(out_dir):
    """[plain build, build under the address and undefined-behaviour sanitizers]"""
    return [cpu_driver.build(DRIVER, out_dir, "planner_cell_driver_" + name, flags=("-ffp-contract=off", "-O2"),
                             includes=(cpu_driver.CSRC, cpu_driver.INCLUDE), sanitized=san)
            for name, san in (("plain", False), ("san", True))]


def labels32(came):
    return np.where(came >= np.uint64(UNL32), np.uint64(UNL32), came).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def visits(nx, ny, sx, sy):
    """int64 [ny, nx]: how many of the four quadrant nests of updateVisibility visit each cell from the pivot (sx, sy) -- the axes
    through the pivot belong to two quadrants, the pivot to four, and the nests towards lower x / lower y stop at x = 1 / y = 1"""
    y, x = np.mgrid[0:ny, 0:nx]
    dx, dy = x - sx, y - sy
    n = ((dx >= 0) & (dy >= 0)).astype(np.int64)
    n += (dx <= 0) & (dy >= 0) & (x >= 1) & (sx >= 1)
    n += (dx <= 0) & (dy <= 0) & (x >= 1) & (y >= 1) & (sx >= 1) & (sy >= 1)
    n += (dx >= 0) & (dy <= 0) & (y >= 1) & (sy >= 1)
    return n


def first_state(occ, pivot):
    """what solve() sets up before its first step: nothing lit, the start labelled 0"""
    came = np.full(occ.shape, UNLABELLED, np.uint64)
    came[pivot[1], pivot[0]] = 0
    return came, np.zeros(occ.shape, np.float64), np.array([pivot], np.int32)


def oracle_steps(oracle, steps):
    """steps: [(occ, pivot, end, thr, nb, pivots [nb + 1, 2], came before, union before)] -> the driver's input records and, per step,
    what the oracle gives: (status, top, bits of top_h, n_pushed, labels after, union after)"""
    blob, want = [], []
    for occ, pivot, end, thr, nb, piv, came, vg in steps:
        ny, nx = occ.shape
        came, vg = came.copy(), vg.copy()
        head = struct.pack("<7id", nx, ny, pivot[0], pivot[1], end[0], end[1], nb, thr)
        before = vg.tobytes() + labels32(came).tobytes() + np.ascontiguousarray(piv, np.int32).tobytes()
        r = oracle.planner_step(occ, pivot, end, thr, nb, piv, came, vg)
        local = r["vis_local"]
        unswept = visits(nx, ny, pivot[0], pivot[1]) == 0
        assert not local[unswept].any()
        local[unswept] = STALE
        blob.append(head + local.tobytes() + before)
        want.append((r["status"], r["top"], struct.pack("<d", r["top_h"]).hex(), r["n_pushed"], came, vg))
    return b"".join(blob), want


def run(drivers, mode, blob, n):
    """the driver's n output lines for `blob` in `mode` ("step" or "rank"), the same from both builds"""
    outs = []
    for exe in drivers:
        p = subprocess.run([exe, mode], input=blob, capture_output=True, check=False)
        assert p.returncode == 0, (exe, p.returncode, p.stderr.decode()[-2000:])
        outs.append(p.stdout)
    assert outs[0] == outs[1], "the sanitizer build and the plain build disagree"
    lines = outs[0].decode().splitlines()
    assert len(lines) == n
    return lines


def compare(oracle, drivers, steps):
    """every step through both drivers and the oracle; returns per step (pick, rank of the pick, cells at the minimal h, oracle status)"""
    blob, want = oracle_steps(oracle, steps)
    out = []
    for k, (line, (status, top, hbits, n_pushed, came, vg)) in enumerate(zip(run(drivers, "step", blob, len(steps)), want)):
        occ, pivot, end, thr, nb = steps[k][:5]
        ny, nx = occ.shape
        what = "step %d: %d x %d, pivot %r, end %r, threshold %g, label %d, map %r" % (k, nx, ny, pivot, end, thr, nb, occ.tolist())
        f = line.split()
        pick, h, rank, tied, pushed, cells = (int(f[0]), int(f[1])), int(f[2], 16), int(f[3], 16), int(f[4]), int(f[5]), f[6]
        n = nx * ny
        assert [int(v, 16) for v in f[7: 7 + n]] == labels32(came).reshape(-1).tolist(), what + ": labels"
        assert [int(v, 16) for v in f[7 + n: 7 + 2 * n]] == vg.view(np.uint64).reshape(-1).tolist(), what + ": union"
        marks = np.frombuffer(cells.encode(), np.uint8).reshape(ny, nx)
        is_pushed = marks == ord("p")
        assert pushed == int(is_pushed.sum())
        assert int(visits(nx, ny, pivot[0], pivot[1])[is_pushed].sum()) == n_pushed, what + ": pushes"
        assert np.array_equal(marks == ord("u"), visits(nx, ny, pivot[0], pivot[1]) == 0), what + ": unswept cells"
        if status == 3:   # nothing pushed: the reference would call top() on an empty heap
            assert pick == (-1, -1) and pushed == 0, what
        else:
            assert status == 0 and pick == top, "%s: pick %r, the oracle's top %r (%d cells at the minimal h)" % (what, pick, top, tied)
            assert struct.pack("<Q", h).hex() == hbits, what + ": h"
            assert tied >= 1 and rank == first_touch_rank(nx, ny, pivot[0], pivot[1], pick[0], pick[1])
        out.append((pick, rank, tied, status))
    return out


def replay(oracle, occ, start, end, thr, r):
    """the steps of the oracle's solve r, one per pivot, each with the state the oracle left before it; also returns that state after
    the last step (labels, union)"""
    came, vg, _ = first_state(occ, start)
    steps = []
    for nb in range(r["n_pivots"]):   # (the list's last entry was picked, or is `end`, and is not swept)
        piv = r["pivots"][: nb + 1].copy()
        pivot = tuple(int(v) for v in piv[nb])
        steps.append((occ, pivot, end, thr, nb, piv, came.copy(), vg.copy()))
        oracle.planner_step(occ, pivot, end, thr, nb, piv, came, vg)
    return steps, came, vg
