"""The inputs of tests/test_gpu_side_kernels.py: the entry points beside the tuned sweeps and the planner, at the sizes where their
loops first repeat (tests/test_side_kernel_shapes.py proves, without a GPU, that every input is past the size it is meant to pass).

  A  host staging: more than 1 GiB of fields, so stage_slices (csrc/vhp_capi.hip) copies, launches and copies out a second slice;
  B  the queue variant: more sources than one launch of launch_queue_sweep_impl (csrc/vhp_queue.hip.h) holds scratch for;
  C  the union kernel: more cells than one pass of launch_union's capped grid (csrc/vhp_union.hip.h), and fields a stride apart;
  D  the variant and offset sweeps (csrc/vhp_variant.hip.h): fronts longer than the workgroup, LDS either side of 64 KB, side 4096;
  E  the variant planner: every status, ties of its pick, a side above 1024.

Every input is built once and handed out read-only; oracle results are computed once per distinct input and shared."""
import numpy as np

import edge_inputs
import maps

_cache = {}
_want = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- the union's helpers (tests/test_union.py imports them from here) ------------------------------------------------------------

def _numpy_union(fields, first_index):
    """(best, arg): sequential max-union, replace on strict improvement only"""
    best = np.full(fields.shape[1:], -1.0, fields.dtype)
    arg = np.full(fields.shape[1:], 0x7fffffff, np.int32)
    for k in range(fields.shape[0]):
        better = fields[k] > best
        best = np.where(better, fields[k], best)
        arg = np.where(better, np.int32(first_index + k), arg)
    return best, arg


def _tied_fields(rng, n, ny, nx, dtype):
    """random fields in [0, 1] with many exact ties: values from a small set, whole fields repeated, zeros"""
    f = rng.choice(np.array([0.0, 0.25, 0.5, 0.75, 1.0]), size=(n, ny, nx)).astype(dtype)
    f += (rng.rand(n, ny, nx) < 0.3) * rng.rand(n, ny, nx).astype(dtype) * 0.1
    if n > 3:
        f[3] = f[1]          # two equal fields: every cell a tie between sources 1 and 3
        f[n - 1] = f[0]
    f[:, : ny // 4] = 0.0    # a region where every source is dark: the lowest index wins
    return np.ascontiguousarray(f.astype(dtype))


# ---- A. host staging past one slice ---------------------------------------------------------------------------------------------

STAGE_NX = STAGE_NY = 1024
STAGE_FIELD_BYTES = STAGE_NX * STAGE_NY * 8          # fp64
# csrc/vhp_capi.hip stage_slices: `slice = max(1, min(n_src, (1 << 30) / field))` sources per copy-in, launch and copy-out
STAGE_SLICE = 2**30 // STAGE_FIELD_BYTES
STAGE_SOURCES = STAGE_SLICE + 3
STAGE_REPEAT = (64, 63)   # source 64 is source 63 again: one position twice, next to each other


def _stage_map(seed):
    return maps.random_rect_map(STAGE_NX, STAGE_NY, 40, 20, 120, 20, 120, seed)


def _stage_positions(occ_list):
    """Five distinct positions: a free interior cell, two corners, a blocked cell, a second free interior cell (on the first map)."""
    occ = occ_list[0]
    free = [tuple(int(v) for v in s) for s in maps.free_sources(occ, 2, 19)]
    blocked = np.argwhere(occ == 0)
    by, bx = (int(v) for v in blocked[len(blocked) // 2])
    pos = [free[0], (0, 0), (STAGE_NX - 1, STAGE_NY - 1), (bx, by), free[1]]
    assert len(set(pos)) == 5 and occ[by, bx] == 0 and all(occ[y, x] for x, y in (pos[0], pos[1], pos[2], pos[4]))
    return pos


def _stage_sources(pos):
    src = np.array([pos[i % len(pos)] for i in range(STAGE_SOURCES)], np.int32)
    src[STAGE_REPEAT[0]] = src[STAGE_REPEAT[1]]
    return src


def stage_batch():
    """(occ uint8 [1024, 1024], sources int32 [131, 2]) for vhp_sweep_batch: 131 fp64 fields of 8 MiB, slices of 128."""
    def make():
        occ = _stage_map(3)
        return _frozen(occ, _stage_sources(_stage_positions([occ])))
    return _once("stage", make)


def stage_maps_batch():
    """(occ uint8 [2, 1024, 1024], sources int32 [131, 2], map index int32 [131]) for vhp_sweep_maps_batch."""
    def make():
        occ = np.stack([_stage_map(3), _stage_map(4)])
        src = _stage_sources(_stage_positions(occ))
        idx = np.array([(i // 3) % 2 for i in range(STAGE_SOURCES)], np.int32)
        # the second slice is not the first one again: a dropped `+ s0` on either array changes a field
        head, tail = slice(0, 3), slice(STAGE_SLICE, STAGE_SLICE + 3)
        assert (idx[tail] != idx[head]).any() and (src[tail] != src[head]).any()
        return _frozen(occ, src, idx)
    return _once("stage_maps", make)


def stage_oracle_fields(oracle):
    """{(sx, sy): the oracle's fp64 field} for the distinct sources of stage_batch()"""
    if "stage" not in _want:
        occ, src = stage_batch()
        _want["stage"] = {xy: oracle.sweep_full(np.array(occ), *xy) for xy in sorted({(int(x), int(y)) for x, y in src})}
    return _want["stage"]


def stage_maps_oracle_fields(oracle):
    """{(map, sx, sy): the oracle's fp64 field on the source's own map} for stage_maps_batch()"""
    if "stage_maps" not in _want:
        occ, src, idx = stage_maps_batch()
        keys = sorted({(int(k), int(x), int(y)) for (x, y), k in zip(src, idx)})
        _want["stage_maps"] = {(k, x, y): oracle.sweep_full(np.array(occ[k]), x, y) for k, x, y in keys}
    return _want["stage_maps"]


# ---- B. the queue variant -------------------------------------------------------------------------------------------------------

QUEUE_NX, QUEUE_NY = 400, 300
QUEUE_CELLS = QUEUE_NX * QUEUE_NY
# csrc/vhp_queue.hip.h launch_queue_sweep_impl: `slice = max(1, min(n_src, (1 << 30) / (cells * 33 + 64)))` sources per launch
QUEUE_SLICE = 2**30 // (33 * QUEUE_CELLS + 64)
QUEUE_SOURCES = QUEUE_SLICE + 3
QUEUE_OBSTACLES = 260


def queue_batch():
    """(occ uint8 [300, 400], sources int32 [274, 2]): twelve distinct positions in turn -- the four corners, a blocked cell, seven
    free cells -- on a map dense enough that a flood (one lane per source) stays short."""
    def make():
        nx, ny = QUEUE_NX, QUEUE_NY
        occ = maps.random_rect_map(nx, ny, QUEUE_OBSTACLES, 3, 28, 3, 28, 23)
        blocked = np.argwhere(occ == 0)
        by, bx = (int(v) for v in blocked[len(blocked) // 3])
        pos = [tuple(int(v) for v in s) for s in maps.free_sources(occ, 7, 29)]
        pos[1:1] = [(0, 0), (nx - 1, ny - 1)]
        pos[5:5] = [(bx, by), (nx - 1, 0)]
        pos.append((0, ny - 1))
        assert len(pos) == 12 and len(set(pos)) == 12 and occ[by, bx] == 0
        src = np.array([pos[i % 12] for i in range(QUEUE_SOURCES)], np.int32)
        assert (src[QUEUE_SLICE:] != src[:3]).any()
        return _frozen(occ, src)
    return _once("queue", make)


def queue_oracle_fields(oracle):
    if "queue" not in _want:
        occ, src = queue_batch()
        _want["queue"] = {xy: oracle.sweep_queue(np.array(occ), *xy) for xy in sorted({(int(x), int(y)) for x, y in src})}
    return _want["queue"]


def queue_small():
    """(occ uint8 [97, 120], sources int32 [n, 2]): edge_inputs.edge_map(120, 97), for fp32 and the device entry point."""
    return _once("queue_small", lambda: _frozen(*edge_inputs.edge_map(120, 97, 41)))


def queue_small_oracle_fields(oracle):
    if "queue_small" not in _want:
        occ, src = queue_small()
        _want["queue_small"] = {xy: oracle.sweep_queue(np.array(occ), *xy) for xy in sorted({(int(x), int(y)) for x, y in src})}
    return _want["queue_small"]


# ---- C. the union past one pass of its grid, and field_stride -------------------------------------------------------------------

# csrc/vhp_union.hip.h launch_union: `cap = n_cus * 16` workgroups of kUnionThreads = 256 threads, a thread owns two cells; so the
# kernel's `p += step` / `c += step` run again only above 2 * 256 * 16 = 8192 cells per CU
UNION_CELLS_PER_CU_AND_PASS = 2 * 256 * 16
UNION_GRIDS = {"odd": (2311, 2275), "even": (2310, 2276)}   # odd cells: the partials' cell path and the fields' last single cell
UNION_FIELDS = 6                                             # the four-at-a-time body and a remainder of two
UNION_FIRST_INDEX = 100
UNION_CUTS = ((0, 2), (2, 5), (5, 6))                        # the partials: three cuts ...
UNION_SLOTS = (2, 0, 1)                                      # ... in scrambled slots
STRIDE_GRID = (203, 150)
STRIDE_FIELDS = 5
STRIDE_PADS = {"pairs": 6, "cells": 5}                       # an even stride: the 16-byte path; an odd one: cell by cell


def union_fields(grid, dtype):
    """fp64 fields [6, ny, nx] with ties (_tied_fields), or the same values in fp32 (a cast keeps equal values equal)"""
    def make():
        nx, ny = UNION_GRIDS[grid]
        return _frozen(_tied_fields(np.random.RandomState(nx), UNION_FIELDS, ny, nx, np.float64))[0]
    f = _once(("union", grid), make)
    return f if dtype == np.float64 else _once(("union", grid, "f32"), lambda: _frozen(f.astype(np.float32))[0])


def union_want(grid, dtype):
    key = ("union", grid, np.dtype(dtype).name)
    if key not in _want:
        _want[key] = _numpy_union(union_fields(grid, dtype), UNION_FIRST_INDEX)
    return _want[key]


def stride_fields(dtype):
    nx, ny = STRIDE_GRID
    return _once(("stride", np.dtype(dtype).name), lambda: _frozen(_tied_fields(np.random.RandomState(77), STRIDE_FIELDS, ny, nx, dtype))[0])


def padded(fields, pad):
    """The fields `cells + pad` elements apart in one flat array, +inf in every padding element (and behind the last field)."""
    n, cells = fields.shape[0], fields[0].size
    flat = np.full(n * (cells + pad), np.inf, fields.dtype)
    for k in range(n):
        flat[k * (cells + pad): k * (cells + pad) + cells] = fields[k].reshape(-1)
    return flat


# ---- D. the variant and offset sweeps above 1024 --------------------------------------------------------------------------------

VARIANT_THREADS = 1024          # csrc/vhp_capi.hip variant_launch_sweep / vhp_sweep_batch_offset: dim3(1024)
VARIANT_MAX_SIDE = 4096         # ... `std::max(nx, ny) > 4096`: VHP_ERR_TOO_LARGE
LDS_DEFAULT_LIMIT = 65536       # above it a launch needs hipFuncAttributeMaxDynamicSharedMemorySize (raise_lds_limit)
VARIANT_GRIDS = [(1500, 1100), (2729, 1030), (2730, 1030), (4096, 1100), (1100, 4096)]
VARIANT_PARAMS = [(1.0, 1.0), (0.995, 0.5)]   # (alpha, fac)
OFFSETS = [0.0, 1.0]


def variant_lds_bytes(nx, ny):
    """csrc/vhp_capi.hip variant_launch_sweep: `lds = 3 * (max(nx, ny) + 1) * sizeof(double)`"""
    return 3 * (max(nx, ny) + 1) * 8


def variant_case(nx, ny):
    """(occ, sources int32 [4, 2]): three corners and an interior cell, all free.  With a corner source one quadrant owns the whole
    grid, and its longest fronts are min(nx, ny) cells."""
    def make():
        occ = maps.random_rect_map(nx, ny, 25, 2, nx // 6, 2, ny // 6, nx + ny)
        src = np.array([(0, 0), (nx - 1, ny - 1), (nx - 1, 0), (nx // 3, ny // 2)], np.int32)
        for x, y in src:
            occ[y, x] = 1
        return _frozen(occ, src)
    return _once(("variant", nx, ny), make)


def too_large_maps():
    """One side past VARIANT_MAX_SIDE, either orientation: (occ, a free source)"""
    def make():
        out = []
        for nx, ny in ((VARIANT_MAX_SIDE + 1, 8), (8, VARIANT_MAX_SIDE + 1)):
            occ = maps.random_rect_map(nx, ny, 6, 2, max(nx // 8, 2), 2, max(ny // 8, 2), nx)
            occ[ny // 2, nx // 2] = 1
            out.append(_frozen(occ)[0])
        return out
    return _once("too_large", make)


# ---- E. the variant planner -----------------------------------------------------------------------------------------------------

def _free_pair(occ, seed):
    a, b = maps.free_sources(occ, 2, seed)
    return tuple(int(v) for v in a), tuple(int(v) for v in b)


def _planner_cases():
    cases = {}
    occ = maps.random_rect_map(203, 150, 14, 3, 30, 3, 30, 9)
    start, end = _free_pair(occ, 12)
    cases["203x150 thr 0.2"] = (occ, start, end, 0.2, 1.0, 60)
    cases["203x150 thr 0.5 alpha 0.98"] = (occ, start, end, 0.5, 0.98, 60)
    big = maps.random_rect_map(1100, 1040, 80, 20, 180, 20, 180, 5)
    start, end = _free_pair(big, 8)
    cases["1100x1040 max_iter 12"] = (big, start, end, 0.5, 0.998, 12)
    # tests/test_gpu_planner.py test_tie_break_symmetric_map's maps, start at the centre; the decay keeps the end out of sight
    sym = np.ones((65, 65), np.uint8)
    cases["symmetric open"] = (sym, (32, 32), (64, 64), 0.5, 0.97, 10)
    walls = sym.copy()
    walls[20:45, 40] = 0
    walls[40, 20:45] = 0
    cases["symmetric with walls"] = (walls, (32, 32), (64, 64), 0.5, 0.97, 20)
    # On a 65-wide map the mirror images about the diagonal are a multiple of 64 cells apart: the same lane of two wavefronts.  Two
    # maps that are symmetric about a column instead put the tied cells in two lanes: of two wavefronts, and of one (31 wide)
    bar = sym.copy()
    bar[45, 20:45] = 0
    cases["tie across wavefronts and lanes"] = (bar, (32, 32), (32, 64), 0.3, 0.97, 10)
    narrow = np.ones((65, 31), np.uint8)
    narrow[50, 11:20] = 0
    cases["tie across lanes"] = (narrow, (15, 32), (15, 64), 0.5, 0.97, 10)
    # a start whose 8 neighbours are blocked: one candidate, a degenerate scale
    boxed = np.ones((40, 56), np.uint8)
    boxed[9:12, 19:22] = 0
    boxed[10, 20] = 1
    cases["start walled in"] = (boxed, (20, 10), (50, 30), 0.3, 1.0, 10)
    # a wall across the whole map but for a gap: the start does not see the end
    gap = np.ones((60, 90), np.uint8)
    gap[:50, 45] = 0
    cases["max_iter 0"] = (gap, (5, 5), (85, 5), 0.5, 1.0, 0)
    cases["max_iter 2"] = (gap, (5, 5), (85, 5), 0.5, 0.9, 2)
    cases["end in plain sight"] = (gap, (5, 5), (30, 40), 0.5, 1.0, 10)
    cases["start is end"] = (gap, (70, 20), (70, 20), 0.5, 1.0, 10)
    cases["blocked start"] = (gap, (45, 10), (85, 5), 0.5, 1.0, 10)
    for c in cases.values():
        c[0].setflags(write=False)
    return cases


def planner_cases():
    """{name: (occ, start, end, threshold, alpha, max_iter)}"""
    return _once("planner", _planner_cases)


PLANNER_NAMES = ["203x150 thr 0.2", "203x150 thr 0.5 alpha 0.98", "1100x1040 max_iter 12", "symmetric open", "symmetric with walls",
                 "tie across wavefronts and lanes", "tie across lanes", "start walled in", "max_iter 0", "max_iter 2", "end in plain sight", "start is end", "blocked start"]
# what the oracle has to answer for the case to reach its branch (tests/test_side_kernel_shapes.py): status, waypoints (None: any)
PICK_THREADS = 1024   # csrc/vhp_capi.hip vhp_planner_solve_variant launches vhp_variant_pick with dim3(1024): cell k is thread k % 1024's
# (same wavefront, same lane) of the two cells tied for the first pick: the final scan, the whole reduction, the shuffles alone
PLANNER_TIES = {"symmetric with walls": (False, True), "tie across wavefronts and lanes": (False, False), "tie across lanes": (True, False)}
PLANNER_EXPECT = {"start walled in": (3, 1), "max_iter 0": (20, 2), "max_iter 2": (20, 4), "end in plain sight": (0, 1),
                  "start is end": (0, 1), "blocked start": (3, 1)}


def planner_want(oracle, name):
    if ("planner", name) not in _want:
        occ, start, end, thr, alpha, max_iter = planner_cases()[name]
        _want[("planner", name)] = oracle.solve_matlab(np.array(occ), start, end, thr, alpha, max_iter)
    return _want[("planner", name)]


def first_pick_minima(oracle, name):
    """Linear indices of the cells that attain the minimum of the first pick's heuristic (csrc/vhp_variant.hip.h vhp_variant_pick,
    oracle/vhp_oracle_matlab.cpp :122-147), from the oracle's first field: more than one is a tie the pick has to break."""
    occ, start, end, thr, alpha, _ = planner_cases()[name]
    ny, nx = occ.shape
    uni = oracle.sweep_matlab(np.array(occ), start[0], start[1], alpha, 1.0)
    y, x = np.mgrid[0:ny, 0:nx].astype(np.float64)
    dt = np.sqrt((x - end[0]) * (x - end[0]) + (y - end[1]) * (y - end[1])) + np.sqrt((x - start[0]) * (x - start[0]) + (y - start[1]) * (y - start[1]))
    cand = uni > thr
    vmin, vmax, dmin, dmax = uni[cand].min(), uni[cand].max(), dt[cand].min(), dt[cand].max()
    fun = np.where(cand, ((dmax - dmin) * (uni - vmin) / (vmax - vmin) + dmin) + dt, np.inf)
    return np.flatnonzero(fun.reshape(-1) == fun.min())
