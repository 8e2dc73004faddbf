"""The batches of tests/test_gpu_large_batches.py: more sources than one pass of a sweep's launch-order pre-kernel takes.

The pool sweep's vhp_pool_order orders up to 1024 sources (8192 units) in LDS (order_units_lds) and anything larger through global memory
(order_units); the front sweep's vhp_order_units has four units per source and 1024 threads, so 257 sources are its first second pass.
The grids are 136 wide or high on purpose: a unit has a boundary line -- a line base that a broken scan would get wrong -- only from two
strips of 64 rows on, and batch() asserts, through tests/pool_scratch_driver.cpp, that more than 1024 units of a batch have one.

Every batch of a grid is a prefix of the same source list (free cells, the four corners, some positions twice), so a grid's oracle
fields are computed once, per distinct source, and shared."""
import numpy as np

import maps
import pool_scratch_lib

N_MAX = 1031
GRIDS = {"w8": (136, 136), "anyw": (130, 136)}   # a width that is a multiple of 8, and one for the pool sweep's ANYW build
# pool batches: (sources, three of them outside the map)
POOL = {"1024_lds_full": (1024, False),        # 8192 units: the last size of order_units_lds, eight units a thread
        "1025_global": (1025, False),          # the first size of order_units
        "1031_three_outside": (1031, True)}    # records with -1 on the global path
ORDER_BODY = {name: "order_units_lds" if n * 8 <= 8192 else "order_units" for name, (n, _) in POOL.items()}

_cache = {}


def sources(grid):
    """(occ, N_MAX sources inside the map int32 [N_MAX, 2]); the same read-only arrays on every call."""
    if grid not in _cache:
        nx, ny = GRIDS[grid]
        occ = maps.random_rect_map(nx, ny, 10, 2, nx // 6, 2, ny // 6, 7 * nx + ny)
        src = maps.free_sources(occ, N_MAX, nx + 2 * ny).copy()
        # the corners: within the first 256, and one again as the first source past 1024
        src[3], src[40], src[200], src[250], src[1024] = (0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1), (nx - 1, ny - 1)
        # positions twice: neighbours, far apart, and either side of 1024
        src[7], src[255], src[1000], src[1026] = src[6], src[11], src[10], src[1023]
        occ.setflags(write=False)
        src.setflags(write=False)
        _cache[grid] = (occ, src)
    return _cache[grid]


def batch(grid, n, with_outside=False):
    """(occ, sources int32 [n, 2], indices of the sources outside the map)"""
    key = (grid, n, with_outside)
    if key not in _cache:
        nx, ny = GRIDS[grid]
        occ, all_src = sources(grid)
        src = all_src[:n].copy()
        outside = []
        if with_outside:
            src[5] = (nx, 3)         # one past the right edge
            src[600] = (-3, 20)      # a negative x
            src[n - 4] = (7, -1)     # above row 0
            outside = [5, 600, n - 4]
        if n >= 1024:
            bound, need, _, units, counted = pool_scratch_lib.lines_of_sources(nx, ny, src)
            assert counted == n and units > 1024, "%s, %d sources: only %d units have a boundary line" % (grid, n, units)
            assert 0 < need <= bound
        src.setflags(write=False)
        _cache[key] = (occ, src, outside)
    return _cache[key]


_want = {}


def oracle_fields(oracle, grid):
    """{(sx, sy): the oracle's fp64 field} for every source of the grid's list, computed once."""
    if grid not in _want:
        occ, src = sources(grid)
        occ = np.array(occ)
        _want[grid] = {xy: oracle.sweep_full(occ, xy[0], xy[1]) for xy in sorted({(int(x), int(y)) for x, y in src})}
        for f in _want[grid].values():
            f.setflags(write=False)
    return _want[grid]


# the stack of maps: 5 maps of 104 x 77, 1025 sources (4100 units of the front sweep: five passes of its pre-kernel)
MAPS_SHAPE = (5, 104, 77)
MAPS_SOURCES = 1025


def maps_batch():
    """(occ uint8 [5, 77, 104], sources int32 [1025, 2], map index int32 [1025])"""
    if "maps" not in _cache:
        m, nx, ny = MAPS_SHAPE
        occ = np.stack([maps.random_rect_map(nx, ny, 8, 2, nx // 5, 2, ny // 5, 31 + 17 * k) for k in range(m)])
        rng = maps.Lcg(5)
        src = np.array([(rng.below(nx), rng.below(ny)) for _ in range(MAPS_SOURCES)], np.int32)   # (free or blocked cells alike)
        idx = np.array([rng.below(m) for _ in range(MAPS_SOURCES)], np.int32)
        src[2], src[300], src[1023], src[1024] = (0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1)
        src[1001] = src[1000]   # the same position on another map
        idx[1000], idx[1001] = 1, 4
        for a in (occ, src, idx):
            a.setflags(write=False)
        _cache["maps"] = (occ, src, idx)
    return _cache["maps"]


def maps_oracle_fields(oracle):
    """{(map, sx, sy): the oracle's fp64 field} for the sources of maps_batch()"""
    if "maps" not in _want:
        occ, src, idx = maps_batch()
        keys = sorted({(int(k), int(x), int(y)) for (x, y), k in zip(src, idx)})
        _want["maps"] = {(k, x, y): oracle.sweep_full(np.array(occ[k]), x, y) for k, x, y in keys}
    return _want["maps"]
