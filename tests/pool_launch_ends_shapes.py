"""The batches of tests/test_gpu_pool_launch_ends.py and tests/test_pool_sim_launch_ends.py: the smallest at which the two ends of a
pool-sweep launch -- the order pre-kernel's records and the sweep kernel's first round -- take each of their paths on a 256-CU device
with three contexts per workgroup (the static round is on from 8 * n_sources = 3 * 256 units).  tests/test_launch_plans.py asks the
launcher's own plan (csrc/vhp_launch_plan.hpp plan_pool) whether each shape takes the path its comment claims."""
import numpy as np

import maps

# name: (n sources, nx, ny, sources outside the map)
SHAPES = {
    "96_static_round": (96, 136, 136, 0),     # 768 units = 3 contexts x 256 CUs: every context's first unit comes by workgroup index
    "95_all_pulled": (95, 136, 136, 0),       # one below: the static round is off, everything is pulled
    "9_fewer_units_than_groups": (9, 72, 40, 0),   # contexts that find no record
    "97_two_outside": (97, 136, 136, 2),      # records with -1 in the first round
    "96_anyw": (96, 130, 136, 0),             # the build for widths that are no multiple of 8, through the same prologue
}

_cache = {}


def batch(name):
    """(occ, sources int32 [n, 2], indices of the sources outside the map); the same arrays on every call."""
    if name not in _cache:
        n, nx, ny, n_out = SHAPES[name]
        occ = maps.random_rect_map(nx, ny, 10, 2, max(nx // 6, 3), 2, max(ny // 6, 3), nx * 5 + ny + n)
        src = maps.free_sources(occ, n, nx + n).copy()
        outside = []
        if n_out:
            src[5] = (nx, 3)      # one past the right edge
            src[n - 1] = (7, -1)  # above the first row
            outside = [5, n - 1]
        occ.setflags(write=False)
        src.setflags(write=False)
        _cache[name] = (occ, src, outside)
    return _cache[name]


_want = {}


def oracle_fields(oracle, name):
    """The oracle's fp64 fields of the batch's sources inside the map {index: field}, computed once."""
    if name not in _want:
        occ, src, outside = batch(name)
        _want[name] = {k: oracle.sweep_full(np.array(occ), int(sx), int(sy)) for k, (sx, sy) in enumerate(src) if k not in outside}
    return _want[name]
