"""The clearance field in numpy, for the tests of vhp_map_clearance / vhp_maps_clearance (test_clearance_cpu.py, test_gpu_clearance.py):
written out from the definition in include/vhp.h alone -- pad the blocked mask by more than any reach with the border's value, try
every offset of a box, keep the smallest metric that is at most p_max.  Nothing here knows of rows, packed words or distances along
a line: it is a statement of its own.  Sizes, maps and special cells are those of inflate_cases."""
import numpy as np

import inflate_cases as ic
from inflate_cases import DISC, SQUARE, DIAMOND, SIDES, case_maps, special_cells  # noqa: F401  (shared with the inflation's tests)

FAR = 0xFFFF
PAD = ic.MAX_INFLATE + 1   # one cell past any reach

# (shape, p_max): reach up to 3, every side of SIDES; reach 63 and 64, four size pairs each (test_clearance_cpu.py)
SMALL = ((DISC, 0), (DISC, 1), (DISC, 2), (DISC, 5), (DISC, 9), (SQUARE, 1), (SQUARE, 3), (DIAMOND, 1), (DIAMOND, 3))
LARGE = ((DISC, 3969), (DISC, 4096), (DISC, 4224), (SQUARE, 63), (SQUARE, 64), (DIAMOND, 64))
# the p at which (clearance > p) is held to the inflation, where p <= p_max; p_max itself is added
WITNESS_P = (0, 1, 2, 8, 9, 3969, 4096)


def metric(shape, dx, dy):
    """m(dx, dy) of include/vhp.h, on integers or integer arrays"""
    if shape == DISC:
        return dx * dx + dy * dy
    if shape == SQUARE:
        return np.maximum(np.abs(dx), np.abs(dy))
    if shape == DIAMOND:
        return np.abs(dx) + np.abs(dy)
    raise ValueError(shape)


def clearance(occ, shape, p_max, border=False):
    """uint8 [ny, nx] (!= 0 is free; leading axes are so many maps) -> uint16: per cell the smallest m(dx, dy) <= p_max over the
    blocked cells (x + dx, y + dy), cells outside the grid being free, or blocked with `border`; FAR where there is none."""
    occ = np.asarray(occ)
    ny, nx = occ.shape[-2:]
    # 0 where blocked, FAR where free: (cost | m) is then m on a blocked cell and FAR on a free one
    cost = np.full(occ.shape[:-2] + (ny + 2 * PAD, nx + 2 * PAD), 0 if border else FAR, np.uint16)
    cost[..., PAD:PAD + ny, PAD:PAD + nx] = np.where(occ == 0, 0, FAR)
    d = np.arange(-PAD, PAD + 1)
    dx, dy = np.meshgrid(d, d)
    m = metric(shape, dx, dy)
    inside = m <= p_max
    assert not inside[0].any() and not inside[-1].any() and not inside[:, 0].any() and not inside[:, -1].any(), "p_max beyond the box"
    out = np.full(occ.shape, FAR, np.uint16)
    for ox, oy, v in zip(dx[inside].tolist(), dy[inside].tolist(), m[inside].tolist()):
        np.minimum(out, cost[..., PAD + oy:PAD + oy + ny, PAD + ox:PAD + ox + nx] | np.uint16(v), out=out)
    return out


def witness_ps(shape, p_max):
    return sorted({p for p in WITNESS_P if p <= p_max} | {p_max})
