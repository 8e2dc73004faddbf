"""The grids, maps and sources of the ray-cast tests (tests/test_raycast_cpu.py, tests/test_gpu_raycast.py), and raycasting()
(reference src/visibilityBasedSolver.cpp:267-290) restated in Python for the line-of-sight expectations."""
import numpy as np

import maps

# nx, ny, seed of the map.  The four tiny grids are drawn by hand (tiny_map); the others put the 64-cell boundary of the packed words
# on both axes and are seeded random rectangles at about 15 % density.
TINY = [(1, 1), (1, 7), (7, 1), (2, 2)]
RECT = [(63, 65, 2), (64, 64, 3), (65, 63, 5), (130, 67, 7)]
GRIDS = [(nx, ny, None) for nx, ny in TINY] + RECT


def tiny_map(nx, ny):
    """1 x 1: free.  The lines: one blocked cell inside, one at the far end (in plain sight, nothing behind it).  2 x 2: a blocked corner."""
    occ = np.ones((ny, nx), np.uint8)
    if nx * ny > 1:
        occ.reshape(-1)[[nx * ny // 2, nx * ny - 1]] = 0
    return occ


def rect_map(nx, ny, seed):
    n = max(1, nx * ny * 15 // 100 // 20)   # rectangles of 3..8 x 3..8, about 30 cells each, a third of them lost to overlap and clamping
    return maps.random_rect_map(nx, ny, n, 3, 8, 3, 8, seed)


def grid_map(nx, ny, seed):
    return tiny_map(nx, ny) if seed is None else rect_map(nx, ny, seed)


def sources_for(occ):
    """(x, y) list: the four corners, one cell on each edge, the centre, a free cell next to an obstacle and one blocked cell (where the
    map has them); no cell twice."""
    ny, nx = occ.shape
    out = [(0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1), (nx // 3, 0), (nx - 1, ny // 3), (2 * nx // 3, ny - 1), (0, 2 * ny // 3),
           (nx // 2, ny // 2)]
    blocked = np.argwhere(occ == 0)
    if len(blocked):
        for y, x in blocked:
            if x > 0 and occ[y, x - 1]:
                out.append((int(x) - 1, int(y)))
                break
        y, x = blocked[len(blocked) // 2]
        out.append((int(x), int(y)))
    seen = []
    for p in out:
        if p not in seen:
            seen.append(p)
    return seen


def ray(occ, x0, y0, x1, y1):
    """raycasting(x0, y0, x1, y1): the first blocked cell its loop meets, or None where it reaches the target."""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    sx = 1 if x0 < x1 else -1
    sy = 1 if y0 < y1 else -1
    err = dx - dy
    while x0 != x1 or y0 != y1:
        if occ[y0, x0] == 0:
            return (x0, y0)
        e2 = 2 * err
        if e2 > -dy:
            err -= dy
            x0 += sx
        if e2 < dx:
            err += dx
            y0 += sy
    return None


def hits_from(occ, sx, sy):
    """int32 [ny, nx, 2]: ray() from (sx, sy) to every cell, (-1, -1) where it is clear."""
    ny, nx = occ.shape
    out = np.full((ny, nx, 2), -1, np.int32)
    for y in range(ny):
        for x in range(nx):
            h = ray(occ, sx, sy, x, y)
            if h is not None:
                out[y, x] = h
    return out


def field_from_hits(hits):
    """The union relation: cell c is 0 exactly where the ray to c is blocked or c is the hit of some ray."""
    ny, nx, _ = hits.shape
    field = np.ones((ny, nx), np.float64)
    blocked = hits[..., 0] >= 0
    field[blocked] = 0.0
    field[hits[blocked][:, 1], hits[blocked][:, 0]] = 0.0
    return field
