"""Inputs the sweeps are seldom given, shared by the GPU tests (tests/test_gpu_inputs.py) and the CPU simulators' tests: sources on
blocked cells, the same source more than once in a batch, maps that are all blocked, all free, or free only at the source."""
import numpy as np

import maps


def edge_map(nx, ny, seed):
    """A random map with the edge cases placed in it, and a batch that holds each of them: sources on a blocked corner, a blocked
    border cell, a blocked interior cell with free neighbours, a free cell walled in on all 8 sides (where the grid has room), and
    one source twice next to each other, a third time far away, another one twice far apart."""
    occ = maps.random_rect_map(nx, ny, max(3, min(30, nx * ny // 600)), 1, max(nx // 8, 2), 1, max(ny // 8, 2), seed)
    src = []
    occ[0, 0] = 0
    src.append((0, 0))                                   # blocked corner
    occ[ny - 1, nx // 2] = 0
    src.append((nx // 2, ny - 1))                        # blocked border cell
    if nx >= 8 and ny >= 8:
        cx, cy = nx // 2, ny // 2
        occ[cy - 1:cy + 2, cx - 1:cx + 2] = 1
        occ[cy, cx] = 0
        src.append((cx, cy))                             # blocked interior cell, free neighbours
        wx, wy = nx // 4, ny // 4
        occ[wy - 1:wy + 2, wx - 1:wx + 2] = 0
        occ[wy, wx] = 1
        src.append((wx, wy))                             # free cell walled in on all 8 sides
    a, b = [tuple(map(int, s)) for s in maps.free_sources(occ, 2, seed + 1)]
    src = [a, a] + src + [b, a, (nx - 1, 0), b]          # repeated: adjacent, far apart; 3 copies of a, 2 of b
    return occ, np.array(src, np.int32)


def whole_maps(nx, ny):
    """all blocked, all free, free only at the source: (name, map, batch)"""
    src = np.array([(nx // 3, ny // 2), (0, 0), (nx // 3, ny // 2), (nx - 1, ny - 1)], np.int32)
    lone = np.zeros((ny, nx), np.uint8)
    lone[ny // 2, nx // 3] = 1
    return [("all blocked", np.zeros((ny, nx), np.uint8), src), ("all free", np.ones((ny, nx), np.uint8), src),
            ("free only at the source", lone, src[[0, 0, 2]])]
