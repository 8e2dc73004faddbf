"""Maps whose fields are hard on the value-dependent parts of the sweep kernels -- TEST INFRASTRUCTURE ONLY (numpy, no GPU).

Rectangle and salt maps give fields of 1, 0 and a narrow penumbra.  The maps here give the rest:

  corridor_star   one-cell-wide diagonal corridors at offset i - j = k from the source, walled on i - j = k +- 1, in all eight
                  octants.  The stencil a - c (a - b) has a = 0 in every corridor cell, so the corridor's value is multiplied by
                  c = j / i at every step and falls like 1 / C(i, j): tiny, then fp32-subnormal, then below fp32 altogether, then
                  fp64-subnormal, then an exact +0.0 by arithmetic alone.  A strip of a latency or band sweep that holds such a
                  corridor dies by decay, not behind a blocked cell.
  dot_lattice     single blocked cells on a lattice: almost every lit cell fractional, tens of thousands of them at or below the
                  queue variant's 0.001 cut-off.
  salt_walled     random blocked cells plus a few full walls: light that dies early behind blocked cells.

CASES names the (map, sources) pairs the tests share (tests/test_hard_maps.py: what each of them has to contain, checked with the
oracle alone; tests/test_gpu_hard_maps.py: every kernel on them); fields(oracle, name) is the oracle's answer, computed once."""
import functools

import numpy as np


def corridor_star(nx, ny, sx, sy, ks):
    """uint8 [ny, nx], 1 = free: for every k of ks the walls i - j = k - 1 and i - j = k + 1 (j >= 1) of the corridor i - j = k, in each
    of the eight octants around (sx, sy).  k = 1: one wall is the octant's own diagonal beyond the source (the stale diagonal, SURVEY
    Q1, next to a wall)."""
    occ = np.ones((ny, nx), np.uint8)
    for k in ks:
        for i in range(k, max(nx, ny)):
            for d in (k - 1, k + 1):
                j = i - d
                if j < 1:
                    continue
                for dx in (-1, 1):
                    for dy in (-1, 1):
                        for a, b in ((i, j), (j, i)):
                            x, y = sx + dx * a, sy + dy * b
                            if 0 <= x < nx and 0 <= y < ny:
                                occ[y, x] = 0
    occ[sy, sx] = 1
    return occ


def dot_lattice(nx, ny, px, py):
    """uint8 [ny, nx], all free but one blocked cell per px x py cells"""
    occ = np.ones((ny, nx), np.uint8)
    occ[py // 2::py, px // 2::px] = 0
    return occ


def salt_walled(nx, ny, seed, density):
    """A map where light dies early: random cells blocked with the given density, plus a few full walls."""
    rng = np.random.RandomState(seed)
    occ = (rng.rand(ny, nx) >= density).astype(np.uint8)
    for k in range(3):
        occ[rng.randint(0, ny), :] = 0
        occ[:, rng.randint(0, nx)] = 0
    return occ


# name: (generator, its arguments, the first source)
_SPECS = {
    "star401": (corridor_star, (401, 401, 200, 200, (40,)), (200, 200)),
    "star400x363": (corridor_star, (400, 363, 200, 180, (40,)), (200, 180)),
    "star328_lo": (corridor_star, (328, 300, 1, 1, (100,)), (1, 1)),
    "star328_hi": (corridor_star, (328, 300, 326, 298, (100,)), (326, 298)),
    "star_q1": (corridor_star, (264, 200, 130, 100, (1, 4, 30)), (130, 100)),
    # above 1024: the latency sweep deals an octant's bands to several workgroups and passes death through the global record
    "star1304": (corridor_star, (1304, 1203, 1, 1, (600,)), (1, 1)),
    "star1200": (corridor_star, (1200, 1200, 0, 0, (560,)), (0, 0)),
    "dots2x2": (dot_lattice, (328, 300, 2, 2), (160, 150)),
    "dots3x5": (dot_lattice, (328, 300, 3, 5), (160, 150)),
    "dots7x4": (dot_lattice, (328, 300, 7, 4), (160, 150)),
    "dots2x2_333": (dot_lattice, (333, 301, 2, 2), (160, 150)),
    "dots3x5_333": (dot_lattice, (333, 301, 3, 5), (160, 150)),
    "dots7x4_333": (dot_lattice, (333, 301, 7, 4), (160, 150)),
    "salt333": (salt_walled, (333, 301, 7, 0.15), (166, 150)),
}
CASE_NAMES = tuple(_SPECS)


@functools.lru_cache(maxsize=None)
def case(name):
    """(occ uint8 [ny, nx], sources int32 [n, 2]) of a named case, both read-only.  The first source is the star's centre (the lattice's
    and the salt map's: a cell near the middle); the others see the map as just an awkward map: the four corners, the first source
    + (7, -3) clipped to the grid, and (nx // 2, 0).  Every source cell is free."""
    make, args, (sx, sy) = _SPECS[name]
    occ = make(*args)
    ny, nx = occ.shape
    src = [(sx, sy), (0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1), (min(max(sx + 7, 0), nx - 1), min(max(sy - 3, 0), ny - 1)), (nx // 2, 0)]
    src = np.array(list(dict.fromkeys(src)), np.int32)   # (a centre in a corner is listed once)
    occ[src[:, 1], src[:, 0]] = 1
    occ.setflags(write=False)
    src.setflags(write=False)
    return occ, src


def __getattr__(name):
    if name == "CASES":   # the named list of (occ, sources), built when first asked for
        return [(n,) + case(n) for n in CASE_NAMES]
    raise AttributeError(name)


_fields = {}


def fields(oracle, name):
    """float64 [n, ny, nx], read-only: the oracle's field of every source of a case, computed once per process"""
    if name not in _fields:
        occ, src = case(name)
        f = np.stack([oracle.sweep_full(occ, int(x), int(y)) for x, y in src])
        f.setflags(write=False)
        _fields[name] = f
    return _fields[name]
