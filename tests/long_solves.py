"""Planner solves of 300 to 2800 pivots -- TEST INFRASTRUCTURE ONLY (numpy, no GPU).

Every planner kernel that reads the pivot list takes another path beyond a fixed pivot count: the epilogues stage pivots 0..1023 in LDS
and read the rest from global memory, vhp_tree_fields stages tables below 1024 pivots and reads larger ones through L2, vhp_tree_tables'
loops repeat past 256 entries and vhp_paths_parents takes a second block past 256.  A live-lock repeats one pivot and lights no new
cell, so its labels stay tiny however large max_iter is; the solves here are productive instead.  The maps are random "salt" (each
cell blocked with probability 0.40), solved at threshold 0.5: every pivot is a new cell and labels run up to n_pivots - 1.

MAPS and CASES hold what the oracle gives for them (tests/test_long_solves.py pins every number with the oracle alone, so that no GPU
test goes vacuous); solve(oracle, name) is the oracle's result for a case, computed once per process."""
import functools

import numpy as np

THRESHOLD = 0.5
DENSITY = 0.40
OK, MAX_ITER = 0, 20
LDS_PIVOTS = 1024   # kPivLds of the epilogues, kTreeLdsPivots of vhp_tree_fields

_FREE_300 = ((1, 1), (298, 298), (150, 150), (1, 150), (298, 150), (298, 1), (1, 298))
_FREE_301 = ((1, 1), (299, 275), (299, 138), (299, 1), (1, 275), (1, 138), (150, 1), (150, 275))

# name: nx, ny, seed, cells freed after the draw (one map serves all its queries), free cells, zlib.crc32 of the uint8 bytes
MAPS = {
    "M300": dict(nx=300, ny=300, seed=3, free=_FREE_300, n_free=54029, crc=0x5bfbb225),    # a multiple of 8 less 4
    "M301": dict(nx=301, ny=277, seed=3, free=_FREE_301, n_free=50078, crc=0xdeee6c39),    # odd in both sides
    "M301b": dict(nx=301, ny=277, seed=5, free=_FREE_301, n_free=50270, crc=0x9959a498),
}

# name: map, start, end, max_iter and what the oracle gives: status, n_pivots, distinct cells among the list's n_pivots + 1 entries (all
# of them in a productive solve, but in H, I and J the last pivot is `end` itself, which closes the list once more), cells labelled
# >= 1024, cells labelled 255 / 256 / 1023 / 1024 / 1025 (None: not pinned), pivots whose own cell's label is >= 1024 (None: not pinned),
# points of the path from `end` (None: none, or not pinned)
CASES = {
    "A": dict(map="M300", start=(1, 1), end=(298, 298), max_iter=3000, status=OK, n_pivots=2833, distinct=2834, beyond=10225,
              at=(14, 9, 13, 9, 0), pivots_beyond=1623, n_path=215),
    "B": dict(map="M300", start=(298, 298), end=(1, 1), max_iter=3000, status=OK, n_pivots=1037, distinct=1038, beyond=112,
              at=(5, 9, 1, 6, 6), pivots_beyond=12, n_path=223),
    "C": dict(map="M300", start=(150, 150), end=(298, 298), max_iter=3000, status=OK, n_pivots=2507, distinct=2508, beyond=8728,
              at=(6, 4, 7, 0, 5), pivots_beyond=1336, n_path=107),
    "D": dict(map="M300", start=(1, 150), end=(298, 150), max_iter=3000, status=OK, n_pivots=736, distinct=737, beyond=0,
              at=(1, 2, 0, 0, 0), pivots_beyond=0, n_path=215),
    "E": dict(map="M300", start=(1, 1), end=(298, 298), max_iter=1030, status=MAX_ITER, n_pivots=1031, distinct=1032, beyond=18,
              at=(14, 9, 13, 9, 0), pivots_beyond=1, n_path=None),
    "F": dict(map="M300", start=(1, 1), end=(150, 150), max_iter=1500, status=MAX_ITER, n_pivots=1501, distinct=1502, beyond=3028,
              at=(16, 7, 1, 1, 15), pivots_beyond=420, n_path=None),
    "L": dict(map="M300", start=(298, 1), end=(1, 298), max_iter=300, status=MAX_ITER, n_pivots=301, distinct=5, beyond=0,
              at=None, pivots_beyond=0, n_path=None),   # a live-lock
    "G": dict(map="M301", start=(299, 275), end=(1, 1), max_iter=3000, status=OK, n_pivots=1287, distinct=1288, beyond=1607,
              at=(0, 19, 7, 7, 1), pivots_beyond=247, n_path=256),
    "H": dict(map="M301", start=(1, 1), end=(299, 138), max_iter=3000, status=OK, n_pivots=1501, distinct=1501, beyond=3147,
              at=(2, 22, 11, 1, 13), pivots_beyond=441, n_path=236),
    "I": dict(map="M301", start=(299, 1), end=(1, 275), max_iter=3000, status=OK, n_pivots=681, distinct=681, beyond=0,
              at=(6, 1, 0, 0, 0), pivots_beyond=0, n_path=196),
    "J": dict(map="M301", start=(1, 138), end=(299, 138), max_iter=3000, status=OK, n_pivots=982, distinct=982, beyond=0,
              at=None, pivots_beyond=0, n_path=183),
    "K": dict(map="M301b", start=(1, 1), end=(299, 275), max_iter=1600, status=OK, n_pivots=983, distinct=984, beyond=0,
              at=None, pivots_beyond=0, n_path=None),
    "N": dict(map="M301b", start=(299, 275), end=(1, 1), max_iter=1600, status=MAX_ITER, n_pivots=1601, distinct=1602, beyond=3226,
              at=None, pivots_beyond=None, n_path=None),
}
AT_LABELS = (255, 256, 1023, 1024, 1025)


def salt(nx, ny, seed, free=()):
    """uint8 [ny, nx], 1 = free: each cell blocked with probability DENSITY, then the cells (x, y) of `free` freed"""
    occ = (np.random.RandomState(seed).rand(ny, nx) >= DENSITY).astype(np.uint8)
    for x, y in free:
        occ[y, x] = 1
    return occ


@functools.lru_cache(maxsize=None)
def map_of(name):
    """the named map, read-only"""
    m = MAPS[name]
    occ = salt(m["nx"], m["ny"], m["seed"], m["free"])
    occ.setflags(write=False)
    return occ


def query(name):
    """(start_x, start_y, end_x, end_y) of a case"""
    c = CASES[name]
    return tuple(c["start"]) + tuple(c["end"])


_solves = {}


def solve_at(oracle, map_name, start, end, max_iter):
    """the oracle's solve of a query on a named map at THRESHOLD, its arrays read-only, computed once per process"""
    key = (map_name, tuple(start), tuple(end), int(max_iter))
    if key not in _solves:
        r = oracle.solve(map_of(map_name), key[1], key[2], THRESHOLD, key[3])
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _solves[key] = r
    return _solves[key]


def solve(oracle, name, max_iter=None):
    """the oracle's result for a case (max_iter: the case's query under another iteration cap), computed once per process"""
    c = CASES[name]
    return solve_at(oracle, c["map"], c["start"], c["end"], c["max_iter"] if max_iter is None else max_iter)


def labels_of_pivots(r):
    """uint64 [n_pivots]: the label of the own cell of each of pivots 0 .. n_pivots - 1 (the list's last entry is `end`, no pivot)"""
    piv = r["pivots"][: r["n_pivots"]]
    return r["came_from"][piv[:, 1], piv[:, 0]]


def first_pivot_difference(got, want):
    """index of the first entry at which two pivot lists differ (the shorter one's length if one is a prefix of the other), None if
    they are the same: a solve that diverges differs everywhere after that point"""
    a, b = np.asarray(got).reshape(-1, 2), np.asarray(want).reshape(-1, 2)
    n = min(len(a), len(b))
    bad = np.flatnonzero((a[:n] != b[:n]).any(axis=1))
    if bad.size:
        return int(bad[0])
    return None if len(a) == len(b) else n
