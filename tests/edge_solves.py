"""Planner solves at the grid's edge -- TEST INFRASTRUCTURE ONLY (numpy, no GPU).

Column 0 is swept only from a pivot with sx == 0 and row 0 only from one with sy == 0; the planner kernels keep cells a pivot
does not sweep out of the union, the labels and the heap with one predicate (csrc/vhp_planner_cell.hpp planner_unswept), which is all
that hides what an earlier pivot left there in a field that is not cleared between pivots.  That needs a pivot on row 0 or column 0
followed by one off it, which only a start on the border gives; push_rank's branch for empty quadrants needs a pivot on the border too.
Four groups of cases:
  T  tiny grids, all-free and with one blocked cell, every pair of free cells as (start, end): fewer cells than one workgroup has threads
  W  thin grids whose sides sit at the edges of the packed map's 64-bit words: 64, 65, 63, 129 by 1, 2 or 3
  B  productive solves (every pivot a new cell) from a corner of a salt map to the opposite corner; only the start (0, 0) sees its end,
     the other three corners are cut by max_iter because an end on row 0 / column 0 is never lit from off it
  Z  threshold 0.0 on a serpentine: `v >= 0` labels and pushes dark and blocked cells, and the pivots are blocked cells
MAPS, CASES and T_COUNTS hold what the oracle gives (tests/test_edge_solves.py pins every number with the oracle alone, so that no GPU
test goes vacuous); solve(oracle, name) is the oracle's result for a case, computed once per process."""
import functools

import numpy as np

OK, NOTHING_LIT, MAX_ITER = 0, 3, 20
UNL64 = 1000000000000000


def salt(nx, ny, seed, density, free=()):
    """uint8 [ny, nx], 1 = free: each cell blocked with probability `density`, then the cells (x, y) of `free` freed"""
    occ = (np.random.RandomState(seed).rand(ny, nx) >= density).astype(np.uint8)
    for x, y in free:
        occ[y, x] = 1
    return occ


def serpentine(nx, ny):
    """uint8 [ny, nx], 1 = free: every odd row a wall with one gap, at the last column and at column 0 in turn"""
    occ = np.ones((ny, nx), np.uint8)
    for y in range(1, ny, 2):
        occ[y, :] = 0
        occ[y, nx - 1 if (y // 2) % 2 == 0 else 0] = 1
    return occ


def corners(nx, ny):
    """the corner cells, each once"""
    return list(dict.fromkeys([(0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1)]))


def mid_borders(nx, ny):
    """the middle cell of the top, bottom, left and right border"""
    return [(nx // 2, 0), (nx // 2, ny - 1), (0, ny // 2), (nx - 1, ny // 2)]


def border_cells(nx, ny):
    """every cell of the grid's border, each once, row-major"""
    return [(x, y) for y in range(ny) for x in range(nx) if x in (0, nx - 1) or y in (0, ny - 1)]


# ---- group T

T_GRIDS = ((1, 1), (1, 2), (2, 1), (2, 2), (1, 7), (7, 1), (3, 3), (2, 9), (9, 2))   # (nx, ny)
T_PLAIN_GRIDS = T_GRIDS[:7]   # the plain solve runs these; the batch solves run all
T_THRESHOLDS = (0.0, 0.5)
T_MAX_ITER = 6


def t_maps(nx, ny):
    """the all-free grid, then each single cell blocked in turn: uint8 [nx * ny + 1, ny, nx]"""
    stack = np.ones((nx * ny + 1, ny, nx), np.uint8)
    for k in range(nx * ny):
        stack[k + 1].reshape(-1)[k] = 0
    return stack


def t_queries(occ):
    """every (start, end) pair of free cells, a cell with itself included, as (sx, sy, ex, ey), row-major in both"""
    ny, nx = occ.shape
    free = [(int(x), int(y)) for y, x in np.argwhere(occ == 1)]
    return [s + e for s in free for e in free]


# (nx, ny, threshold): queries, of them OK, OK after one pivot, cut by max_iter
T_COUNTS = {
    (1, 1, 0.0): (1, 1, 1, 0),
    (1, 1, 0.5): (1, 1, 1, 0),
    (1, 2, 0.0): (6, 5, 5, 1),
    (1, 2, 0.5): (6, 5, 5, 1),
    (2, 1, 0.0): (6, 5, 5, 1),
    (2, 1, 0.5): (6, 5, 5, 1),
    (2, 2, 0.0): (52, 31, 30, 21),
    (2, 2, 0.5): (52, 30, 30, 22),
    (1, 7, 0.0): (301, 210, 210, 91),
    (1, 7, 0.5): (301, 210, 210, 91),
    (7, 1, 0.0): (301, 210, 210, 91),
    (7, 1, 0.5): (301, 210, 210, 91),
    (3, 3, 0.0): (657, 395, 381, 262),
    (3, 3, 0.5): (657, 388, 368, 269),
    (2, 9, 0.0): (5526, 3461, 3446, 2065),
    (2, 9, 0.5): (5526, 3424, 3266, 2102),
    (9, 2, 0.0): (5526, 3461, 3397, 2065),
    (9, 2, 0.5): (5526, 3362, 3279, 2164),
}

# ---- groups W, B and Z

W_SIZES = ((64, 1), (1, 64), (65, 1), (1, 65), (63, 2), (2, 63), (65, 3), (3, 65), (129, 2))
# (nx, ny): free cells, zlib.crc32 of the uint8 bytes
W_PINS = {
    (64, 1): (44, 0xed3da4fd),
    (1, 64): (44, 0xed3da4fd),
    (65, 1): (45, 0x66e46c1e),
    (1, 65): (45, 0x66e46c1e),
    (63, 2): (90, 0xe10fb631),
    (2, 63): (90, 0xe10fb631),
    (65, 3): (138, 0x784c191a),
    (3, 65): (139, 0xf5fbc2bf),
    (129, 2): (189, 0x91751183),
}
W_DENSITY, W_SEED, W_MAX_ITER = 0.25, 1, 12

# name: how the map is made, free cells, zlib.crc32 of the uint8 bytes
MAPS = {
    "B130x9": dict(kind="salt", nx=130, ny=9, density=0.25, seed=1, n_free=877, crc=0x432aa56d),
    "B9x130": dict(kind="salt", nx=9, ny=130, density=0.25, seed=3, n_free=904, crc=0x5d8fbba4),
    "B65x13": dict(kind="salt", nx=65, ny=13, density=0.25, seed=1, n_free=635, crc=0xd00213ea),
    "B7x64": dict(kind="salt", nx=7, ny=64, density=0.25, seed=3, n_free=340, crc=0x8df77443),
    "B17x17": dict(kind="salt", nx=17, ny=17, density=0.40, seed=3, n_free=176, crc=0x2f16d8e3),
    "Z9x9": dict(kind="serpentine", nx=9, ny=9, n_free=49, crc=0xf1aa4d3f),
    "Z9x9t": dict(kind="serpentine_t", nx=9, ny=9, n_free=49, crc=0x68cc4392),
    "Z130x9": dict(kind="serpentine", nx=130, ny=9, n_free=654, crc=0xa7b6ac7a),
}
for _nx, _ny in W_SIZES:
    MAPS["W%dx%d" % (_nx, _ny)] = dict(kind="salt_w", nx=_nx, ny=_ny, density=W_DENSITY, seed=W_SEED, n_free=W_PINS[(_nx, _ny)][0],
                                       crc=W_PINS[(_nx, _ny)][1])


@functools.lru_cache(maxsize=None)
def map_of(name):
    """the named map, read-only"""
    m = MAPS[name]
    nx, ny = m["nx"], m["ny"]
    if m["kind"] == "salt":      # the corners freed
        occ = salt(nx, ny, m["seed"], m["density"], corners(nx, ny))
    elif m["kind"] == "salt_w":  # the corners and the mid-border cells freed
        occ = salt(nx, ny, m["seed"], m["density"], corners(nx, ny) + mid_borders(nx, ny))
    elif m["kind"] == "serpentine":
        occ = serpentine(nx, ny)
    else:
        occ = np.ascontiguousarray(serpentine(ny, nx).T)
    occ.setflags(write=False)
    return occ


B_THRESHOLD, B_MAX_ITER, B_MAX_ITER_CUT = 0.5, 200, 40   # (the start (0, 0) is case _0 of a map; the three other corners are cut)
Z_MAX_ITER = 40
C = MAX_ITER

# name (its map, then the query's number), start, end and what the oracle gives: status, n_pivots, distinct cells among the list's
# n_pivots + 1 entries, pivots 0 .. n_pivots - 1 on (x = 0, y = 0, x = nx - 1, y = ny - 1), blocked cells among the list's entries after
# the start (`end`, which closes the list of a solved query, left out).  W: threshold 0.5, max_iter 12; B: 0.5, 200 from (0, 0) and 40
# from the other corners; Z: 0.0, 40.
_ROWS = (
    ("W64x1_0", (0,0), (63,0), C, 13, 1, (13,13,0,13), 0),
    ("W64x1_1", (63,0), (0,0), C, 13, 1, (0,13,13,13), 0),
    ("W64x1_2", (32,0), (32,0), OK, 1, 1, (0,1,0,1), 0),
    ("W1x64_0", (0,0), (0,63), C, 13, 1, (13,13,13,0), 0),
    ("W1x64_1", (0,63), (0,0), C, 13, 1, (13,0,13,13), 0),
    ("W1x64_2", (0,32), (0,32), OK, 1, 1, (1,0,1,0), 0),
    ("W65x1_0", (0,0), (64,0), C, 13, 1, (13,13,0,13), 0),
    ("W65x1_1", (64,0), (0,0), C, 13, 1, (0,13,13,13), 0),
    ("W65x1_2", (32,0), (32,0), OK, 1, 1, (0,1,0,1), 0),
    ("W1x65_0", (0,0), (0,64), C, 13, 1, (13,13,13,0), 0),
    ("W1x65_1", (0,64), (0,0), C, 13, 1, (13,0,13,13), 0),
    ("W1x65_2", (0,32), (0,32), OK, 1, 1, (1,0,1,0), 0),
    ("W63x2_0", (0,0), (62,1), C, 13, 3, (1,1,0,12), 0),
    ("W63x2_1", (62,0), (0,1), C, 13, 1, (0,13,13,0), 0),
    ("W63x2_2", (0,1), (62,0), C, 13, 1, (13,0,0,13), 0),
    ("W63x2_3", (62,1), (0,0), C, 13, 1, (0,0,13,13), 0),
    ("W63x2_4", (31,0), (31,1), OK, 1, 2, (0,1,0,0), 0),
    ("W63x2_5", (31,1), (31,0), C, 13, 1, (0,0,0,13), 0),
    ("W63x2_6", (0,1), (62,1), C, 13, 1, (13,0,0,13), 0),
    ("W63x2_7", (62,1), (0,1), C, 13, 1, (0,0,13,13), 0),
    ("W2x63_0", (0,0), (1,62), C, 13, 1, (13,13,0,0), 0),
    ("W2x63_1", (1,0), (0,62), C, 13, 1, (0,13,13,0), 0),
    ("W2x63_2", (0,62), (1,0), C, 13, 1, (13,0,0,13), 0),
    ("W2x63_3", (1,62), (0,0), C, 13, 1, (0,0,13,13), 0),
    ("W2x63_4", (1,0), (1,62), C, 13, 1, (0,13,13,0), 0),
    ("W2x63_5", (1,62), (1,0), C, 13, 1, (0,0,13,13), 0),
    ("W2x63_6", (0,31), (1,31), OK, 1, 2, (1,0,0,0), 0),
    ("W2x63_7", (1,31), (0,31), C, 13, 1, (0,0,13,0), 0),
    ("W65x3_0", (0,0), (64,2), C, 13, 5, (1,1,0,10), 0),
    ("W65x3_1", (64,0), (0,2), C, 13, 5, (0,1,1,11), 0),
    ("W65x3_2", (0,2), (64,0), C, 13, 3, (1,0,0,12), 0),
    ("W65x3_3", (64,2), (0,0), C, 13, 4, (0,0,1,2), 0),
    ("W65x3_4", (32,0), (32,2), OK, 1, 2, (0,1,0,0), 0),
    ("W65x3_5", (32,2), (32,0), C, 13, 5, (0,0,0,2), 0),
    ("W65x3_6", (0,1), (64,1), C, 13, 1, (13,0,0,0), 0),
    ("W65x3_7", (64,1), (0,1), C, 13, 1, (0,0,13,0), 0),
    ("W3x65_0", (0,0), (2,64), C, 13, 5, (1,1,10,0), 0),
    ("W3x65_1", (2,0), (0,64), C, 13, 1, (0,13,13,0), 0),
    ("W3x65_2", (0,64), (2,0), C, 13, 5, (1,0,10,1), 0),
    ("W3x65_3", (2,64), (0,0), C, 13, 4, (0,0,12,1), 0),
    ("W3x65_4", (1,0), (1,64), C, 13, 1, (0,13,0,0), 0),
    ("W3x65_5", (1,64), (1,0), C, 13, 3, (0,0,12,1), 0),
    ("W3x65_6", (0,32), (2,32), OK, 1, 2, (1,0,0,0), 0),
    ("W3x65_7", (2,32), (0,32), C, 13, 3, (0,0,1,0), 0),
    ("W129x2_0", (0,0), (128,1), C, 13, 2, (1,1,0,12), 0),
    ("W129x2_1", (128,0), (0,1), C, 13, 2, (0,1,1,12), 0),
    ("W129x2_2", (0,1), (128,0), C, 13, 1, (13,0,0,13), 0),
    ("W129x2_3", (128,1), (0,0), C, 13, 1, (0,0,13,13), 0),
    ("W129x2_4", (64,0), (64,1), OK, 1, 2, (0,1,0,0), 0),
    ("W129x2_5", (64,1), (64,0), C, 13, 1, (0,0,0,13), 0),
    ("W129x2_6", (0,1), (128,1), C, 13, 1, (13,0,0,13), 0),
    ("W129x2_7", (128,1), (0,1), C, 13, 1, (0,0,13,13), 0),
    ("B130x9_0", (0,0), (129,8), OK, 47, 48, (1,1,0,5), 0),
    ("B130x9_1", (129,0), (0,8), C, 41, 42, (0,1,1,3), 0),
    ("B130x9_2", (0,8), (129,0), C, 41, 42, (1,0,0,4), 0),
    ("B130x9_3", (129,8), (0,0), C, 41, 42, (0,0,1,3), 0),
    ("B9x130_0", (0,0), (8,129), OK, 57, 58, (1,1,4,1), 0),
    ("B9x130_1", (8,0), (0,129), C, 41, 16, (0,1,2,0), 0),
    ("B9x130_2", (0,129), (8,0), C, 41, 42, (1,0,3,1), 0),
    ("B9x130_3", (8,129), (0,0), C, 41, 42, (0,0,3,2), 0),
    ("B65x13_0", (0,0), (64,12), OK, 30, 31, (1,1,1,2), 0),
    ("B65x13_1", (64,0), (0,12), C, 41, 42, (0,1,1,2), 0),
    ("B65x13_2", (0,12), (64,0), C, 41, 42, (1,0,1,3), 0),
    ("B65x13_3", (64,12), (0,0), C, 41, 42, (0,0,2,2), 0),
    ("B7x64_0", (0,0), (6,63), OK, 31, 32, (1,1,8,0), 0),
    ("B7x64_1", (6,0), (0,63), C, 41, 16, (0,1,2,0), 0),
    ("B7x64_2", (0,63), (6,0), C, 41, 29, (1,0,19,1), 0),
    ("B7x64_3", (6,63), (0,0), C, 41, 14, (0,0,1,1), 0),
    ("B17x17_0", (0,0), (16,16), OK, 15, 15, (1,1,3,1), 0),
    ("B17x17_1", (16,0), (0,16), C, 41, 18, (0,1,1,25), 0),
    ("B17x17_2", (0,16), (16,0), C, 41, 15, (1,0,0,1), 0),
    ("B17x17_3", (16,16), (0,0), C, 41, 10, (0,0,2,3), 0),
    ("Z9x9_0", (0,0), (8,0), OK, 1, 2, (1,1,0,0), 0),
    ("Z9x9_1", (0,0), (0,8), C, 41, 2, (41,1,0,0), 41),
    ("Z9x9_2", (0,0), (8,8), C, 41, 3, (1,1,0,0), 40),
    ("Z9x9_3", (8,0), (0,0), C, 41, 2, (0,1,1,0), 41),
    ("Z9x9_4", (8,0), (0,8), C, 41, 3, (0,1,1,0), 40),
    ("Z9x9_5", (8,0), (8,8), C, 41, 2, (0,1,41,0), 41),
    ("Z9x9_6", (0,8), (0,0), C, 41, 2, (41,0,0,1), 41),
    ("Z9x9_7", (0,8), (8,0), C, 41, 3, (1,0,0,1), 40),
    ("Z9x9_8", (0,8), (8,8), OK, 1, 2, (1,0,0,1), 0),
    ("Z9x9_9", (8,8), (0,0), C, 41, 3, (0,0,1,1), 40),
    ("Z9x9_10", (8,8), (8,0), C, 41, 2, (0,0,41,1), 41),
    ("Z9x9_11", (8,8), (0,8), C, 41, 2, (0,0,1,1), 41),
    ("Z9x9t_0", (0,0), (8,0), C, 41, 2, (1,41,0,0), 41),
    ("Z9x9t_1", (0,0), (0,8), OK, 1, 2, (1,1,0,0), 0),
    ("Z9x9t_2", (0,0), (8,8), C, 41, 3, (1,1,0,0), 40),
    ("Z9x9t_3", (8,0), (0,0), C, 41, 2, (0,41,1,0), 41),
    ("Z9x9t_4", (8,0), (0,8), C, 41, 2, (0,1,1,0), 41),
    ("Z9x9t_5", (8,0), (8,8), OK, 1, 2, (0,1,1,0), 0),
    ("Z9x9t_6", (0,8), (0,0), C, 41, 2, (1,0,0,1), 41),
    ("Z9x9t_7", (0,8), (8,0), C, 41, 2, (1,0,0,1), 41),
    ("Z9x9t_8", (0,8), (8,8), C, 41, 2, (1,0,0,41), 41),
    ("Z9x9t_9", (8,8), (0,0), C, 41, 3, (0,0,1,1), 40),
    ("Z9x9t_10", (8,8), (8,0), C, 41, 2, (0,0,1,1), 41),
    ("Z9x9t_11", (8,8), (0,8), C, 41, 2, (0,0,1,41), 41),
    ("Z130x9_0", (0,0), (129,8), OK, 2, 2, (1,1,1,1), 0),
)


def _case(row):
    name, start, end, status, n_pivots, distinct, border, blocked = row
    group, first = name[0], name.endswith("_0")
    thr = 0.0 if group == "Z" else B_THRESHOLD
    max_iter = W_MAX_ITER if group == "W" else Z_MAX_ITER if group == "Z" else B_MAX_ITER if first else B_MAX_ITER_CUT
    return dict(map=name.rsplit("_", 1)[0], start=start, end=end, thr=thr, max_iter=max_iter, status=status, n_pivots=n_pivots,
                distinct=distinct, border=border, blocked=blocked)


CASES = {row[0]: _case(row) for row in _ROWS}


def _opposite(nx, ny, p):
    return (nx - 1 - p[0], ny - 1 - p[1])


def w_queries(nx, ny):
    """from every corner to the opposite one, from mid-border to mid-border both ways, each once"""
    m = mid_borders(nx, ny)
    qs = [(s, _opposite(nx, ny, s)) for s in corners(nx, ny)] + [(m[0], m[1]), (m[1], m[0]), (m[2], m[3]), (m[3], m[2])]
    return list(dict.fromkeys(qs))


def case_names(group):
    """the cases of group "W", "B" or "Z", in the table's order"""
    return [n for n in CASES if n.startswith(group)]


def query(name):
    """(start_x, start_y, end_x, end_y) of a case"""
    c = CASES[name]
    return tuple(c["start"]) + tuple(c["end"])


_solves = {}


def solve_on(oracle, occ, start, end, threshold, max_iter):
    """the oracle's solve of a query on a map, its arrays read-only, computed once per process"""
    key = (occ.shape, occ.tobytes(), tuple(start), tuple(end), float(threshold), int(max_iter))
    if key not in _solves:
        r = oracle.solve(np.ascontiguousarray(occ), key[2], key[3], key[4], key[5])
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _solves[key] = r
    return _solves[key]


def solve(oracle, name):
    """the oracle's result for a case of W, B or Z"""
    c = CASES[name]
    return solve_on(oracle, map_of(c["map"]), c["start"], c["end"], c["thr"], c["max_iter"])


def border_counts(r):
    """pivots 0 .. n_pivots - 1 (the list's last entry is no pivot: it was not swept) on x = 0, y = 0, x = nx - 1, y = ny - 1"""
    ny, nx = r["came_from"].shape
    piv = r["pivots"][: r["n_pivots"]]
    return (int((piv[:, 0] == 0).sum()), int((piv[:, 1] == 0).sum()), int((piv[:, 0] == nx - 1).sum()), int((piv[:, 1] == ny - 1).sum()))
