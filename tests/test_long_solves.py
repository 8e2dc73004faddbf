"""What tests/long_solves.py says about its maps and solves, pinned with the CPU oracle alone -- no GPU.  The GPU tests of
test_gpu_long_solves.py reach the kernels' paths beyond 1024 pivots (and beyond 256 table entries) only because these numbers are what
they are: if a change to the generator or to the oracle moves a count below 1024, this file fails before a GPU test passes for the wrong
reason.
It also runs the stand-alone CPU drivers of the walk functions (tests/tree_driver.cpp, tests/paths_driver.cpp; plain and sanitized, as
test_tree_walk.py and test_paths_walk.py build them) on the oracle's tables of cases A and G."""
import struct
import zlib

import numpy as np
import pytest

import long_solves as ls
import test_paths_walk as pw
import test_tree_walk as tw


@pytest.mark.parametrize("name", sorted(ls.MAPS))
def test_maps(name):
    m = ls.MAPS[name]
    occ = ls.map_of(name)
    assert occ.shape == (m["ny"], m["nx"]) and occ.dtype == np.uint8
    assert zlib.crc32(occ.tobytes()) == m["crc"], "%s: crc32 %08x" % (name, zlib.crc32(occ.tobytes()))
    assert int(occ.sum()) == m["n_free"]
    assert all(occ[y, x] == 1 for x, y in m["free"])


def test_map_shapes_are_the_awkward_ones():
    assert ls.MAPS["M300"]["nx"] % 8 == 4                                    # a multiple of 8 less 4
    assert ls.MAPS["M301"]["nx"] % 2 == 1 and (301 * 277) % 2 == 1           # an odd width, an odd cell count
    assert (ls.MAPS["M301"]["nx"], ls.MAPS["M301"]["ny"]) == (ls.MAPS["M301b"]["nx"], ls.MAPS["M301b"]["ny"])   # one stack


@pytest.mark.parametrize("name", sorted(ls.CASES))
def test_cases(oracle, name):
    c = ls.CASES[name]
    r = ls.solve(oracle, name)
    came, piv = r["came_from"], r["pivots"]
    assert r["status"] == c["status"]
    assert r["n_pivots"] == c["n_pivots"] and len(piv) == c["n_pivots"] + 1
    assert len({(int(x), int(y)) for x, y in piv}) == c["distinct"]
    if name != "L":   # productive: every pivot is a new cell (the list's last entry, `end`, may repeat the last pivot)
        assert len({(int(x), int(y)) for x, y in piv[:-1]}) == c["n_pivots"] and c["distinct"] >= c["n_pivots"]
    lit = came[came != tw.UNL64]
    assert int(lit.max()) <= c["n_pivots"] - 1
    assert int((lit >= ls.LDS_PIVOTS).sum()) == c["beyond"]
    if c["at"] is not None:
        assert tuple(int((lit == t).sum()) for t in ls.AT_LABELS) == c["at"]
    if c["pivots_beyond"] is not None:
        assert int((ls.labels_of_pivots(r) >= ls.LDS_PIVOTS).sum()) == c["pivots_beyond"]
    ex, ey = c["end"]
    if c["status"] == ls.OK:
        assert came[ey, ex] != tw.UNL64
        if c["n_path"] is not None:
            d, path = oracle.reconstruct_path(came, piv, c["end"])
            assert len(path) == c["n_path"] and d > 0
            assert tuple(path[0]) == c["start"] and tuple(path[-1]) == c["end"]
    else:
        assert came[ey, ex] == tw.UNL64   # (the path calls say VHP_ERR_ARG there)


def test_what_the_gpu_tests_rely_on(oracle):
    """the notes of the case table: which cases cross which bound"""
    cases = ls.CASES
    assert all(cases[n]["at"][2] > 0 and cases[n]["at"][3] > 0 and cases[n]["at"][4] > 0 for n in ("B",)), "B holds labels 1023, 1024 and 1025"
    assert cases["B"]["n_pivots"] - ls.LDS_PIVOTS == 13
    for n in ("A", "C", "F", "G", "H"):   # the tree's parent chains run through entries beyond 1024, not only its leaves
        assert cases[n]["pivots_beyond"] >= 200
    for n in ("D", "I", "J", "K"):        # the controls: below 1024, above 256
        assert 256 < cases[n]["n_pivots"] < ls.LDS_PIVOTS and cases[n]["beyond"] == 0
    # the batch of test_gpu_long_solves.py ends its queries at four different iterations; at max_iter 1030 four are cut, D finishes
    assert sorted(cases[n]["n_pivots"] for n in "ACBD") == [736, 1037, 2507, 2833]
    for n in "BC":
        r = ls.solve(oracle, n, max_iter=1030)
        assert r["status"] == ls.MAX_ITER and r["n_pivots"] == 1031
        assert int(r["came_from"][r["came_from"] != tw.UNL64].max()) == 1030
    # the deepest path over all cells of A is no shorter than its end's
    r = ls.solve(oracle, "A")
    counts = _all_counts(tw_vhp(), r)
    assert int(counts.max()) >= cases["A"]["n_path"] == 215


def tw_vhp():
    import vhp_amd
    vhp_amd.build_library()
    vhp_amd.load_library()
    return vhp_amd


def _all_counts(vhp, r):
    """n_path of vhp_reconstruct_path from every cell (0 where it has none)"""
    import ctypes as C
    lib = vhp.load_library()
    came = np.ascontiguousarray(r["came_from"], np.uint64)
    piv = np.ascontiguousarray(r["pivots"], np.int32)
    ny, nx = came.shape
    out = np.zeros((ny, nx), np.uint32)
    n, d = C.c_uint32(0), C.c_double(0.0)
    pc, pp = came.ctypes.data_as(C.c_void_p), piv.ctypes.data_as(C.c_void_p)
    for y, x in np.argwhere(came != tw.UNL64):
        if lib.vhp_reconstruct_path(pc, pp, r["n_pivots"], nx, ny, int(x), int(y), None, 0, C.byref(n), C.byref(d)) == 0:
            out[y, x] = n.value
    return out


@pytest.fixture(scope="module")
def vhp():
    return tw_vhp()


@pytest.fixture(scope="module")
def tree_drivers(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("long_tree_driver"))
    return [tw.cpu_driver.build(tw.DRIVER, d, "tree_driver_" + name, flags=("-ffp-contract=off", "-O2"), includes=(tw.CSRC,), sanitized=san)
            for name, san in (("plain", False), ("san", True))]


@pytest.fixture(scope="module")
def paths_drivers(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("long_paths_driver"))
    return [pw.cpu_driver.build(pw.DRIVER, d, "paths_driver_" + name, flags=("-ffp-contract=off", "-O2"), includes=(pw.CSRC,), sanitized=san)
            for name, san in (("plain", False), ("san", True))]


def _beyond_goals(r, n, seed):
    """n cells to walk from in full: the end, pivots' cells labelled >= 1024 (the deepest chains), seeded labelled cells"""
    rng = np.random.default_rng(seed)
    piv = r["pivots"][: r["n_pivots"]]
    deep = piv[ls.labels_of_pivots(r) >= ls.LDS_PIVOTS]
    lit = np.argwhere(r["came_from"] != tw.UNL64)[:, ::-1]
    goals = [tuple(int(v) for v in r["pivots"][-1])]
    goals += [tuple(int(v) for v in deep[k]) for k in rng.integers(0, len(deep), n // 2)]
    goals += [tuple(int(v) for v in lit[k]) for k in rng.integers(0, len(lit), n - len(goals))]
    return goals


@pytest.mark.parametrize("name", ["A", "G"])
def test_tree_walk_on_long_tables(vhp, oracle, tree_drivers, name):
    """tree_build_tables / tree_cell / tree_goal_path (the bodies of vhp_tree.hip.h's kernels) on tables of 2834 and 1288 entries, every
    cell a goal: status, count and length bits of every cell (no path buffer: a buffer's 90 000 paths of ~100 points are text the
    drivers would print twice), and every point from 600 cells, half of them pivots' cells labelled >= 1024."""
    r = ls.solve(oracle, name)
    cap = r["n_pivots"] + 3
    goals = _beyond_goals(r, 600, 5)
    every, some = tw._compare(vhp, tree_drivers, [(r["came_from"], r["pivots"], tw.ALL, -1), (r["came_from"], r["pivots"], goals, cap)])
    # (40 % of a salt map is blocked and a solve stops when it sees its end: test_tree_walk's "half of all cells" cannot hold here)
    n_lit = int((r["came_from"] != tw.UNL64).sum())
    assert sum(1 for w in every if w[0] == tw.OK) == n_lit >= 9000 and sum(1 for w in every if w[1] >= 100) >= 2000
    ny, nx = r["came_from"].shape
    ex, ey = ls.CASES[name]["end"]
    assert every[ey * nx + ex][:2] == (tw.OK, ls.CASES[name]["n_path"])
    assert max(w[1] for w in every) >= ls.CASES[name]["n_path"]
    d, path = oracle.reconstruct_path(r["came_from"], r["pivots"], (ex, ey))
    assert some[0][0] == tw.OK and struct.unpack("<d", bytes.fromhex(some[0][2]))[0] == d and some[0][3] == path.reshape(-1).tolist()
    assert sum(1 for w in some if w[0] == tw.OK and w[1] >= 100) >= 100   # (long chains, walked point by point)


@pytest.mark.parametrize("name", ["A", "G"])
def test_paths_walk_on_long_tables(vhp, oracle, paths_drivers, name):
    """paths_parent_entry + the walk (the bodies of vhp_paths.hip.h's kernels) on the same tables.  The paths driver takes the whole
    label field once per goal, so every cell of a 300 x 300 grid would be 32 GB of input: 48 goals -- the end, pivots' cells
    labelled >= 1024, seeded labelled cells -- and, as a goal without a path, a blocked cell."""
    r = ls.solve(oracle, name)
    occ = ls.map_of(ls.CASES[name]["map"])
    cap = r["n_pivots"] + 3
    goals = _beyond_goals(r, 48, 6)
    by, bx = (int(v) for v in np.argwhere(occ == 0)[1000])
    tables = [(r["came_from"], r["pivots"], g, cap) for g in goals] + [(r["came_from"], r["pivots"], (bx, by), cap),
                                                                        (r["came_from"], r["pivots"], goals[0], 100),
                                                                        (r["came_from"], r["pivots"], goals[0], -1)]
    got = pw._compare(vhp, paths_drivers, tables)
    d, path = oracle.reconstruct_path(r["came_from"], r["pivots"], goals[0])
    st, n, bits, buf = got[0]
    assert st == pw.OK and n == ls.CASES[name]["n_path"] and struct.unpack("<d", bytes.fromhex(bits))[0] == d
    assert buf[: 2 * n] == path.reshape(-1).tolist() and set(buf[2 * n:]) <= {pw.SENTINEL}
    assert all(g[0] == pw.OK for g in got[: len(goals)]) and sum(g[1] >= 100 for g in got[: len(goals)]) >= 12
    assert got[len(goals)][:2] == (pw.ERR_ARG, 0)
    assert got[len(goals) + 1][:2] == (pw.ERR_TOO_LARGE, n) and got[len(goals) + 1][2] == bits
    assert got[len(goals) + 2][:3] == got[0][:3]
