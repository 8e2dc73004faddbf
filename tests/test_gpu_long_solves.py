"""Planner solves of 1000 to 2800 pivots through every kernel that reads the pivot list (tests/long_solves.py: the maps and cases,
tests/test_long_solves.py: what the oracle gives for them).  Beyond 1024 pivots the epilogues of the plain, batch and speculative
solves take a lit cell's parent from global memory instead of LDS and vhp_tree_fields reads its tables through L2; beyond 256 table
entries the loops of vhp_tree_tables repeat and vhp_paths_parents runs more than one block.  The other planner tests end after 251
pivots at most.
Every exact solve is compared with the CPU oracle byte for byte (test_gpu_planner._assert_same_solution); a failure also names the
first pivot that differs, since a solve that diverges differs everywhere after that point.  The speculative solve's fast mode is held
to test_gpu_speculative's validity checks, the path and tree calls to test_gpu_planner_paths' and test_gpu_planner_tree's."""
import ctypes as C

import numpy as np
import pytest

import long_solves as ls
from test_gpu_planner import _assert_same_solution
from test_gpu_planner_paths import _bits, _old_route
from test_gpu_planner_paths import _check as _check_paths
from test_gpu_planner_tree import KINDS, _against_oracle_walk, _check_fields, _check_goals, _fields_device, _goals_device, _same as _same_fields
from test_gpu_speculative import _check_valid_plan, _union_of_the_pivots_fields

pytestmark = pytest.mark.gpu

THR = ls.THRESHOLD
UNL32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def vhp():
    import torch  # noqa: F401
    import vhp_amd
    return vhp_amd


def _ctx(vhp, map_name):
    c = vhp.Context(0)
    c.set_map(ls.map_of(map_name))
    return c


def _same(got, want, what):
    """_assert_same_solution; a failure also says which pivot first differs"""
    try:
        _assert_same_solution(got, want, what)
    except AssertionError as e:
        k = ls.first_pivot_difference(got["pivots"], want["pivots"])
        where = "the pivot lists agree" if k is None else "first differing pivot: index %d of %d" % (k, want["n_pivots"])
        raise AssertionError("%s [%s]" % (e, where)) from None


def _labels32(came):
    return np.where(came >= np.uint64(UNL32), np.uint64(UNL32), came).astype(np.uint32)


def _fetch(p, shape, dtype):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    a = np.empty(shape, dtype)
    assert hip.hipMemcpy(a.ctypes.data, p, a.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return a


def _device_results_equal(ptr, want, what):
    """the four device arrays of a results_device call against the oracle's solve"""
    ny, nx = want["came_from"].shape
    lab = _fetch(ptr["labels"], (ny, nx), np.uint32)
    assert lab.tobytes() == _labels32(want["came_from"]).tobytes(), what + ": labels"
    assert _fetch(ptr["vis_global"], (ny, nx), np.float64).tobytes() == want["vis_global"].tobytes(), what + ": vis_global"
    assert _fetch(ptr["vis_local"], (ny, nx), np.float64).tobytes() == want["vis_local"].tobytes(), what + ": vis_local"
    piv = _fetch(ptr["pivots"], (want["n_pivots"] + 1, 2), np.int32)
    assert piv.tolist() == want["pivots"].tolist(), "%s: pivots, first difference at %r" % (what, ls.first_pivot_difference(piv, want["pivots"]))


# ---- a. the plain solve

@pytest.mark.parametrize("name", ["A", "B", "E", "F", "G", "H", "L"])
def test_plain_solve(vhp, oracle, name):
    case = ls.CASES[name]
    c = _ctx(vhp, case["map"])
    got = c.planner_solve(case["start"], case["end"], THR, case["max_iter"])
    assert c.last_sweep_kernel() == 4
    _same(got, ls.solve(oracle, name), "case " + name)
    assert got["n_pivots"] == case["n_pivots"]


@pytest.mark.parametrize("name", ["B", "G"])
def test_plain_solve_device_results(vhp, oracle, name):
    case = ls.CASES[name]
    want = ls.solve(oracle, name)
    c = _ctx(vhp, case["map"])
    rc, n_piv, ptr = c.planner_solve_device(case["start"], case["end"], THR, case["max_iter"])
    assert (rc, n_piv) == (want["status"], want["n_pivots"]) == (0, case["n_pivots"])
    assert c.last_sweep_kernel() == 4
    _device_results_equal(ptr, want, "case %s, device results" % name)
    assert int((_fetch(ptr["labels"], want["came_from"].shape, np.uint32) == UNL32).sum()) == int((want["came_from"] == vhp.UNLABELLED).sum())


def test_two_plain_solves_on_one_context_larger_first(vhp, oracle):
    c = _ctx(vhp, "M300")
    for name in ("A", "B"):   # 2833 pivots, then 1037 in the state the first left
        case = ls.CASES[name]
        _same(c.planner_solve(case["start"], case["end"], THR, case["max_iter"]), ls.solve(oracle, name), "case %s, second of A then B" % name)


# ---- b. the speculative solve, exact mode

@pytest.mark.parametrize("name,k", [("B", 2), ("B", 8), ("G", 2), ("G", 8), ("A", 4)])
def test_speculative_exact(vhp, oracle, name, k):
    case = ls.CASES[name]
    c = _ctx(vhp, case["map"])
    got = c.planner_solve_speculative(case["start"], case["end"], THR, case["max_iter"], k=k, mode=0)
    assert c.last_sweep_kernel() == 4
    _same(got, ls.solve(oracle, name), "case %s, exact mode, k=%d" % (name, k))
    assert got["hits"] + got["sweeps"] == case["n_pivots"]   # (one look-up per iteration: a hit or a sweep)


# ---- c. the speculative solve, fast mode

# (case, k, max_iter): (status, n_pivots, sweep launches, largest label) as first measured on an MI355X after the validity checks had
# passed; the solve is deterministic (the runner-ups come from per-wavefront minima of a fixed launch shape), so they are pinned.
# On M300 the fast mode does not see A's end within 3000 pivots at any k (the exact solve needs 2833): it is cut, with labels up to
# 3001; on M301 it solves G with 1150 to 2250 pivots.
FAST_RUNS = {
    ("A", 2, 3000): (20, 3002, 1502, 3001),
    ("A", 4, 3000): (20, 3002, 757, 3001),
    ("A", 8, 3000): (20, 3002, 390, 3000),
    ("G", 2, 3000): (0, 1150, 577, 1149),
    ("G", 4, 3000): (0, 1290, 327, 1289),
    ("G", 8, 3000): (0, 2250, 291, 2249),
    ("A", 8, 1030): (20, 1032, 144, 1031),
}


def _check_cut_plan(vhp, occ, r, start):
    """_check_valid_plan's conditions for a solve that ran out of iterations (no end, no path): labels index pivots, every pivot was lit
    by an earlier one"""
    piv, came, n = r["pivots"], r["came_from"], r["n_pivots"]
    assert tuple(piv[0]) == tuple(start)
    assert came[came != vhp.UNLABELLED].max() < n
    for k in range(1, n):
        x, y = int(piv[k][0]), int(piv[k][1])
        assert came[y, x] < k, "pivot %d at (%d,%d) carries label %d" % (k, x, y, came[y, x])
        assert occ[y, x] == 1


def _fast(vhp, oracle, name, k, max_iter):
    case = ls.CASES[name]
    occ = ls.map_of(case["map"])
    c = _ctx(vhp, case["map"])
    r = c.planner_solve_speculative(case["start"], case["end"], THR, max_iter, k=k, mode=1)
    assert c.last_sweep_kernel() == 4
    lab = r["came_from"][r["came_from"] != vhp.UNLABELLED]
    print("fast mode %r: status %d, n_pivots %d, sweeps %d, hits %d, largest label %d, cells labelled >= 1024: %d" % (
        (name, k, max_iter), r["status"], r["n_pivots"], r["sweeps"], r["hits"], int(lab.max()), int((lab >= ls.LDS_PIVOTS).sum())))
    assert r["status"] in (vhp.VHP_OK, vhp.VHP_ERR_MAX_ITER)
    assert r["n_pivots"] <= max_iter + 8
    if r["status"] == vhp.VHP_OK:
        _check_valid_plan(vhp, occ, r, case["start"], case["end"], THR)
    else:
        _check_cut_plan(vhp, occ, r, case["start"])
    return c, r, int(lab.max())


@pytest.mark.parametrize("name,k,max_iter", sorted(FAST_RUNS))
def test_speculative_fast(vhp, oracle, name, k, max_iter):
    case = ls.CASES[name]
    occ = ls.map_of(case["map"])
    c, r, top = _fast(vhp, oracle, name, k, max_iter)
    # the union, the labels and the last local field from the oracle's sweeps of exactly the committed pivots, in commit order (a sweep
    # per pivot: 1.6 s for 3002 of them)
    union, label, last = _union_of_the_pivots_fields(oracle, occ, r, THR, case["start"])
    assert np.array_equal(r["vis_global"], union)
    assert np.array_equal(r["vis_local"], last)
    got = np.where(r["came_from"] == vhp.UNLABELLED, -1, r["came_from"].astype(np.int64))
    bad = np.argwhere(got != label)
    assert bad.size == 0, "%d labels differ, the smallest label involved: %d" % (len(bad), min(int(got[got != label].min()), int(label[got != label].min())))
    if max_iter == 1030:
        assert r["status"] == vhp.VHP_ERR_MAX_ITER and 1030 < r["n_pivots"] <= 1038   # (the room for max_iter + 8 pivots, past 1024)
    # the path call on the tree a fast solve leaves: the old route on its own host arrays (a cut solve: VHP_ERR_ARG, both zero)
    cap = r["n_pivots"] + 3
    want = [_old_route(vhp, r, case["end"], cap)]
    _check_paths(vhp, c, c.lib.vhp_planner_path, c.lib.vhp_planner_path_device, want, cap, "fast mode path")
    p = c.planner_path()
    assert (p["status"], p["n_path"], _bits(p["length"]), p["path"].tolist()) == want[0]
    if r["status"] != vhp.VHP_OK:
        assert want[0] == (vhp.VHP_ERR_ARG, 0, _bits(0.0), [])
    else:
        assert want[0][0] == vhp.VHP_OK and want[0][1] >= 3
        if want[0][1] > 100:
            small = [_old_route(vhp, r, case["end"], 100)]
            assert small[0][0] == vhp.VHP_ERR_TOO_LARGE and small[0][1] == want[0][1]
            _check_paths(vhp, c, c.lib.vhp_planner_path, c.lib.vhp_planner_path_device, small, 100, "fast mode path, cap 100")
    assert (r["status"], r["n_pivots"], r["sweeps"], top) == FAST_RUNS[(name, k, max_iter)]


def test_fast_mode_reaches_beyond_1024_on_each_map():
    """at least one pinned run per map commits 1025 pivots or more and labels a cell >= 1024: the `nb + nc` staging of that epilogue"""
    for m in ("A", "G"):
        assert any(v[1] >= 1025 and v[3] >= ls.LDS_PIVOTS for (name, _, _), v in FAST_RUNS.items() if name == m), m


# ---- d. the batch solve on M300

def _oob_query():
    return (-3, 7) + ls.CASES["A"]["end"]


def _batch1():
    """max_iter 3000: A, C, B and D end at iterations 2833, 2507, 1037 and 736 -- the set of running queries shrinks four times"""
    return [ls.query("A"), ls.query("D"), ls.query("B"), ls.query("C"), _oob_query(), ls.query("A")], ["A", "D", "B", "C", None, "A"], 3000


def _batch2():
    """max_iter 1030: four queries are cut at 1031 pivots with labels up to 1030, D finishes"""
    return [ls.query("A"), ls.query("B"), ls.query("C"), ls.query("D"), ls.query("F")], ["A", "B", "C", "D", "F"], 1030


def _batch_oracle(oracle, names, max_iter):
    """the oracle's solve per query (None: no case, a query that fails validation); a case that ends below max_iter is its own solve"""
    out = []
    for n in names:
        case = ls.CASES[n] if n else None
        ended = n and case["status"] == ls.OK and case["n_pivots"] <= max_iter <= case["max_iter"]
        out.append(None if n is None else ls.solve(oracle, n) if ended else ls.solve(oracle, n, max_iter=min(max_iter, case["max_iter"])))
    return out


def _compare_batch(vhp, res, orc, codes, what):
    """every query of a batch against its oracle solve (orc[q] None: the validation code codes[q] and no results)"""
    assert [r["status"] for r in res] == [codes[q] if o is None else o["status"] for q, o in enumerate(orc)], what
    assert [r["n_pivots"] for r in res] == [0 if o is None else o["n_pivots"] for o in orc], what
    for q, (r, o) in enumerate(zip(res, orc)):
        if o is None:
            assert r["came_from"] is None
        else:
            _same(r, o, "%s, query %d" % (what, q))


@pytest.fixture(scope="module")
def batch1(vhp, oracle):
    """(context, results, oracle's solves, queries) of batch 1, solved with planner_batch_group 1, 2 and 0 -- no result depends on G --;
    the state left is the automatic group's"""
    queries, names, max_iter = _batch1()
    orc = _batch_oracle(oracle, names, max_iter)
    c = _ctx(vhp, "M300")
    for group in (1, 2, 0):
        c.set_option("planner_batch_group", group)
        res = c.planner_solve_batch(queries, THR, max_iter)
        assert c.last_sweep_kernel() == 4
        if group:
            assert c.planner_batch_group() == group
        else:
            assert c.planner_batch_group() >= 8   # (the automatic group: the largest of 32, 16, 8 ... that fits)
        _compare_batch(vhp, res, orc, {4: vhp.VHP_ERR_START_OOB}, "batch 1, group %d" % group)
    return c, res, orc, queries


@pytest.fixture(scope="module")
def batch2(vhp, oracle):
    queries, names, max_iter = _batch2()
    orc = _batch_oracle(oracle, names, max_iter)
    c = _ctx(vhp, "M300")
    res = c.planner_solve_batch(queries, THR, max_iter)
    assert c.last_sweep_kernel() == 4
    _compare_batch(vhp, res, orc, {}, "batch 2")
    return c, res, orc, queries


def test_batch_of_long_and_short_queries(vhp, batch1):
    c, res, orc, _ = batch1
    assert [r["n_pivots"] for r in res] == [2833, 736, 1037, 2507, 0, 2833]
    for name in ("came_from", "vis_global", "vis_local", "pivots"):
        assert res[0][name].tobytes() == res[5][name].tobytes()
    for q in (2, 0):   # 13 pivots past 1024, and 1809
        _device_results_equal(c.planner_batch_results_device(q), orc[q], "batch 1, query %d, device results" % q)


def test_batch_cut_past_1024(vhp, batch2):
    c, res, orc, _ = batch2
    assert [(r["status"], r["n_pivots"]) for r in res] == [(vhp.VHP_ERR_MAX_ITER, 1031)] * 3 + [(vhp.VHP_OK, 736), (vhp.VHP_ERR_MAX_ITER, 1031)]
    for q in (0, 1, 2, 4):
        assert int(orc[q]["came_from"][orc[q]["came_from"] != vhp.UNLABELLED].max()) == 1030
    _device_results_equal(c.planner_batch_results_device(1), orc[1], "batch 2, query 1, device results")


# ---- e. the maps batch on the odd-sided stack

def _maps_case():
    occ = ls.map_of("M301b")
    by, bx = (int(v) for v in np.argwhere(occ == 0)[5000])
    blocked_end = ls.CASES["K"]["start"] + (bx, by)
    queries = [ls.query("G"), ls.query("H"), ls.query("I"), ls.query("K"), ls.query("N"), blocked_end]
    return queries, ["G", "H", "I", "K", "N", None], [0, 0, 0, 1, 1, 1], 1600


@pytest.fixture(scope="module")
def maps_batch(vhp, oracle):
    queries, names, idx, max_iter = _maps_case()
    orc = _batch_oracle(oracle, names, max_iter)
    stack = np.stack([ls.map_of("M301"), ls.map_of("M301b")])
    c = vhp.Context(0)
    c.set_maps(stack)
    res = c.planner_solve_maps_batch(queries, idx, THR, max_iter)
    assert c.last_sweep_kernel() == 4
    _compare_batch(vhp, res, orc, {5: vhp.VHP_ERR_END_OCCUPIED}, "maps batch")
    return c, res, orc, queries, idx, stack


def test_maps_batch_on_the_odd_stack(vhp, maps_batch):
    c, res, orc, queries, idx, stack = maps_batch
    assert [r["n_pivots"] for r in res] == [1287, 1501, 681, 983, 1601, 0]
    ref = vhp.Context(0)
    for k in (0, 1):   # ... and the plain solve on set_map(that map)
        ref.set_map(stack[k])
        for q, qu in enumerate(queries):
            if idx[q] == k and orc[q] is not None:
                _same(ref.planner_solve(qu[:2], qu[2:], THR, 1600), res[q], "maps batch query %d vs set_map + planner_solve" % q)
    _device_results_equal(c.planner_maps_batch_results_device(4), orc[4], "maps batch, query 4, device results")


# ---- f. paths

def _path_wants(vhp, res, queries, cap):
    return [_old_route(vhp, r, q[2:], cap) if r["came_from"] is not None else (r["status"], 0, _bits(0.0), []) for r, q in zip(res, queries)]


def _paths_three_ways(vhp, oracle, c, host_call, dev_call, default_call, res, orc, queries, what):
    """cap = None (the binding's default room), cap = 100 (below every path here) and no path buffer, host and device forms, against the
    old route on the solve's host arrays and against the oracle's reconstruct_path on the oracle's"""
    cap = max(r["n_pivots"] for r in res) + 3
    want = _path_wants(vhp, res, queries, cap)
    got = _check_paths(vhp, c, host_call, dev_call, want, cap, what)   # (the call without a buffer is in there too)
    dflt = default_call()
    assert [(p["status"], p["n_path"], _bits(p["length"]), p["path"].tolist()) for p in dflt] == want, what + ", default room"
    small = _path_wants(vhp, res, queries, 100)
    _check_paths(vhp, c, host_call, dev_call, small, 100, what + ", cap 100")
    n_long = 0
    for q, o in enumerate(orc):
        if o is not None and o["status"] == 0:
            d, path = oracle.reconstruct_path(o["came_from"], o["pivots"], queries[q][2:])
            assert got[q] == (0, len(path), _bits(d), path.tolist()), "%s, query %d vs the oracle" % (what, q)
            assert len(path) > 100 and small[q][:3] == (vhp.VHP_ERR_TOO_LARGE, len(path), _bits(d)), (what, q)
            n_long += 1
        elif o is not None:   # cut by max_iter: the end is unlabelled
            assert got[q] == (vhp.VHP_ERR_ARG, 0, _bits(0.0), []) and small[q] == got[q], (what, q)
    return got, n_long


def test_plain_paths(vhp, oracle):
    c = _ctx(vhp, "M300")
    lib = c.lib
    for name in ("A", "E", "F"):   # E and F: cut by max_iter, their ends unlabelled
        case = ls.CASES[name]
        r = c.planner_solve(case["start"], case["end"], THR, case["max_iter"])
        o = ls.solve(oracle, name)
        _same(r, o, "case " + name)
        got, n_long = _paths_three_ways(vhp, oracle, c, lib.vhp_planner_path, lib.vhp_planner_path_device, lambda: [c.planner_path()], [r], [o],
                                        [ls.query(name)], "plain " + name)
        assert n_long == (1 if name == "A" else 0)
        if name == "A":
            assert got[0][1] == case["n_path"] == 215


def test_batch_paths(vhp, oracle, batch1, batch2):
    for which, (c, res, orc, queries), n_ok in (("batch 1", batch1, 5), ("batch 2", batch2, 1)):
        got, n_long = _paths_three_ways(vhp, oracle, c, c.lib.vhp_planner_batch_paths, c.lib.vhp_planner_batch_paths_device, c.planner_batch_paths,
                                        res, orc, queries, which)
        assert n_long == n_ok
    assert (max(r["n_pivots"] for r in batch1[1]) + 1 + 255) // 256 == 12   # blocks in x of vhp_paths_parents after batch 1


def test_maps_batch_paths(vhp, oracle, maps_batch):
    c, res, orc, queries, _, _ = maps_batch
    got, n_long = _paths_three_ways(vhp, oracle, c, c.lib.vhp_planner_maps_batch_paths, c.lib.vhp_planner_maps_batch_paths_device,
                                    c.planner_maps_batch_paths, res, orc, queries, "maps batch")
    assert n_long == 4 and got[5][0] == vhp.VHP_ERR_END_OCCUPIED
    assert sorted(r["n_pivots"] + 1 for r in res if r["came_from"] is not None) == [682, 984, 1288, 1502, 1602]   # the rows of one launch


# ---- g. the tree calls

def _tree_goals(vhp, orc, occ_of, nx, ny, seed, n_random=4096):
    """(q, x, y) rows: every pivot's cell of a query whose own label is >= 1024, n_random seeded labelled cells over the queries, some
    unlabelled free and some blocked cells, one cell outside the grid"""
    rng = np.random.default_rng(seed)
    solved = [q for q, o in enumerate(orc) if o is not None]
    goals, n_through = [], 0
    for q in solved:
        o = orc[q]
        piv = o["pivots"][: o["n_pivots"]]
        own = ls.labels_of_pivots(o)
        goals += [(q, int(x), int(y)) for x, y in piv[own >= ls.LDS_PIVOTS]]
        # a pivot's cell labelled t >= 1024 where pivot t's own cell is labelled >= 1024 too: a chain through two entries beyond the bound
        deep = own[own >= ls.LDS_PIVOTS].astype(np.int64)
        n_through += int((own[deep] >= ls.LDS_PIVOTS).sum())
    n_beyond = len(goals)
    for q in solved:
        o = orc[q]
        lit = np.argwhere(o["came_from"] != vhp.UNLABELLED)
        goals += [(q, int(lit[k][1]), int(lit[k][0])) for k in rng.integers(0, len(lit), n_random // len(solved) + 1)]
        dark = np.argwhere((o["came_from"] == vhp.UNLABELLED) & (occ_of(q) == 1))
        goals += [(q, int(dark[k][1]), int(dark[k][0])) for k in rng.integers(0, len(dark), 8)]
        blocked = np.argwhere(occ_of(q) == 0)
        goals += [(q, int(blocked[k][1]), int(blocked[k][0])) for k in rng.integers(0, len(blocked), 8)]
    goals.append((solved[0], nx, 3))
    return goals, n_beyond, n_through


def _deepest(vhp, orc):
    """the largest n_path over all cells of the solved queries, from the oracle's arrays (depth of a label + 2)"""
    top = 0
    for o in orc:
        if o is None:
            continue
        n = o["n_pivots"]
        parent = np.zeros(n + 1, np.int64)
        parent[:n] = ls.labels_of_pivots(o).astype(np.int64)
        depth = np.zeros(n + 1, np.int64)
        for t in range(1, n):   # (a pivot's label is below its own index: one pass)
            depth[t] = depth[parent[t]] + 1
        top = max(top, int(depth[:n].max()) + 2)
    return top


def _check_tree(vhp, oracle, c, solve, res, orc, occ_of, nx, ny, what, seed):
    # every cell of every query: both outputs, host and device forms, sub-ranges, a shifted start (_check_fields); the solves equal the
    # oracle's byte for byte, so the old route on their arrays is the old route on the oracle's
    wl, wc = _check_fields(vhp, c, solve, res, nx, ny, what)
    gl, gc = c.planner_length_fields(solve)
    assert _against_oracle_walk(vhp, oracle, c, solve, [o if o is not None else {"status": -1} for o in orc], gl, gc, what) >= 25
    for shift in (0, 1):   # both outputs together, the start 16-byte aligned and 8 bytes (4 for the counts) off it: the scalar path
        dl, dc = _fields_device(vhp, c, KINDS[solve], 0, len(res), nx, ny, shift=shift)
        _same_fields(dl, dc, wl, wc, "%s, device form, shift %d" % (what, shift))
    goals, n_beyond, n_through = _tree_goals(vhp, orc, occ_of, nx, ny, seed)
    deepest = _deepest(vhp, orc)
    assert 100 < int(wc.max()) <= deepest   # (room for any cell's path: a pivot that labels no cell may be the deepest)
    got = _check_goals(vhp, c, solve, res, goals, deepest, what)
    assert {g[0] for g in got} >= {vhp.VHP_OK, vhp.VHP_ERR_ARG, vhp.VHP_ERR_END_OOB}
    assert sum(g[1] > 100 for g in got) >= 1000
    small = _check_goals(vhp, c, solve, res, goals[::16], 100, what + ", cap 100")
    assert {g[0] for g in small} >= {vhp.VHP_OK, vhp.VHP_ERR_TOO_LARGE}
    return wl, wc, goals, n_beyond, n_through


def test_tree_after_a_plain_solve(vhp, oracle):
    """2834 table entries: the L2 branch of vhp_tree_fields alone, twelve rounds of vhp_tree_tables' loops"""
    case = ls.CASES["A"]
    occ = ls.map_of("M300")
    c = _ctx(vhp, "M300")
    r = c.planner_solve(case["start"], case["end"], THR, case["max_iter"])
    o = ls.solve(oracle, "A")
    _same(r, o, "case A")
    wl, wc, goals, n_beyond, n_through = _check_tree(vhp, oracle, c, "plain", [r], [o], lambda q: occ, 300, 300, "plain A", 21)
    assert n_beyond == case["pivots_beyond"] == 1623 and n_through >= 1000   # chains that pass through entries >= 1024
    ex, ey = case["end"]
    assert int(wc[0, ey, ex]) == 215 and int(wc.max()) >= 215
    # the host form refuses a goal whose query is outside the solve, and writes nothing
    bad = np.array([[0, ex, ey], [1, ex, ey]], np.int32)
    st = np.full(2, 777, np.int32)
    assert c.lib.vhp_planner_goal_paths(c.h, 0, bad.ctypes.data_as(C.c_void_p), 2, None, 0, None, None, st.ctypes.data_as(C.c_void_p)) == vhp.VHP_ERR_ARG
    assert (st == 777).all()
    assert _goals_device(vhp, c, 0, [(1, ex, ey), (-1, ex, ey)], 8) == [(vhp.VHP_ERR_ARG, 0, _bits(0.0), [])] * 2


def test_tree_after_the_batch(vhp, oracle, batch1):
    c, res, orc, queries = batch1
    occ = ls.map_of("M300")
    wl, wc, goals, n_beyond, n_through = _check_tree(vhp, oracle, c, "batch", res, orc, lambda q: occ, 300, 300, "batch 1", 22)
    assert n_beyond == 2 * 1623 + 12 + 1336 and (wl[4] == -1.0).all() and (wc[4] == 0).all()
    # D and B alone: one table staged in LDS and one read through L2 in one launch, under a table stride of 1037 + 1
    assert [res[q]["n_pivots"] for q in (1, 2)] == [736, 1037]
    gl, gc = c.planner_length_fields("batch", q_first=1, n_q=2)
    _same_fields(gl, gc, wl[1:3], wc[1:3], "batch 1, queries 1 and 2, host form")
    for shift in (0, 1):
        dl, dc = _fields_device(vhp, c, 1, 1, 2, 300, 300, shift=shift)
        _same_fields(dl, dc, wl[1:3], wc[1:3], "batch 1, queries 1 and 2, device form, shift %d" % shift)
    st = np.full(1, 777, np.int32)
    bad = np.array([[6, 5, 5]], np.int32)
    assert c.lib.vhp_planner_goal_paths(c.h, 1, bad.ctypes.data_as(C.c_void_p), 1, None, 0, None, None, st.ctypes.data_as(C.c_void_p)) == vhp.VHP_ERR_ARG
    assert st[0] == 777


def test_tree_after_the_maps_batch(vhp, oracle, maps_batch):
    c, res, orc, queries, idx, stack = maps_batch
    wl, wc, goals, n_beyond, n_through = _check_tree(vhp, oracle, c, "maps", res, orc, lambda q: stack[idx[q]], 301, 277, "maps batch", 23)
    assert n_beyond >= 247 + 441 and n_through >= 100
    assert (wl[5] == -1.0).all() and (wc[5] == 0).all()
