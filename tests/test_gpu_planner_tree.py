"""Path lengths to every cell and paths to any goal from a planner solve (vhp_planner_length_fields, vhp_planner_goal_paths; host and
device forms, all three selectors) against the route they replace -- the solve's host copies of labels and pivots + one
vhp_reconstruct_path call per cell: status, point count, every point, and the length by == on its float64 bits -- and, for the exact
solves, against the same call on the CPU oracle's solve() at every checked cell and against the oracle's own reconstruct_path at
seeded cells of every solved query.
Non-vacuity: in every multi-cell case at least half of the checked cells are ones where vhp_reconstruct_path on the ORACLE's arrays
returns VHP_OK and at least a quarter have three or more points.  That is asserted from the oracle's results, so it is a property of
the inputs (maps, queries and thresholds were chosen with the oracle on the CPU), not of the code under test.  A solve stops when it
sees its end, so only far-apart starts and ends light most of a map; on maze_6 the query of BASELINE config 4 labels 16 % of the
cells (64 pivots), the other queries here 10-55 %, so the maze's sample is drawn half from all cells and half from the cells the
oracle labelled (plus every pivot's cell); the condition is then partly true by construction there, and the uniform 4096 cells and
the pivots' cells are checked all the same."""
import ctypes as C
import struct

import numpy as np
import pytest

import maps

pytestmark = pytest.mark.gpu

SENTINEL = -777
KINDS = {"plain": 0, "batch": 1, "maps": 2}


@pytest.fixture(scope="module")
def vhp():
    import torch  # noqa: F401
    import vhp_amd
    return vhp_amd


def _bits(x):
    return struct.pack("<d", float(x)).hex()


def _walk(vhp, r, goal, cap):
    """vhp_reconstruct_path from `goal` on a solve's host arrays: (status, n_path, length bits, points) -- n_path and length 0 where the
    call leaves them alone; cap < 0: no path buffer"""
    lib = vhp.load_library()
    came = r["came_from"]
    ny, nx = came.shape
    path = np.full((max(cap, 1), 2), SENTINEL, np.int32)
    n, d = C.c_uint32(0), C.c_double(0.0)
    rc = lib.vhp_reconstruct_path(came.ctypes.data_as(C.c_void_p), r["pivots"].ctypes.data_as(C.c_void_p), r["n_pivots"], nx, ny, int(goal[0]),
                                  int(goal[1]), path.ctypes.data_as(C.c_void_p) if cap >= 0 else None, max(cap, 0), C.byref(n), C.byref(d))
    return rc, n.value, _bits(d.value), path[: n.value].tolist() if rc == vhp.VHP_OK and cap >= 0 else []


def _prep(r):
    return dict(r, came_from=np.ascontiguousarray(r["came_from"], np.uint64), pivots=np.ascontiguousarray(r["pivots"], np.int32))


def _ref_cells(vhp, r, cells):
    """what the length field must hold at `cells` [(x, y)]: (length float64 with -1.0 filler, n_path uint32 with 0 filler)"""
    length = np.full(len(cells), -1.0, np.float64)
    cnt = np.zeros(len(cells), np.uint32)
    if r is None or r["came_from"] is None:
        return length, cnt
    lib = vhp.load_library()
    r = _prep(r)
    ny, nx = r["came_from"].shape
    pc, pp = r["came_from"].ctypes.data_as(C.c_void_p), r["pivots"].ctypes.data_as(C.c_void_p)
    n, d = C.c_uint32(0), C.c_double(0.0)
    for k, (x, y) in enumerate(cells):
        if lib.vhp_reconstruct_path(pc, pp, r["n_pivots"], nx, ny, int(x), int(y), None, 0, C.byref(n), C.byref(d)) == vhp.VHP_OK:
            length[k], cnt[k] = d.value, n.value
    return length, cnt


def _all_cells(nx, ny):
    return [(x, y) for y in range(ny) for x in range(nx)]


def _not_vacuous(cnts, what):
    cnt = np.concatenate([np.asarray(c).reshape(-1) for c in cnts])
    assert 2 * int((cnt > 0).sum()) >= cnt.size, "%s: only %d of %d cells have a path in the oracle's results" % (what, (cnt > 0).sum(), cnt.size)
    assert 4 * int((cnt >= 3).sum()) >= cnt.size, "%s: only %d of %d cells have a path of three or more points" % (what, (cnt >= 3).sum(), cnt.size)


def _same(got_len, got_cnt, want_len, want_cnt, what):
    assert got_cnt.dtype == np.uint32 and got_len.dtype == np.float64
    bad = np.flatnonzero((got_cnt.reshape(-1) != want_cnt.reshape(-1)) | (got_len.reshape(-1).view(np.uint64) != want_len.reshape(-1).view(np.uint64)))
    assert bad.size == 0, "%s: %d cells differ, first at flat index %d: got (%r, %d), want (%r, %d)" % (
        what, bad.size, bad[0], got_len.reshape(-1)[bad[0]], got_cnt.reshape(-1)[bad[0]], want_len.reshape(-1)[bad[0]], want_cnt.reshape(-1)[bad[0]])


def _fields_device(vhp, c, kind, q_first, n_q, nx, ny, shift=0, want=(True, True)):
    """the _device form into torch buffers pre-filled with a sentinel, `shift` elements into them (shift = 1: fields that start off the
    16-byte grid); also shows that nothing but the fields is written"""
    import torch
    n, pad = n_q * nx * ny, 64
    length = torch.full((n + 2 * pad,), -777.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((n + 2 * pad,), 777, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    at = pad + shift
    c._check(c.lib.vhp_planner_length_fields_device(c.h, kind, q_first, n_q, C.c_void_p(length.data_ptr() + 8 * at if want[0] else None),
                                                    C.c_void_p(cnt.data_ptr() + 4 * at if want[1] else None)))
    c.sync()
    length, cnt = length.cpu().numpy(), cnt.cpu().numpy()
    for buf, s, w in ((length, -777.0, want[0]), (cnt, 777, want[1])):
        assert (buf[:at] == s).all() and (buf[at + n:] == s).all(), "written outside the fields"
        assert w or (buf == s).all(), "an output that was not asked for was written"
    return length[at: at + n].reshape(n_q, ny, nx), cnt[at: at + n].view(np.uint32).reshape(n_q, ny, nx)


def _against_oracle_walk(vhp, oracle, c, solve, orc, gl, gc, what, per_query=24):
    """the exact solves against the oracle's own reconstruct_path (not the library's host walk): at seeded cells of each solved query
    that the field says have a path, the field's length bits and count and goal_paths' points are the oracle's"""
    checked = 0
    for q, o in enumerate(orc):
        if o["status"] != 0:
            continue
        ys, xs = np.nonzero(gc[q] > 0)
        assert len(xs) > 0, (what, q)
        pick = np.random.default_rng(77 + q).integers(0, len(xs), per_query)
        goals = [(q, int(xs[k]), int(ys[k])) for k in pick] + [(q, int(o["pivots"][-1][0]), int(o["pivots"][-1][1]))]
        got = c.planner_goal_paths(goals, solve, cap=o["n_pivots"] + 3)
        for (_, x, y), g in zip(goals, got):
            d, path = oracle.reconstruct_path(o["came_from"], o["pivots"], (x, y))
            assert (int(gc[q, y, x]), _bits(gl[q, y, x])) == (len(path), _bits(d)), "%s, query %d, cell (%d, %d) vs the oracle's walk" % (what, q, x, y)
            assert (g["status"], g["n_path"], _bits(g["length"]), g["path"].tolist()) == (0, len(path), _bits(d), path.tolist()), (what, q, x, y)
            checked += 1
    return checked


def _check_fields(vhp, c, solve, res, nx, ny, what, orc=None, oracle=None):
    """every cell of every query, host and device forms, whole range and sub-ranges, against the old route (and the oracle's)"""
    kind = KINDS[solve]
    cells = _all_cells(nx, ny)
    want = [_ref_cells(vhp, r, cells) for r in res]
    wl = np.stack([w[0] for w in want]).reshape(len(res), ny, nx)
    wc = np.stack([w[1] for w in want]).reshape(len(res), ny, nx)
    if orc is not None:
        oc = [_ref_cells(vhp, r if r["status"] in (0, 20) else None, cells) for r in orc]
        _not_vacuous([o[1] for o in oc], what)
        for q, (o, r) in enumerate(zip(oc, orc)):
            if r["status"] in (0, 20):
                _same(o[0], o[1], wl[q], wc[q], "%s, query %d: old route vs oracle" % (what, q))
    Q = len(res)
    gl, gc = c.planner_length_fields(solve)
    _same(gl, gc, wl, wc, what + ", host form")
    if oracle is not None:
        _against_oracle_walk(vhp, oracle, c, solve, orc, gl, gc, what)
    dl, dc = _fields_device(vhp, c, kind, 0, Q, nx, ny)
    _same(dl, dc, wl, wc, what + ", device form")
    if Q > 1:
        gl, gc = c.planner_length_fields(solve, q_first=1)
        _same(gl, gc, wl[1:], wc[1:], what + ", host form from query 1")
        dl, dc = _fields_device(vhp, c, kind, 1, Q - 1, nx, ny)
        _same(dl, dc, wl[1:], wc[1:], what + ", device form from query 1")
        dl, dc = _fields_device(vhp, c, kind, Q - 1, 1, nx, ny, shift=1)
        _same(dl, dc, wl[Q - 1:], wc[Q - 1:], what + ", device form, last query, buffers one element off")
    # one output only
    length = np.empty((Q, ny, nx), np.float64)
    c._check(c.lib.vhp_planner_length_fields(c.h, kind, 0, Q, length.ctypes.data_as(C.c_void_p), None))
    cnt = np.empty((Q, ny, nx), np.uint32)
    c._check(c.lib.vhp_planner_length_fields(c.h, kind, 0, Q, None, cnt.ctypes.data_as(C.c_void_p)))
    _same(length, cnt, wl, wc, what + ", host form, one output per call")
    dl, _ = _fields_device(vhp, c, kind, 0, Q, nx, ny, want=(True, False))
    _, dc = _fields_device(vhp, c, kind, 0, Q, nx, ny, shift=1, want=(False, True))
    _same(dl, dc, wl, wc, what + ", device form, one output per call")
    return wl, wc


def _goals_device(vhp, c, kind, goals, cap, with_paths=True):
    import torch
    n = len(goals)
    g = torch.tensor(np.asarray(goals, np.int32).reshape(-1, 3), dtype=torch.int32, device="cuda")
    xy = torch.full((n, max(cap, 1), 2), SENTINEL, dtype=torch.int32, device="cuda")
    cnt = torch.full((n + 8,), 777, dtype=torch.int32, device="cuda")
    length = torch.full((n + 8,), -777.0, dtype=torch.float64, device="cuda")
    st = torch.full((n + 8,), 777, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    c._check(c.lib.vhp_planner_goal_paths_device(c.h, kind, C.c_void_p(g.data_ptr()), n, C.c_void_p(xy.data_ptr() if with_paths else None), cap,
                                                 C.c_void_p(cnt.data_ptr()), C.c_void_p(length.data_ptr()), C.c_void_p(st.data_ptr())))
    c.sync()
    assert (g.cpu().numpy() == np.asarray(goals, np.int32).reshape(-1, 3)).all()
    xy, cnt, length, st = xy.cpu().numpy(), cnt.cpu().numpy(), length.cpu().numpy(), st.cpu().numpy()
    assert (cnt[n:] == 777).all() and (length[n:] == -777.0).all() and (st[n:] == 777).all()
    out = []
    for k in range(n):
        m = int(cnt[k]) if st[k] == vhp.VHP_OK and with_paths else 0
        assert (xy[k, m:] == SENTINEL).all(), "goal %d: points written beyond its path (status %d)" % (k, st[k])
        out.append((int(st[k]), int(cnt[k]), _bits(length[k]), xy[k, :m].tolist()))
    return out


def _check_goals(vhp, c, solve, res, goals, cap, what):
    """both forms against the old route per goal (a query without results: its validation code); returns the host form's results"""
    kind = KINDS[solve]
    prepped = [_prep(r) if r["came_from"] is not None else r for r in res]
    want = [_walk(vhp, prepped[q], (x, y), cap) if res[q]["came_from"] is not None else (res[q]["status"], 0, _bits(0.0), []) for q, x, y in goals]
    got_h = [(p["status"], p["n_path"], _bits(p["length"]), p["path"].tolist()) for p in c.planner_goal_paths(goals, solve, cap=cap)]
    got_d = _goals_device(vhp, c, kind, goals, cap)
    for k in range(len(goals)):
        assert got_h[k] == want[k], "%s, goal %r, host form: %r vs the old route's %r" % (what, goals[k], got_h[k][:3], want[k][:3])
        assert got_d[k] == want[k], "%s, goal %r, device form: %r vs the old route's %r" % (what, goals[k], got_d[k][:3], want[k][:3])
    # counts and lengths only: no path buffer, no VHP_ERR_TOO_LARGE
    n = len(goals)
    g = np.ascontiguousarray(goals, np.int32)
    cnt, length, st = np.zeros(n, np.uint32), np.zeros(n, np.float64), np.zeros(n, np.int32)
    c._check(c.lib.vhp_planner_goal_paths(c.h, kind, g.ctypes.data_as(C.c_void_p), n, None, 0, cnt.ctypes.data_as(C.c_void_p),
                                          length.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p)))
    nopath_d = _goals_device(vhp, c, kind, goals, 0, with_paths=False)
    for k, w in enumerate(want):
        e = (vhp.VHP_OK if w[0] == vhp.VHP_ERR_TOO_LARGE else w[0], w[1], w[2])
        assert (int(st[k]), int(cnt[k]), _bits(length[k])) == e and nopath_d[k][:3] == e, (what, goals[k])
    return got_h


def _corner_map(seed):
    occ = maps.random_rect_map(100, 100, 25, 2, 20, 2, 20, seed=seed)
    occ[5, 5] = occ[95, 95] = 1
    return occ


def _spread_goals(res, queries, occ_of, nx, ny, seed, per_query=6):
    """per query: its own end, seeded cells, a blocked cell, goals outside the grid -- queries without results included"""
    rng = np.random.default_rng(seed)
    goals = []
    for q, qu in enumerate(queries):
        goals.append((q, qu[2], qu[3]))
        goals += [(q, int(rng.integers(0, nx)), int(rng.integers(0, ny))) for _ in range(per_query)]
        by, bx = (int(v) for v in np.argwhere(occ_of(q) == 0)[int(rng.integers(0, 50))])
        goals.append((q, bx, by))
    goals += [(0, -1, 5), (len(queries) - 1, nx, 0), (0, 3, ny), (1 % len(queries), 2, -7)]
    order = rng.permutation(len(goals))
    return [goals[k] for k in order]


def _consistency(vhp, c, solve, res, queries, paths_call, wl, wc, goals, got, what):
    """goal_paths at each query's own end equals the path call; length_fields at a goal equals goal_paths there"""
    ends = [(q, qu[2], qu[3]) for q, qu in enumerate(queries)]
    cap = max(r["n_pivots"] for r in res) + 3
    at_end = c.planner_goal_paths(ends, solve, cap=cap)
    by_paths = c._paths(paths_call, len(queries), cap)
    for q, (a, b) in enumerate(zip(at_end, by_paths)):
        if res[q]["came_from"] is None:
            assert a["status"] == res[q]["status"], (what, q)
        assert (a["status"], a["n_path"], _bits(a["length"]), a["path"].tolist()) == (b["status"], b["n_path"], _bits(b["length"]), b["path"].tolist()), (what, q)
    ny, nx = wl.shape[1:]
    for (q, x, y), g in zip(goals, got):
        if 0 <= x < nx and 0 <= y < ny and res[q]["came_from"] is not None:
            if g[0] in (vhp.VHP_OK, vhp.VHP_ERR_TOO_LARGE):
                assert (g[1], g[2]) == (int(wc[q, y, x]), _bits(wl[q, y, x])), (what, q, x, y)
            else:
                assert (int(wc[q, y, x]), wl[q, y, x]) == (0, -1.0), (what, q, x, y)


def test_errors_and_empty_calls(vhp):
    occ = _corner_map(101)
    c = vhp.Context(0)
    lib = c.lib
    buf = np.zeros(3 * 100 * 100, np.float64)
    p = buf.ctypes.data_as(C.c_void_p)
    g = np.array([[0, 5, 5]], np.int32)
    pg = g.ctypes.data_as(C.c_void_p)
    for kind in (0, 1, 2):   # before any map and any solve
        assert lib.vhp_planner_length_fields(c.h, kind, 0, 1, p, None) == vhp.VHP_ERR_ARG
        assert lib.vhp_planner_goal_paths(c.h, kind, pg, 1, None, 0, None, None, None) == vhp.VHP_ERR_ARG
    c.set_map(occ)
    c.set_maps(occ[None])
    for kind in (0, 1, 2):
        assert lib.vhp_planner_length_fields(c.h, kind, 0, 1, p, None) == vhp.VHP_ERR_ARG
        assert lib.vhp_planner_goal_paths_device(c.h, kind, None, 0, None, 0, None, None, None) == vhp.VHP_ERR_ARG
    c.planner_solve((5, 5), (95, 95), 0.25, 250)
    c.planner_solve_batch([(5, 5, 95, 95)] * 2, 0.25, 250, outputs=False)
    c.planner_solve_maps_batch([(5, 5, 95, 95)] * 3, [0] * 3, 0.25, 250, outputs=False)
    for kind, Q in ((0, 1), (1, 2), (2, 3)):
        assert lib.vhp_planner_length_fields(c.h, kind, 0, Q, p, None) == vhp.VHP_OK
        for q_first, n_q in ((0, Q + 1), (Q, 1), (-1, 1), (0, 0), (0, -1), (1, Q)):
            assert lib.vhp_planner_length_fields(c.h, kind, q_first, n_q, p, None) == vhp.VHP_ERR_ARG, (kind, q_first, n_q)
        assert lib.vhp_planner_length_fields(c.h, kind, 0, Q, None, None) == vhp.VHP_ERR_ARG
        assert lib.vhp_planner_goal_paths(c.h, kind, None, 0, None, 0, None, None, None) == vhp.VHP_OK      # n_goals = 0
        assert lib.vhp_planner_goal_paths_device(c.h, kind, None, 0, None, 0, None, None, None) == vhp.VHP_OK
        assert lib.vhp_planner_goal_paths(c.h, kind, None, 1, None, 0, None, None, None) == vhp.VHP_ERR_ARG
        assert lib.vhp_planner_goal_paths(c.h, kind, pg, -1, None, 0, None, None, None) == vhp.VHP_ERR_ARG
        # the host form refuses a goal whose query is outside the solve, and writes nothing
        bad = np.array([[0, 5, 5], [Q, 5, 5]], np.int32)
        st = np.full(2, 777, np.int32)
        assert lib.vhp_planner_goal_paths(c.h, kind, bad.ctypes.data_as(C.c_void_p), 2, None, 0, None, None, st.ctypes.data_as(C.c_void_p)) == vhp.VHP_ERR_ARG
        assert (st == 777).all()
        # ... the device form gives that goal VHP_ERR_ARG
        got = _goals_device(vhp, c, kind, [(0, 95, 95), (Q, 5, 5), (-1, 5, 5)], 8)
        assert got[0][0] == vhp.VHP_OK and got[1] == (vhp.VHP_ERR_ARG, 0, _bits(0.0), []) and got[2] == got[1]
    for kind in (3, -1):
        assert lib.vhp_planner_length_fields(c.h, kind, 0, 1, p, None) == vhp.VHP_ERR_ARG
        assert lib.vhp_planner_goal_paths(c.h, kind, pg, 1, None, 0, None, None, None) == vhp.VHP_ERR_ARG
    # no state of a solve changes: kernel, elapsed time, group, results
    k0, ms0, g0 = c.last_sweep_kernel(), c.last_elapsed_ms(), c.planner_maps_batch_group()
    c.planner_length_fields("maps")
    c.planner_goal_paths([(0, 95, 95)], "batch")
    assert (c.last_sweep_kernel(), c.last_elapsed_ms(), c.planner_maps_batch_group()) == (k0, ms0, g0)
    c.set_map(occ)   # (drops the plain and the batch results; the maps batch is the stack's)
    assert [lib.vhp_planner_length_fields(c.h, kind, 0, 1, p, None) for kind in (0, 1, 2)] == [vhp.VHP_ERR_ARG, vhp.VHP_ERR_ARG, vhp.VHP_OK]


@pytest.mark.parametrize("seed,max_iter", [(105, 250), (100, 250), (104, 3)])
def test_plain_solves_every_cell(vhp, oracle, seed, max_iter):
    """one 100 x 100 map: solved (9 pivots), live-locked until max_iter (251 pivots), stopped after 3 iterations"""
    occ = _corner_map(seed)
    c = vhp.Context(0)
    c.set_map(occ)
    r = c.planner_solve((5, 5), (95, 95), 0.25, max_iter)
    orc = oracle.solve(occ, (5, 5), (95, 95), 0.25, max_iter)
    assert r["status"] == orc["status"] == (0 if seed == 105 else vhp.VHP_ERR_MAX_ITER)
    what = "plain, seed %d, max_iter %d" % (seed, max_iter)
    wl, wc = _check_fields(vhp, c, "plain", [r], 100, 100, what, orc=[orc], oracle=oracle)
    queries = [(5, 5, 95, 95)]
    goals = _spread_goals([r], queries, lambda q: occ, 100, 100, seed, per_query=40)
    cap = r["n_pivots"] + 3
    got = _check_goals(vhp, c, "plain", [r], goals, cap, what)
    assert {g[0] for g in got} >= {vhp.VHP_OK, vhp.VHP_ERR_ARG, vhp.VHP_ERR_END_OOB}
    _consistency(vhp, c, "plain", [r], queries, c.lib.vhp_planner_path, wl, wc, goals, got, what)
    # the speculative solve's fast mode leaves a different tree in the same state
    r2 = c.planner_solve_speculative((5, 5), (95, 95), 0.25, max_iter, k=4, mode=1)
    l2, c2 = _ref_cells(vhp, r2, _all_cells(100, 100))
    gl, gc = c.planner_length_fields()
    _same(gl, gc, l2, c2, what + ", speculative fast")
    # a solve that fails validation: the filler everywhere, its code for every goal
    bad = c.planner_solve((-1, 0), (95, 95), 0.25, max_iter)
    assert bad["status"] == vhp.VHP_ERR_START_OOB
    gl, gc = c.planner_length_fields()
    assert (gl == -1.0).all() and (gc == 0).all()
    p = c.planner_goal_paths([(0, 95, 95), (0, -1, 3)], cap=8)
    assert [(v["status"], v["n_path"], v["length"], len(v["path"])) for v in p] == [(vhp.VHP_ERR_START_OOB, 0, 0.0, 0)] * 2


def _batch_case():
    """one 100 x 100 map, queries between its corners, one that fails validation, one whose solve hits max_iter"""
    occ = _corner_map(104)
    occ[5, 95] = occ[95, 5] = 1
    queries = [(5, 5, 95, 95), (5, 95, 95, 5), (-1, 5, 95, 95), (95, 5, 5, 95), (5, 5, 95, 95)]
    return occ, queries, [0.25, 0.25, 0.25, 0.25, 0.3], 40


def _maps_case():
    """a stack of 100 x 100 maps, a query on each (map 0's live-locks until max_iter), one that fails validation"""
    seeds = [100, 101, 103, 104, 105, 102]
    stack = np.stack([_corner_map(s) for s in seeds])
    idx = [0, 1, 2, 3, 4, 5, 2, 4]
    queries = [(5, 5, 95, 95)] * 6 + [(5, 5, 100, 95), (95, 95, 5, 5)]
    return stack, idx, queries, 0.25, 250


def test_batch_every_cell(vhp, oracle):
    occ, queries, thr, max_iter = _batch_case()
    c = vhp.Context(0)
    c.set_map(occ)
    res = c.planner_solve_batch(queries, thr, max_iter)
    orc = [oracle.solve(occ, q[:2], q[2:], t, max_iter) for q, t in zip(queries, thr)]
    assert [r["status"] for r in res] == [o["status"] for o in orc]
    assert vhp.VHP_ERR_START_OOB in [r["status"] for r in res] and vhp.VHP_ERR_MAX_ITER in [r["status"] for r in res]
    wl, wc = _check_fields(vhp, c, "batch", res, 100, 100, "batch", orc=orc, oracle=oracle)
    goals = _spread_goals(res, queries, lambda q: occ, 100, 100, 11)
    cap = max(r["n_pivots"] for r in res) + 3
    got = _check_goals(vhp, c, "batch", res, goals, cap, "batch")
    assert {g[0] for g in got} >= {vhp.VHP_OK, vhp.VHP_ERR_ARG, vhp.VHP_ERR_END_OOB, vhp.VHP_ERR_START_OOB}
    _consistency(vhp, c, "batch", res, queries, c.lib.vhp_planner_batch_paths, wl, wc, goals, got, "batch")
    # a cap that is too small for some goals only
    counts = sorted(g[1] for g in got if g[0] == 0)
    small = counts[len(counts) // 2]
    assert counts[0] <= small < counts[-1]
    got_small = _check_goals(vhp, c, "batch", res, goals, small, "batch, cap %d" % small)
    assert {g[0] for g in got_small} >= {vhp.VHP_OK, vhp.VHP_ERR_TOO_LARGE}
    # the results call after the tree calls: the same bytes as before them
    came = np.empty((100, 100), np.uint64)
    c._check(c.lib.vhp_planner_batch_results(c.h, 0, came.ctypes.data_as(C.c_void_p), None, None, None))
    assert came.tobytes() == res[0]["came_from"].tobytes()


def test_maps_batch_every_cell(vhp, oracle):
    stack, idx, queries, thr, max_iter = _maps_case()
    c = vhp.Context(0)
    c.set_maps(stack)
    res = c.planner_solve_maps_batch(queries, idx, thr, max_iter)
    orc = [oracle.solve(stack[k], q[:2], q[2:], thr, max_iter) for q, k in zip(queries, idx)]
    assert [r["status"] for r in res] == [o["status"] for o in orc]
    assert vhp.VHP_ERR_END_OOB in [r["status"] for r in res] and vhp.VHP_ERR_MAX_ITER in [r["status"] for r in res]
    wl, wc = _check_fields(vhp, c, "maps", res, 100, 100, "maps batch", orc=orc, oracle=oracle)
    goals = _spread_goals(res, queries, lambda q: stack[idx[q]], 100, 100, 12)
    cap = max(r["n_pivots"] for r in res) + 3
    got = _check_goals(vhp, c, "maps", res, goals, cap, "maps batch")
    assert {g[0] for g in got} >= {vhp.VHP_OK, vhp.VHP_ERR_ARG, vhp.VHP_ERR_END_OOB}
    _consistency(vhp, c, "maps", res, queries, c.lib.vhp_planner_maps_batch_paths, wl, wc, goals, got, "maps batch")


def _odd_case(nx, ny):
    """a width that is no multiple of 4 (and, 101 x 77, an odd cell count: every other query's field starts off the 16-byte grid)"""
    stack = np.stack([maps.random_rect_map(nx, ny, 14, 3, 16, 3, 16, s) for s in (42, 43)])
    a, b = (2, 2, nx - 3, ny - 3), (nx - 3, 2, 2, ny - 3)
    for q in (a, b):
        stack[:, q[1], q[0]] = stack[:, q[3], q[2]] = 1
    idx = [0, 1, 1, 0, 0]
    queries = [a, a, b, b, a[2:] + a[:2]]
    return stack, idx, queries, 0.25, 100


@pytest.mark.parametrize("nx,ny", [(101, 77), (102, 76)])
def test_odd_sizes(vhp, oracle, nx, ny):
    stack, idx, queries, thr, max_iter = _odd_case(nx, ny)
    c = vhp.Context(0)
    c.set_maps(stack)
    res = c.planner_solve_maps_batch(queries, idx, thr, max_iter)
    orc = [oracle.solve(stack[k], q[:2], q[2:], thr, max_iter) for q, k in zip(queries, idx)]
    what = "%d x %d stack" % (nx, ny)
    wl, wc = _check_fields(vhp, c, "maps", res, nx, ny, what, orc=orc, oracle=oracle)
    goals = _spread_goals(res, queries, lambda q: stack[idx[q]], nx, ny, 13)
    got = _check_goals(vhp, c, "maps", res, goals, max(r["n_pivots"] for r in res) + 3, what)
    _consistency(vhp, c, "maps", res, queries, c.lib.vhp_planner_maps_batch_paths, wl, wc, goals, got, what)
    # ... and the same width on one map
    c.set_map(stack[0])
    on0 = [q for q, k in zip(queries, idx) if k == 0]
    res = c.planner_solve_batch(on0, thr, max_iter)
    _check_fields(vhp, c, "batch", res, nx, ny, "%d x %d batch" % (nx, ny), orc=[o for o, k in zip(orc, idx) if k == 0], oracle=oracle)


def _maze_case():
    occ = maps.maze_6()
    ny = occ.shape[0]
    c4 = (345, ny - 1 - 391, 341, ny - 1 - 10)
    pts = maps.free_sources(occ, 10, 7)
    pairs = [tuple(int(v) for v in pts[2 * k]) + tuple(int(v) for v in pts[2 * k + 1]) for k in range(5)]
    return occ, [c4] + pairs, 0.1, 250


def _maze_sample(orc, nx, ny, q):
    """every pivot's cell, 4096 seeded cells of the grid and 4096 seeded cells among those the oracle labelled"""
    rng = np.random.default_rng(1000 + q)
    cells = [(int(x), int(y)) for x, y in orc["pivots"]]
    cells += [(int(rng.integers(0, nx)), int(rng.integers(0, ny))) for _ in range(4096)]
    lit = np.argwhere(orc["came_from"] < np.uint64(10 ** 9))
    cells += [(int(lit[k][1]), int(lit[k][0])) for k in rng.integers(0, len(lit), 4096)]
    return cells


def test_maze6_sampled(vhp, oracle):
    """maze_6 (BASELINE config 4's query first, the path the reference prints as 1529.55) at Q = 6"""
    occ, queries, thr, max_iter = _maze_case()
    ny, nx = occ.shape
    c = vhp.Context(0)
    c.set_map(occ)
    res = c.planner_solve_batch(queries, thr, max_iter)
    orc = [oracle.solve(occ, q[:2], q[2:], thr, max_iter) for q in queries]
    assert [r["status"] for r in res] == [o["status"] for o in orc] and res[0]["n_pivots"] == 64
    gl, gc = c.planner_length_fields("batch")
    dl, dc = _fields_device(vhp, c, 1, 0, len(queries), nx, ny)
    assert gl.tobytes() == dl.tobytes() and gc.tobytes() == dc.tobytes()
    cnts = []
    for q, (r, o) in enumerate(zip(res, orc)):
        cells = _maze_sample(o, nx, ny, q)
        assert len(cells) >= 4096 + o["n_pivots"]
        xs, ys = np.array([p[0] for p in cells]), np.array([p[1] for p in cells])
        wl, wc = _ref_cells(vhp, r, cells)
        ol, oc = _ref_cells(vhp, o, cells)
        cnts.append(oc)
        _same(ol, oc, wl, wc, "maze_6, query %d: old route vs oracle" % q)
        _same(gl[q, ys, xs], gc[q, ys, xs], wl, wc, "maze_6, query %d" % q)
        # the filler is exactly where the labels are missing or the walk fails: nowhere else in the field is -1
        assert ((gl[q] == -1.0) == (gc[q] == 0)).all() and (gl[q][gc[q] > 0] >= 0).all()
        goals = [(q, x, y) for x, y in cells[:: max(1, len(cells) // 64)]]
        got = _check_goals(vhp, c, "batch", res, goals, r["n_pivots"] + 3, "maze_6, query %d" % q)
        for (_, x, y), g in zip(goals, got):
            if g[0] == 0:
                assert (g[1], g[2]) == (int(gc[q, y, x]), _bits(gl[q, y, x]))
    _not_vacuous(cnts, "maze_6")
    assert _against_oracle_walk(vhp, oracle, c, "batch", orc, gl, gc, "maze_6") >= 25 * 4
    ends = c.planner_goal_paths([(q, qu[2], qu[3]) for q, qu in enumerate(queries)], "batch")
    assert ends[0]["status"] == 0 and "%.6g" % ends[0]["length"] == "1529.55"
    by_paths = c.planner_batch_paths()
    assert [(a["status"], _bits(a["length"]), a["path"].tolist()) for a in ends] == [(b["status"], _bits(b["length"]), b["path"].tolist()) for b in by_paths]
