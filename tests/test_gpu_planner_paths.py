"""The device-side path reconstruction (vhp_planner_path, vhp_planner_batch_paths, vhp_planner_maps_batch_paths; host and device forms)
against the route it replaces -- the solve's host copies of labels and pivots + vhp_reconstruct_path: status, point count, every
point, and the length by == on its float64 bits -- and, for the exact solves, against the CPU oracle's solve() + reconstruct_path.
In every multi-query case at least three quarters of the queries are solved with a path of three or more points; that is asserted
from the ORACLE's results, so it is a property of the inputs (the seeds were chosen with the oracle), not of the code under test."""
import ctypes as C
import struct

import numpy as np
import pytest

import maps

pytestmark = pytest.mark.gpu

SENTINEL = -777


@pytest.fixture(scope="module")
def vhp():
    import torch  # noqa: F401
    import vhp_amd
    return vhp_amd


def _bits(x):
    return struct.pack("<d", float(x)).hex()


def _old_route(vhp, r, end, cap):
    """vhp_reconstruct_path on the host copies a solve / results call gives: (status, n_path, length bits, points) -- n_path and length
    0 where the call returns VHP_ERR_ARG and leaves them alone."""
    lib = vhp.load_library()
    came = np.ascontiguousarray(r["came_from"], np.uint64)
    ny, nx = came.shape
    piv = np.ascontiguousarray(r["pivots"], np.int32)
    path = np.full((max(cap, 1), 2), SENTINEL, np.int32)
    n, d = C.c_uint32(0), C.c_double(0.0)
    rc = lib.vhp_reconstruct_path(came.ctypes.data_as(C.c_void_p), piv.ctypes.data_as(C.c_void_p), r["n_pivots"], nx, ny, int(end[0]), int(end[1]),
                                  path.ctypes.data_as(C.c_void_p), cap, C.byref(n), C.byref(d))
    return rc, n.value, _bits(d.value), path[: n.value].tolist() if rc == vhp.VHP_OK else []


def _host_form(c, call, n, cap):
    return [(p["status"], p["n_path"], _bits(p["length"]), p["path"].tolist()) for p in c._paths(call, n, cap)]


def _device_form(vhp, c, call, n, cap):
    """the _device entry point into torch buffers pre-filled with a sentinel: also shows that nothing but the paths is written"""
    import torch
    xy = torch.full((n, max(cap, 1), 2), SENTINEL, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
    length = torch.zeros(n, dtype=torch.float64, device="cuda")
    st = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    c._check(call(c.h, C.c_void_p(xy.data_ptr()), cap, C.c_void_p(cnt.data_ptr()), C.c_void_p(length.data_ptr()), C.c_void_p(st.data_ptr())))
    c.sync()
    xy, cnt, length, st = xy.cpu().numpy(), cnt.cpu().numpy(), length.cpu().numpy(), st.cpu().numpy()
    out = []
    for q in range(n):
        ok = st[q] == vhp.VHP_OK
        k = int(cnt[q]) if ok else 0
        assert (xy[q, k:] == SENTINEL).all(), "query %d: points written beyond its path (status %d)" % (q, st[q])
        out.append((int(st[q]), int(cnt[q]), _bits(length[q]), xy[q, :k].tolist()))
    return out


def _check(vhp, c, host_call, dev_call, want, cap, what):
    """both forms against `want` (the old route per query, or a validation code); returns the host form's results"""
    n = len(want)
    got_h = _host_form(c, host_call, n, cap)
    got_d = _device_form(vhp, c, dev_call, n, cap)
    for q in range(n):
        assert got_h[q] == want[q], "%s, query %d, host form: %r vs the old route's %r" % (what, q, got_h[q][:3], want[q][:3])
        assert got_d[q] == want[q], "%s, query %d, device form: %r vs the old route's %r" % (what, q, got_d[q][:3], want[q][:3])
    # counts and lengths only: no path buffer, no VHP_ERR_TOO_LARGE
    cnt, length, st = np.zeros(n, np.uint32), np.zeros(n, np.float64), np.zeros(n, np.int32)
    c._check(host_call(c.h, None, 0, cnt.ctypes.data_as(C.c_void_p), length.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p)))
    for q in range(n):
        w = want[q]
        assert (int(st[q]), int(cnt[q]), _bits(length[q])) == (vhp.VHP_OK if w[0] == vhp.VHP_ERR_TOO_LARGE else w[0], w[1], w[2]), (what, q)
    return got_h


def _oracle_paths(oracle, occ_of, queries, thr, max_iter):
    """[(status, path, length) per query] from the oracle's solve() + reconstruct_path (path None where it did not solve)"""
    out = []
    for q, (sx, sy, ex, ey) in enumerate(queries):
        r = oracle.solve(occ_of(q), (sx, sy), (ex, ey), float(thr[q]), max_iter)
        if r["status"] == 0:
            d, p = oracle.reconstruct_path(r["came_from"], r["pivots"], (ex, ey))
            out.append((0, p.tolist(), d))
        else:
            out.append((r["status"], None, None))
    return out


def _not_vacuous(orc):
    good = sum(1 for st, p, _ in orc if st == 0 and len(p) >= 3)
    assert 4 * good >= 3 * len(orc), "only %d of %d queries are solved with a path of three or more points" % (good, len(orc))


def _against_oracle(got, orc, what):
    for q, (st, p, d) in enumerate(orc):
        if st == 0:
            assert got[q][0] == 0 and got[q][3] == p and got[q][2] == _bits(d), "%s, query %d vs the oracle" % (what, q)


def _free_pairs(occ, n, seed):
    pts = maps.free_sources(occ, 2 * n, seed)
    return [tuple(int(v) for v in pts[2 * k]) + tuple(int(v) for v in pts[2 * k + 1]) for k in range(n)]


def _maze6():
    occ = maps.maze_6()
    ny = occ.shape[0]
    return occ, (345, ny - 1 - 391, 341, ny - 1 - 10)


def _ctx(vhp, occ):
    c = vhp.Context(0)
    c.set_map(occ)
    return c


def test_before_any_solve_and_after_set_map(vhp):
    occ, c4 = _maze6()
    c = vhp.Context(0)
    lib = c.lib
    calls = [lib.vhp_planner_path, lib.vhp_planner_path_device, lib.vhp_planner_batch_paths, lib.vhp_planner_batch_paths_device,
             lib.vhp_planner_maps_batch_paths, lib.vhp_planner_maps_batch_paths_device]
    for call in calls:
        assert call(c.h, None, 0, None, None, None) == vhp.VHP_ERR_ARG
    c.set_map(occ)
    c.set_maps(occ[None])
    for call in calls:
        assert call(c.h, None, 0, None, None, None) == vhp.VHP_ERR_ARG
    c.planner_solve(c4[:2], c4[2:], 0.1, 250)
    c.planner_solve_batch([c4], 0.1, 250, outputs=False)
    c.planner_solve_maps_batch([c4], [0], 0.1, 250, outputs=False)
    for call in calls[::2]:
        assert call(c.h, None, 0, None, None, None) == vhp.VHP_OK
    c.set_map(occ)   # (drops the plain and the batch results; the maps batch is the stack's)
    assert [call(c.h, None, 0, None, None, None) for call in calls[::2]] == [vhp.VHP_ERR_ARG, vhp.VHP_ERR_ARG, vhp.VHP_OK]
    c.set_maps(occ[None])
    assert lib.vhp_planner_maps_batch_paths(c.h, None, 0, None, None, None) == vhp.VHP_ERR_ARG


def test_plain_and_speculative_solves(vhp, oracle):
    occ, c4 = _maze6()
    c = _ctx(vhp, occ)
    lib = c.lib
    start, end = c4[:2], c4[2:]
    orc = _oracle_paths(oracle, lambda q: occ, [c4], [0.1], 250)
    assert orc[0][0] == 0 and len(orc[0][1]) >= 3 and "%.6g" % orc[0][2] == "1529.55"
    solves = [("planner_solve", lambda: c.planner_solve(start, end, 0.1, 250), True),
              ("speculative exact k=4", lambda: c.planner_solve_speculative(start, end, 0.1, 250, k=4, mode=0), True),
              ("speculative fast k=4", lambda: c.planner_solve_speculative(start, end, 0.1, 250, k=4, mode=1), False),
              ("speculative fast k=4, max_iter 20", lambda: c.planner_solve_speculative(start, end, 0.1, 20, k=4, mode=1), False),
              ("planner_solve, max_iter 3", lambda: c.planner_solve(start, end, 0.1, 3), False)]
    for what, solve, exact in solves:
        r = solve()
        cap = r["n_pivots"] + 3
        want = [_old_route(vhp, r, end, cap)]
        got = _check(vhp, c, lib.vhp_planner_path, lib.vhp_planner_path_device, want, cap, what)
        if exact:
            _against_oracle(got, orc, what)
        if r["status"] == vhp.VHP_OK:
            assert got[0][0] == vhp.VHP_OK and got[0][1] >= 3, what
            p = c.planner_path()   # (the binding's default room: n_pivots + 2)
            assert (p["status"], _bits(p["length"]), p["path"].tolist()) == (want[0][0], want[0][2], want[0][3])
            small = [_old_route(vhp, r, end, want[0][1] - 1)]
            assert small[0][0] == vhp.VHP_ERR_TOO_LARGE
            _check(vhp, c, lib.vhp_planner_path, lib.vhp_planner_path_device, small, want[0][1] - 1, what + ", cap one too small")
    # planner_solve_device leaves the same state
    rc, npiv, _ = c.planner_solve_device(start, end, 0.1, 250)
    p = c.planner_path()
    assert rc == 0 and p["status"] == 0 and p["path"].tolist() == orc[0][1] and _bits(p["length"]) == _bits(orc[0][2])
    # a solve that fails validation: its code, no points
    bad = c.planner_solve((-1, 0), end, 0.1, 250)
    assert bad["status"] == vhp.VHP_ERR_START_OOB
    p = c.planner_path(cap=8)
    assert (p["status"], p["n_path"], p["length"], len(p["path"])) == (vhp.VHP_ERR_START_OOB, 0, 0.0, 0)


def _batch_case(vhp, oracle, c, occ, queries, thr, max_iter, what, cap=None, use_oracle=True):
    thr = np.broadcast_to(np.asarray(thr, np.float64), (len(queries),))
    res = c.planner_solve_batch(queries, thr, max_iter)
    lib = c.lib
    cap = max(r["n_pivots"] for r in res) + 3 if cap is None else cap
    want = [_old_route(vhp, r, q[2:], cap) if r["came_from"] is not None else (r["status"], 0, _bits(0.0), []) for r, q in zip(res, queries)]
    got = _check(vhp, c, lib.vhp_planner_batch_paths, lib.vhp_planner_batch_paths_device, want, cap, what)
    # the results call after the paths calls: the same bytes as before them
    for q in (0, len(queries) - 1):
        if res[q]["came_from"] is not None:
            came = np.empty((c.ny, c.nx), np.uint64)
            piv = np.zeros((res[q]["n_pivots"] + 1, 2), np.int32)
            c._check(lib.vhp_planner_batch_results(c.h, q, came.ctypes.data_as(C.c_void_p), None, None, piv.ctypes.data_as(C.c_void_p)))
            assert came.tobytes() == res[q]["came_from"].tobytes() and piv.tobytes() == res[q]["pivots"].tobytes(), (what, q)
    if use_oracle:
        orc = _oracle_paths(oracle, lambda q: occ, queries, thr, max_iter)
        _not_vacuous(orc)
        _against_oracle(got, orc, what)
    return res, got


@pytest.mark.parametrize("n_queries,group", [(1, 0), (5, 4), (32, 0), (64, 0)])
def test_maze6_batches(vhp, oracle, n_queries, group):
    occ, c4 = _maze6()
    c = _ctx(vhp, occ)
    if group:
        c.set_option("planner_batch_group", group)   # (more queries than one group)
    queries = [c4] + _free_pairs(occ, n_queries - 1, 7)
    res, got = _batch_case(vhp, oracle, c, occ, queries, 0.1, 250, "maze_6, Q = %d" % n_queries)
    assert got[0][0] == 0 and "%.6g" % struct.unpack("<d", bytes.fromhex(got[0][2]))[0] == "1529.55"
    # outputs="paths": the same paths, no field
    paths = c.planner_solve_batch(queries, 0.1, 250, outputs="paths")
    for q, p in enumerate(paths):
        assert sorted(p) == ["length", "n_pivots", "path", "path_status", "status"]
        assert (p["status"], p["n_pivots"]) == (res[q]["status"], res[q]["n_pivots"])
        if got[q][0] == 0:
            assert (p["path_status"], _bits(p["length"]), p["path"].tolist()) == (0, got[q][2], got[q][3]), q
    assert [(p["status"], p["path"].tolist()) for p in c.planner_batch_paths()] == [(g[0], g[3]) for g in got]


def test_batch_with_failed_validations_max_iter_and_small_cap(vhp, oracle):
    occ, c4 = _maze6()
    ny, nx = occ.shape
    by, bx = (int(v) for v in np.argwhere(occ == 0)[1000])
    pairs = _free_pairs(occ, 8, 7)
    queries = [c4, (-1, 5, c4[2], c4[3]), pairs[0], (c4[0], c4[1], nx, 3), (bx, by, c4[2], c4[3]), pairs[1], (c4[0], c4[1], bx, by)] + pairs[2:]
    c = _ctx(vhp, occ)
    res, got = _batch_case(vhp, oracle, c, occ, queries, 0.1, 250, "mixed batch", use_oracle=False)
    assert (got[1][0], got[3][0], got[4][0], got[6][0]) == (vhp.VHP_ERR_START_OOB, vhp.VHP_ERR_END_OOB,
                                                      vhp.VHP_ERR_START_OCCUPIED, vhp.VHP_ERR_END_OCCUPIED)
    assert all(got[q][1:] == (0, _bits(0.0), []) for q in (1, 3, 4, 6))
    # a cap that is too small for some queries only
    counts = sorted(g[1] for g in got if g[0] == 0)
    cap = counts[len(counts) // 2]
    assert counts[0] <= cap < counts[-1]
    _, small = _batch_case(vhp, oracle, c, occ, queries, 0.1, 250, "mixed batch, cap %d" % cap, cap=cap, use_oracle=False)
    assert {g[0] for g in small} >= {vhp.VHP_OK, vhp.VHP_ERR_TOO_LARGE}
    # max_iter 3: most queries run out of iterations and leave their end unlabelled
    res3, got3 = _batch_case(vhp, oracle, c, occ, queries, 0.1, 3, "mixed batch, max_iter 3", use_oracle=False)
    assert sum(r["status"] == vhp.VHP_ERR_MAX_ITER for r in res3) >= 4
    assert sum(g[0] == vhp.VHP_ERR_ARG for g in got3) >= 4


def _maps_case(vhp, oracle, stack, queries, idx, thr, max_iter, what):
    c = vhp.Context(0)
    c.set_maps(np.ascontiguousarray(stack, np.uint8))
    lib = c.lib
    thr = np.broadcast_to(np.asarray(thr, np.float64), (len(queries),))
    res = c.planner_solve_maps_batch(queries, idx, thr, max_iter)
    cap = max(r["n_pivots"] for r in res) + 3
    want = [_old_route(vhp, r, q[2:], cap) if r["came_from"] is not None else (r["status"], 0, _bits(0.0), []) for r, q in zip(res, queries)]
    got = _check(vhp, c, lib.vhp_planner_maps_batch_paths, lib.vhp_planner_maps_batch_paths_device, want, cap, what)
    orc = _oracle_paths(oracle, lambda q: stack[idx[q]], queries, thr, max_iter)
    _not_vacuous(orc)
    _against_oracle(got, orc, what)
    paths = c.planner_solve_maps_batch(queries, idx, thr, max_iter, outputs="paths")
    assert [(p["path_status"], p["path"].tolist()) for p in paths] == [(g[0], g[3]) for g in got]
    assert [(p["status"], p["path"].tolist()) for p in c.planner_maps_batch_paths()] == [(g[0], g[3]) for g in got]


def test_stack_of_64_random_maps(vhp, oracle):
    """DESIGN 7c case (b): 64 random 100 x 100 maps, (5, 5) -> (95, 95), threshold 0.25."""
    stack = []
    for seed in range(64):
        occ = maps.random_rect_map(100, 100, 25, 2, 20, 2, 20, seed=100 + seed)
        occ[5, 5] = occ[95, 95] = 1
        stack.append(occ)
    _maps_case(vhp, oracle, np.stack(stack), [(5, 5, 95, 95)] * 64, list(range(64)), 0.25, 250, "64 random maps")


@pytest.mark.parametrize("nx,ny", [(101, 77), (255, 130)])
def test_stack_with_repeated_and_unordered_indices_odd_widths(vhp, oracle, nx, ny):
    stack = np.stack([maps.random_rect_map(nx, ny, 20, 4, 30, 4, 30, 31 + k) for k in range(3)])
    idx = [2, 0, 0, 1, 2, 0, 1, 0]
    queries = [_free_pairs(stack[k], 8, 5)[q] for q, k in enumerate(idx)]   # (each query between free cells of its own map)
    _maps_case(vhp, oracle, stack, queries, idx, 0.2, 100, "%d x %d stack" % (nx, ny))
    # ... and the same width on one map
    c = _ctx(vhp, stack[0])
    _batch_case(vhp, oracle, c, stack[0], _free_pairs(stack[0], 8, 5), 0.2, 100, "%d x %d batch" % (nx, ny))


def test_1000_square(vhp, oracle):
    occ = maps.random_rect_map(1000, 1000, 15, 60, 200, 60, 200, seed=200)
    queries = _free_pairs(occ, 4, 4)
    c = _ctx(vhp, occ)
    _batch_case(vhp, oracle, c, occ, queries, 0.25, 60, "1000 x 1000, Q = 4")
