"""The batch planner (vhp_planner_solve_batch): every query of a batch gives exactly what vhp_planner_solve gives for it alone and
what the CPU oracle gives -- status, pivot count, pivots, labels, union and last local field, bit for bit --, whatever the grouping."""
import ctypes as C

import numpy as np
import pytest

import maps

pytestmark = pytest.mark.gpu

THRESHOLDS = (0.05, 0.1, 0.25, 0.5)


@pytest.fixture(scope="module")
def vhp():
    import torch  # noqa: F401
    import vhp_amd
    return vhp_amd


def _ctx(vhp, occ):
    c = vhp.Context(0)
    c.set_map(occ)
    return c


def _solved(r, vhp):
    return r["status"] in (vhp.VHP_OK, vhp.VHP_ERR_MAX_ITER, vhp.VHP_ERR_NOTHING_LIT)


def _assert_same(got, want, what, vhp):
    """got: a batch result; want: planner_solve's or the oracle's for the same query."""
    assert got["status"] == want["status"], "%s: status %d vs %d" % (what, got["status"], want["status"])
    assert got["n_pivots"] == want["n_pivots"], "%s: %d pivots vs %d" % (what, got["n_pivots"], want["n_pivots"])
    assert got["pivots"].tobytes() == want["pivots"].tobytes(), what + ": pivots differ"
    if not _solved(got, vhp):
        assert got["came_from"] is None and got["vis_global"] is None and got["vis_local"] is None
        return
    for name in ("came_from", "vis_global", "vis_local"):
        a, b = got[name], want[name]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name)
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a != b)
            y, x = bad[0]
            raise AssertionError("%s: %s differs in %d cells, first (x=%d,y=%d): %r vs %r" % (what, name, len(bad), x, y, a[y, x], b[y, x]))


def _check_batch(vhp, oracle, c, occ, queries, thr, max_iter, use_oracle=True):
    """One batch against planner_solve per query (same context) and against the oracle; returns the batch's results."""
    got = c.planner_solve_batch(queries, thr, max_iter)
    thr = np.broadcast_to(np.asarray(thr, np.float64), (len(queries),))
    for q, (sx, sy, ex, ey) in enumerate(np.asarray(queries).tolist()):
        what = "query %d %r thr %g" % (q, (sx, sy, ex, ey), thr[q])
        plain = c.planner_solve((sx, sy), (ex, ey), float(thr[q]), max_iter)
        _assert_same(got[q], plain, what + " vs planner_solve", vhp)
        if thr[q] > 1.0:
            # (nothing reaches such a threshold: the reference's top() of an empty heap, whatever its build makes of that)
            assert got[q]["status"] == vhp.VHP_ERR_NOTHING_LIT, what
        elif use_oracle and _solved(got[q], vhp):   # (the validation codes: planner_solve's, pinned against the oracle in test_gpu_planner.py)
            _assert_same(got[q], oracle.solve(occ, (sx, sy), (ex, ey), float(thr[q]), max_iter), what + " vs oracle", vhp)
    return got


def _free_pairs(occ, n, seed):
    pts = maps.free_sources(occ, 2 * n, seed)
    return [tuple(int(v) for v in pts[2 * k]) + tuple(int(v) for v in pts[2 * k + 1]) for k in range(n)]


def _maze6_config4():
    occ = maps.maze_6()
    ny = occ.shape[0]
    return occ, (345, ny - 1 - 391, 341, ny - 1 - 10)   # BASELINE config 4 (mode 2 flips y)


def test_maze6_sixteen_queries(vhp, oracle):
    occ, c4 = _maze6_config4()
    queries = [c4] + _free_pairs(occ, 15, 7)
    rng = np.random.default_rng(11)
    thr = [0.1] + [float(t) for t in rng.choice(THRESHOLDS, 15)]
    c = _ctx(vhp, occ)
    got = _check_batch(vhp, oracle, c, occ, queries, thr, 250)
    assert got[0]["status"] == vhp.VHP_OK and got[0]["n_pivots"] == 64
    c.planner_solve_batch(queries, thr, 250, outputs=False)
    assert c.last_sweep_kernel() == 4   # (the batch's iterations: the latency sweep)
    assert c.planner_batch_group() >= 16
    # paths of three queries, against the oracle's
    n_paths = 0
    for q in range(len(queries)):
        if got[q]["status"] != vhp.VHP_OK or n_paths == 3:
            continue
        end = queries[q][2:]
        want = oracle.solve(occ, queries[q][:2], end, thr[q], 250)
        d, path = vhp.reconstruct_path(got[q]["came_from"], got[q]["pivots"], end)
        dw, pathw = oracle.reconstruct_path(want["came_from"], want["pivots"], end)
        assert d == dw and path.tolist() == pathw.tolist(), "query %d" % q
        n_paths += 1
    assert n_paths == 3


def test_maze6_single_query_equals_planner_solve(vhp, oracle):
    occ, c4 = _maze6_config4()
    c = _ctx(vhp, occ)
    got = c.planner_solve_batch([c4], 0.1, 250)[0]
    want = c.planner_solve(c4[:2], c4[2:], 0.1, 250)
    _assert_same(got, want, "config 4 alone", vhp)
    assert c.planner_batch_group() >= 1 and c.last_sweep_kernel() == 4


def _edge_queries(occ, seed):
    """Twelve queries of the kinds a batch must keep apart: the returned list is (queries, thresholds)."""
    ny, nx = occ.shape
    free = np.argwhere(occ[1:-1, 1:-1] & occ[1:-1, 2:])   # (a free cell with a free right neighbour: it sees it in one sweep)
    y0, x0 = (int(v) + 1 for v in free[len(free) // 3])
    blocked = np.argwhere(occ == 0)
    by, bx = (int(v) for v in blocked[len(blocked) // 2])
    pairs = _free_pairs(occ, 6, seed + 100)
    queries = [
        (x0, y0, x0 + 1, y0),           # the end lit by the first sweep: done after one iteration
        (x0, y0, x0, y0),               # start == end
        pairs[0],                       # negative threshold: the loop never runs
        pairs[1],                       # threshold above 1: nothing is ever lit
        (-1, pairs[2][1], pairs[2][2], pairs[2][3]),   # start out of bounds
        (pairs[2][0], pairs[2][1], bx, by),            # end occupied
        pairs[3], pairs[3],             # the same query twice
        pairs[4], pairs[5], pairs[2],
        (pairs[4][0], pairs[4][1], nx, 0),             # end out of bounds
    ]
    thr = [0.25, 0.25, -0.5, 1.5, 0.25, 0.25, 0.25, 0.25, 0.5, 0.1, 0.25, 0.25]
    return queries, thr


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_random_maps_edge_queries(vhp, oracle, seed):
    occ = maps.random_rect_map(160, 131, 22, 4, 30, 4, 30, seed)
    queries, thr = _edge_queries(occ, seed)
    c = _ctx(vhp, occ)
    got = _check_batch(vhp, oracle, c, occ, queries, thr, 60)
    st = [r["status"] for r in got]
    assert st[0] == vhp.VHP_OK and got[0]["n_pivots"] == 1
    assert st[1] == vhp.VHP_OK
    assert st[2] == vhp.VHP_OK and got[2]["n_pivots"] == 0
    assert st[3] == vhp.VHP_ERR_NOTHING_LIT
    assert st[4] == vhp.VHP_ERR_START_OOB and st[5] == vhp.VHP_ERR_END_OCCUPIED and st[11] == vhp.VHP_ERR_END_OOB
    for name in ("came_from", "vis_global", "vis_local", "pivots"):
        assert got[6][name].tobytes() == got[7][name].tobytes()
    # a max_iter that ends some queries while others finish
    got = _check_batch(vhp, oracle, c, occ, queries, thr, 1)
    st = [r["status"] for r in got]
    assert vhp.VHP_ERR_MAX_ITER in st and st[0] == vhp.VHP_OK, st


def test_grouping_never_changes_a_result(vhp, oracle):
    occ = maps.random_rect_map(160, 131, 22, 4, 30, 4, 30, 1)
    queries, thr = _edge_queries(occ, 1)
    queries = queries + _free_pairs(occ, 8, 33)
    thr = thr + [0.25, 0.1, 0.5, 0.05, 0.25, 0.1, 0.5, 0.05]
    c = _ctx(vhp, occ)
    runs = {}
    for group in (1, 3, 0):
        c.set_option("planner_batch_group", group)
        runs[group] = c.planner_solve_batch(queries, thr, 60)
        if group:
            assert c.planner_batch_group() == group
    assert c.planner_batch_group() >= 16
    # ... nor does the front sweep (the loop where the latency sweep does not take one source)
    c.set_option("planner_batch_group", 0)
    c.set_option("kernel", 1)
    runs["fronts"] = c.planner_solve_batch(queries, thr, 60)
    assert c.last_sweep_kernel() == 1 and c.planner_batch_group() == 1
    for key, got in runs.items():
        for q in range(len(queries)):
            _assert_same(got[q], runs[0][q], "group %r query %d" % (key, q), vhp)
    c.set_option("kernel", 0)
    _check_batch(vhp, oracle, c, occ, queries, thr, 60, use_oracle=False)


def test_width_not_a_multiple_of_8(vhp, oracle):
    occ = maps.random_rect_map(1001, 971, 15, 60, 200, 60, 200, 3)
    queries = _free_pairs(occ, 8, 5)
    thr = [0.25, 0.5, 0.25, 0.1, 0.5, 0.25, 0.5, 0.25]
    c = _ctx(vhp, occ)
    _check_batch(vhp, oracle, c, occ, queries, thr, 40)


def test_batch_leaves_the_plain_solve_alone(vhp):
    import torch  # noqa: F401
    occ, c4 = _maze6_config4()
    ny, nx = occ.shape
    c = _ctx(vhp, occ)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def fetch(p, shape, dtype):
        a = np.empty(shape, dtype)
        assert hip.hipMemcpy(a.ctypes.data, p, a.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        return a

    def read(ptr, n_piv):
        return [fetch(ptr["labels"], (ny, nx), np.uint32), fetch(ptr["vis_global"], (ny, nx), np.float64),
                fetch(ptr["vis_local"], (ny, nx), np.float64), fetch(ptr["pivots"], (n_piv + 1, 2), np.int32)]

    rc, n_piv, ptr = c.planner_solve_device(c4[:2], c4[2:], 0.1, 250)
    assert rc == 0 and n_piv == 64
    before = read(ptr, n_piv)
    got = c.planner_solve_batch([c4] + _free_pairs(occ, 5, 3), 0.25, 250)
    p = [C.c_void_p() for _ in range(4)]
    assert c.lib.vhp_planner_results_device(c.h, *[C.byref(v) for v in p]) == vhp.VHP_OK
    after = read(dict(labels=p[0].value, vis_global=p[1].value, vis_local=p[2].value, pivots=p[3].value), n_piv)
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()
    # ... and the batch's device arrays are the batch's: query 0 at threshold 0.25
    dev = read(c.planner_batch_results_device(0), got[0]["n_pivots"])
    lab = dev[0].astype(np.uint64)
    lab[lab == 0xFFFFFFFF] = vhp.UNLABELLED
    assert lab.tobytes() == got[0]["came_from"].tobytes()
    assert dev[1].tobytes() == got[0]["vis_global"].tobytes() and dev[2].tobytes() == got[0]["vis_local"].tobytes()
    assert dev[3].tobytes() == got[0]["pivots"].tobytes()


def test_error_paths(vhp):
    c = vhp.Context(0)
    lib = c.lib
    q = np.array([[1, 1, 5, 5]] * 65, np.int32)
    thr = np.full(65, 0.25)
    st = np.zeros(65, np.int32)
    npiv = np.zeros(65, np.uint32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.vhp_planner_solve_batch(c.h, P(q), P(thr), 1, 10, P(st), P(npiv)) == vhp.VHP_ERR_NO_MAP
    c.set_map(maps.random_rect_map(64, 48, 4, 3, 9, 3, 9, 2))
    # no batch yet: no results
    assert lib.vhp_planner_batch_results(c.h, 0, None, None, None, None) == vhp.VHP_ERR_ARG
    assert lib.vhp_planner_batch_results_device(c.h, 0, None, None, None, None) == vhp.VHP_ERR_ARG
    assert lib.vhp_planner_solve_batch(c.h, P(q), P(thr), 0, 10, P(st), P(npiv)) == vhp.VHP_ERR_ARG
    assert lib.vhp_planner_solve_batch(c.h, P(q), P(thr), 65, 10, P(st), P(npiv)) == vhp.VHP_ERR_ARG
    assert lib.vhp_planner_solve_batch(c.h, P(q), P(thr), 2, (1 << 24) + 1, P(st), P(npiv)) == vhp.VHP_ERR_ARG
    for k in range(4):
        args = [P(q), P(thr), P(st), P(npiv)]
        args[k] = None
        assert lib.vhp_planner_solve_batch(c.h, args[0], args[1], 2, 10, args[2], args[3]) == vhp.VHP_ERR_ARG
    occ = maps.random_rect_map(64, 48, 4, 3, 9, 3, 9, 2)
    qs = _free_pairs(occ, 3, 4)
    got = c.planner_solve_batch(qs, 0.25, 10)
    assert lib.vhp_planner_batch_results(c.h, 3, None, None, None, None) == vhp.VHP_ERR_ARG
    assert lib.vhp_planner_batch_results(c.h, -1, None, None, None, None) == vhp.VHP_ERR_ARG
    assert lib.vhp_planner_batch_results_device(c.h, 3, None, None, None, None) == vhp.VHP_ERR_ARG
    assert lib.vhp_planner_batch_results(c.h, 2, None, None, None, None) == vhp.VHP_OK
    assert all(_solved(r, vhp) for r in got)
    # a new map ends the batch's results
    c.set_map(occ)
    assert lib.vhp_planner_batch_results(c.h, 0, None, None, None, None) == vhp.VHP_ERR_ARG
    assert c.planner_batch_group() == 0
    with pytest.raises(vhp.VhpError):
        c.set_option("planner_batch_group", 33)
