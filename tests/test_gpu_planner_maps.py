"""The batch planner across a stack of maps (vhp_planner_solve_maps_batch): query q on map map_idx[q] gives exactly what set_map(that
map) + planner_solve gives (checked on a second context) and what the CPU oracle gives -- status, pivot count, pivots, labels, union
and last local field, bit for bit --, whatever the grouping, and its state is its own."""
import ctypes as C

import numpy as np
import pytest

import maps
from test_gpu_planner_batch import _assert_same, _edge_queries, _free_pairs, _maze6_config4, _solved

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vhp():
    import torch  # noqa: F401
    import vhp_amd
    return vhp_amd


@pytest.fixture(scope="module")
def ref(vhp):
    """the second context: set_map + planner_solve per query"""
    return vhp.Context(0)


def _stack_ctx(vhp, stack):
    c = vhp.Context(0)
    c.set_maps(np.ascontiguousarray(stack, np.uint8))
    return c


def _plain(ref, stack, queries, idx, thr, max_iter):
    """planner_solve of every query on its own map (one set_map per map)"""
    out = [None] * len(queries)
    for k in sorted(set(int(v) for v in idx)):
        ref.set_map(stack[k])
        for q in range(len(queries)):
            if int(idx[q]) == k:
                sx, sy, ex, ey = (int(v) for v in queries[q])
                out[q] = ref.planner_solve((sx, sy), (ex, ey), float(thr[q]), max_iter)
    return out


def _check(vhp, oracle, ref, c, stack, queries, idx, thr, max_iter, use_oracle=True):
    """One maps batch against set_map + planner_solve per query and against the oracle; returns the batch's results."""
    thr = np.broadcast_to(np.asarray(thr, np.float64), (len(queries),))
    got = c.planner_solve_maps_batch(queries, idx, thr, max_iter)
    want = _plain(ref, stack, queries, idx, thr, max_iter)
    for q, (sx, sy, ex, ey) in enumerate(np.asarray(queries).tolist()):
        what = "query %d %r on map %d thr %g" % (q, (sx, sy, ex, ey), idx[q], thr[q])
        _assert_same(got[q], want[q], what + " vs set_map + planner_solve", vhp)
        if thr[q] > 1.0:
            assert got[q]["status"] == vhp.VHP_ERR_NOTHING_LIT, what
        elif use_oracle and _solved(got[q], vhp):
            _assert_same(got[q], oracle.solve(stack[idx[q]], (sx, sy), (ex, ey), float(thr[q]), max_iter), what + " vs oracle", vhp)
    return got


def _random_stack(n, nx, ny, seed):
    return np.stack([maps.random_rect_map(nx, ny, 22, 4, 30, 4, 30, seed + k) for k in range(n)])


def test_random_stack_edge_queries(vhp, oracle, ref):
    """16 random 160 x 131 maps, test_gpu_planner_batch's twelve kinds of edge query spread over them, and free pairs on every map."""
    stack = _random_stack(16, 160, 131, 40)
    queries, idx, thr = [], [], []
    for i in range(12):
        m = (5 * i + 3) % 16 if i != 7 else idx[6]   # (the repeated query: on the same map as its twin)
        qs, ts = _edge_queries(stack[m], 7 + m)
        queries.append(qs[i])
        idx.append(m)
        thr.append(ts[i])
    for m in range(16):
        queries += _free_pairs(stack[m], 1, 50 + m)
        idx.append(m)
        thr.append((0.1, 0.25, 0.5)[m % 3])
    c = _stack_ctx(vhp, stack)
    got = _check(vhp, oracle, ref, c, stack, queries, idx, thr, 60)
    st = [r["status"] for r in got]
    assert st[0] == vhp.VHP_OK and got[0]["n_pivots"] == 1
    assert st[1] == vhp.VHP_OK
    assert st[2] == vhp.VHP_OK and got[2]["n_pivots"] == 0
    assert st[3] == vhp.VHP_ERR_NOTHING_LIT
    assert st[4] == vhp.VHP_ERR_START_OOB and st[5] == vhp.VHP_ERR_END_OCCUPIED and st[11] == vhp.VHP_ERR_END_OOB
    for name in ("came_from", "vis_global", "vis_local", "pivots"):
        assert got[6][name].tobytes() == got[7][name].tobytes()
    assert c.last_sweep_kernel() == 4
    # a max_iter that ends some queries while others finish
    got = _check(vhp, oracle, ref, c, stack, queries, idx, thr, 1)
    st = [r["status"] for r in got]
    assert vhp.VHP_ERR_MAX_ITER in st and st[0] == vhp.VHP_OK, st


def _maze6_stack():
    occ, c4 = _maze6_config4()
    ny, nx = occ.shape
    variants = [occ]
    rng = np.random.default_rng(6)
    for k in range(3):   # (maze_6 with walls of its own: a few blocked rectangles, start and end kept free)
        v = occ.copy()
        for _ in range(4 + 2 * k):
            x, y = int(rng.integers(0, nx - 40)), int(rng.integers(0, ny - 40))
            v[y: y + int(rng.integers(3, 40)), x: x + int(rng.integers(3, 40))] = 0
        v[c4[1], c4[0]] = v[c4[3], c4[2]] = 1
        variants.append(v)
    return np.stack(variants), c4


def test_maze6_in_a_stack(vhp, oracle, ref):
    stack, c4 = _maze6_stack()
    queries, idx = [c4, c4, c4, c4], [0, 1, 2, 3]
    for m in range(4):
        queries += _free_pairs(stack[m], 3, 70 + m)
        idx += [m] * 3
    thr = [0.1] * 4 + [0.25, 0.1, 0.5] * 4
    c = _stack_ctx(vhp, stack)
    got = _check(vhp, oracle, ref, c, stack, queries, idx, thr, 250)
    assert got[0]["status"] == vhp.VHP_OK and got[0]["n_pivots"] == 64
    d, _ = vhp.reconstruct_path(got[0]["came_from"], got[0]["pivots"], c4[2:])
    assert "%.6g" % d == "1529.55"
    assert c.last_sweep_kernel() == 4
    assert c.planner_maps_batch_group() >= 16


def test_one_wall_changes_the_result(vhp, ref):
    """Non-vacuity: the same query on two maps that differ by one wall gives two results, each its own map's."""
    occ = maps.random_rect_map(160, 131, 22, 4, 30, 4, 30, 9)
    sx, sy, ex, ey = _free_pairs(occ, 1, 3)[0]
    a = occ.copy()
    a[max(0, sy - 4): sy + 5, sx + 1: sx + 4] = 1
    a[sy, sx] = a[ey, ex] = 1
    b = a.copy()
    b[max(0, sy - 4): sy + 5, sx + 2] = 0   # (a wall right beside the start: it changes what the first sweep lights)
    b[sy, sx] = b[ey, ex] = 1
    stack = np.stack([a, b])
    c = _stack_ctx(vhp, stack)
    q = [(sx, sy, ex, ey)] * 2
    got = c.planner_solve_maps_batch(q, [0, 1], 0.25, 60)
    want = _plain(ref, stack, q, [0, 1], [0.25, 0.25], 60)
    for k in range(2):
        _assert_same(got[k], want[k], "map %d" % k, vhp)
    assert got[0]["vis_global"].tobytes() != got[1]["vis_global"].tobytes()


def test_identical_stack_equals_the_one_map_batch(vhp):
    occ = maps.random_rect_map(160, 131, 22, 4, 30, 4, 30, 12)
    queries = _free_pairs(occ, 8, 21)
    thr = [0.25, 0.1, 0.5, 0.05, 0.25, 0.1, 0.5, 0.25]
    one = vhp.Context(0)
    one.set_map(occ)
    want = one.planner_solve_batch(queries, thr, 60)
    c = _stack_ctx(vhp, np.stack([occ] * len(queries)))
    for idx in (list(range(len(queries))), [0] * len(queries)):
        got = c.planner_solve_maps_batch(queries, idx, thr, 60)
        for q in range(len(queries)):
            _assert_same(got[q], want[q], "idx %r query %d" % (idx[:2], q), vhp)


def test_grouping_never_changes_a_result(vhp, oracle, ref):
    stack = _random_stack(5, 160, 131, 60)
    queries, idx = [], []
    for m in range(5):
        queries += _free_pairs(stack[m], 4, 80 + m)
        idx += [m] * 4
    thr = [(0.25, 0.1, 0.5, 0.05)[k % 4] for k in range(len(queries))]
    c = _stack_ctx(vhp, stack)
    runs = {}
    for group in (1, 3, 0):
        c.set_option("planner_batch_group", group)
        runs[group] = c.planner_solve_maps_batch(queries, idx, thr, 60)
        if group:
            assert c.planner_maps_batch_group() == group
    assert c.planner_maps_batch_group() >= 16
    c.set_option("kernel", 1)   # (the front sweep: one query at a time, on its own map)
    runs["fronts"] = c.planner_solve_maps_batch(queries, idx, thr, 60)
    assert c.last_sweep_kernel() == 1 and c.planner_maps_batch_group() == 1
    for key, got in runs.items():
        for q in range(len(queries)):
            _assert_same(got[q], runs[0][q], "group %r query %d" % (key, q), vhp)
    c.set_option("kernel", 0)
    _check(vhp, oracle, ref, c, stack, queries, idx, thr, 60, use_oracle=False)


def test_width_not_a_multiple_of_8(vhp, oracle, ref):
    stack = np.stack([maps.random_rect_map(1001, 971, 15, 60, 200, 60, 200, 3 + k) for k in range(4)])
    queries, idx = [], []
    for m in range(4):
        queries += _free_pairs(stack[m], 2, 5 + m)
        idx += [m, m]
    c = _stack_ctx(vhp, stack)
    _check(vhp, oracle, ref, c, stack, queries, idx, [0.25, 0.5] * 4, 8)
    assert c.last_sweep_kernel() == 4


def test_side_above_1024_two_workgroups_per_unit(vhp, ref):
    """1300 x 1100: lat_halves gives the build whose bands read across workgroups (two workgroups per unit)."""
    stack = np.stack([maps.random_rect_map(1300, 1100, 15, 60, 200, 60, 200, 30 + k) for k in range(2)])
    queries = _free_pairs(stack[0], 2, 1) + _free_pairs(stack[1], 2, 2)
    idx, thr = [0, 0, 1, 1], [0.25, 0.5, 0.25, 0.1]
    c = _stack_ctx(vhp, stack)
    got = c.planner_solve_maps_batch(queries, idx, thr, 5)
    assert c.last_sweep_kernel() == 4
    want = _plain(ref, stack, queries, idx, thr, 5)
    for q in range(4):
        _assert_same(got[q], want[q], "query %d" % q, vhp)


def _reader(vhp):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def fetch(p, shape, dtype):
        a = np.empty(shape, dtype)
        assert hip.hipMemcpy(a.ctypes.data, p, a.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        return a

    def read(ptr, n_piv, ny, nx):
        return [fetch(ptr["labels"], (ny, nx), np.uint32), fetch(ptr["vis_global"], (ny, nx), np.float64),
                fetch(ptr["vis_local"], (ny, nx), np.float64), fetch(ptr["pivots"], (n_piv + 1, 2), np.int32)]
    return read


def test_state_isolation(vhp, ref):
    read = _reader(vhp)
    occ, c4 = _maze6_config4()
    ny, nx = occ.shape
    c = vhp.Context(0)
    c.set_map(occ)
    rc, n_piv, ptr = c.planner_solve_device(c4[:2], c4[2:], 0.1, 250)
    assert rc == 0 and n_piv == 64
    plain_before = read(ptr, n_piv, ny, nx)
    batch = c.planner_solve_batch([c4] + _free_pairs(occ, 3, 3), 0.25, 250)
    group_before = c.planner_batch_group()
    batch_before = read(c.planner_batch_results_device(0), batch[0]["n_pivots"], ny, nx)
    # a maps batch leaves the plain solve's and the one-map batch's device results alone
    stack = _random_stack(3, 160, 131, 90)
    c.set_maps(stack)
    qs = _free_pairs(stack[1], 2, 4) + _free_pairs(stack[2], 1, 5)
    got = c.planner_solve_maps_batch(qs, [1, 1, 2], 0.25, 60)
    p = [C.c_void_p() for _ in range(4)]
    assert c.lib.vhp_planner_results_device(c.h, *[C.byref(v) for v in p]) == vhp.VHP_OK
    after = read(dict(labels=p[0].value, vis_global=p[1].value, vis_local=p[2].value, pivots=p[3].value), n_piv, ny, nx)
    for a, b in zip(plain_before, after):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(batch_before, read(c.planner_batch_results_device(0), batch[0]["n_pivots"], ny, nx)):
        assert a.tobytes() == b.tobytes()
    assert c.planner_batch_group() == group_before
    # ... and its device arrays are its own: query 0
    mine = read(c.planner_maps_batch_results_device(0), got[0]["n_pivots"], 131, 160)
    lab = mine[0].astype(np.uint64)
    lab[lab == 0xFFFFFFFF] = vhp.UNLABELLED
    assert lab.tobytes() == got[0]["came_from"].tobytes()
    assert mine[1].tobytes() == got[0]["vis_global"].tobytes() and mine[2].tobytes() == got[0]["vis_local"].tobytes()
    assert mine[3].tobytes() == got[0]["pivots"].tobytes()
    # vhp_set_map leaves the maps batch's results valid
    c.set_map(maps.random_rect_map(64, 48, 4, 3, 9, 3, 9, 2))
    for a, b in zip(mine, read(c.planner_maps_batch_results_device(0), got[0]["n_pivots"], 131, 160)):
        assert a.tobytes() == b.tobytes()
    assert c.lib.vhp_planner_maps_batch_results(c.h, 2, None, None, None, None) == vhp.VHP_OK
    # vhp_set_maps ends them, and the next batch builds the new stack's diagonal maps
    stack2 = _random_stack(2, 120, 97, 95)
    c.set_maps(stack2)
    assert c.lib.vhp_planner_maps_batch_results(c.h, 0, None, None, None, None) == vhp.VHP_ERR_ARG
    assert c.lib.vhp_planner_maps_batch_results_device(c.h, 0, None, None, None, None) == vhp.VHP_ERR_ARG
    assert c.planner_maps_batch_group() == 0
    qs2 = _free_pairs(stack2[0], 2, 6) + _free_pairs(stack2[1], 2, 7)
    got2 = c.planner_solve_maps_batch(qs2, [0, 0, 1, 1], 0.25, 60)
    assert c.last_sweep_kernel() == 4
    want2 = _plain(ref, stack2, qs2, [0, 0, 1, 1], [0.25] * 4, 60)
    for q in range(4):
        _assert_same(got2[q], want2[q], "new stack, query %d" % q, vhp)


def test_error_paths(vhp):
    c = vhp.Context(0)
    lib = c.lib
    q = np.array([[1, 1, 5, 5]] * 65, np.int32)
    idx = np.zeros(65, np.int32)
    thr = np.full(65, 0.25)
    st = np.zeros(65, np.int32)
    npiv = np.zeros(65, np.uint32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.vhp_planner_solve_maps_batch(c.h, P(q), P(idx), P(thr), 1, 10, P(st), P(npiv)) == vhp.VHP_ERR_NO_MAP
    c.set_map(maps.random_rect_map(64, 48, 4, 3, 9, 3, 9, 2))   # (a single map is no stack)
    assert lib.vhp_planner_solve_maps_batch(c.h, P(q), P(idx), P(thr), 1, 10, P(st), P(npiv)) == vhp.VHP_ERR_NO_MAP
    stack = np.stack([maps.random_rect_map(64, 48, 4, 3, 9, 3, 9, s) for s in (2, 3)])
    c.set_maps(stack)
    # no maps batch yet: no results
    assert lib.vhp_planner_maps_batch_results(c.h, 0, None, None, None, None) == vhp.VHP_ERR_ARG
    assert lib.vhp_planner_maps_batch_results_device(c.h, 0, None, None, None, None) == vhp.VHP_ERR_ARG
    assert c.planner_maps_batch_group() == 0
    assert lib.vhp_planner_solve_maps_batch(c.h, P(q), P(idx), P(thr), 0, 10, P(st), P(npiv)) == vhp.VHP_ERR_ARG
    assert lib.vhp_planner_solve_maps_batch(c.h, P(q), P(idx), P(thr), 65, 10, P(st), P(npiv)) == vhp.VHP_ERR_ARG
    assert lib.vhp_planner_solve_maps_batch(c.h, P(q), P(idx), P(thr), 2, (1 << 24) + 1, P(st), P(npiv)) == vhp.VHP_ERR_ARG
    for k in range(5):
        args = [P(q), P(idx), P(thr), P(st), P(npiv)]
        args[k] = None
        assert lib.vhp_planner_solve_maps_batch(c.h, args[0], args[1], args[2], 2, 10, args[3], args[4]) == vhp.VHP_ERR_ARG
    for bad in (-1, 2):
        idx[1] = bad
        assert lib.vhp_planner_solve_maps_batch(c.h, P(q), P(idx), P(thr), 2, 10, P(st), P(npiv)) == vhp.VHP_ERR_ARG
    idx[1] = 0
    with pytest.raises(ValueError):
        c.planner_solve_maps_batch(q[:3], idx[:2], 0.25, 10)
    qs = _free_pairs(stack[0], 2, 4) + [(-1, 0, 3, 3)]
    got = c.planner_solve_maps_batch(qs, [0, 1, 1], 0.25, 10)
    assert got[2]["status"] == vhp.VHP_ERR_START_OOB
    assert lib.vhp_planner_maps_batch_results(c.h, 2, None, None, None, None) == vhp.VHP_ERR_ARG   # (failed validation)
    assert lib.vhp_planner_maps_batch_results(c.h, 3, None, None, None, None) == vhp.VHP_ERR_ARG
    assert lib.vhp_planner_maps_batch_results(c.h, -1, None, None, None, None) == vhp.VHP_ERR_ARG
    assert lib.vhp_planner_maps_batch_results_device(c.h, 2, None, None, None, None) == vhp.VHP_ERR_ARG
    assert lib.vhp_planner_maps_batch_results(c.h, 0, None, None, None, None) == vhp.VHP_OK
