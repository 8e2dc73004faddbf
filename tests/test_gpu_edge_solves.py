"""The planner at the grid's edge, through every consumer of a solve (tests/edge_solves.py: the maps and cases, tests/test_edge_solves.py:
what the oracle gives for them; tests/test_planner_cell_cpu.py: the per-cell step the epilogues share, on the host).
Column 0 is swept only from a pivot with sx == 0 and row 0 only from one with sy == 0; a start on them is followed by pivots off them,
and from then on only planner_unswept keeps what the start's sweep left in a local field or a cache slot out of the union, the labels
and the pick.  A pivot on the border is also what takes push_rank's branch for empty quadrants.  The other planner tests start inside
the grid, on grids of 48 x 40 and more, at thresholds above 0.
Groups (edge_solves.py): T tiny grids below one wavefront of cells, every pair of free cells; W thin grids at the packed words' edges;
B productive solves from the corners of salt maps; Z threshold 0.0 on a serpentine, where the pivots are blocked cells.
Every exact solve is compared with the CPU oracle byte for byte (test_gpu_planner._assert_same_solution, with the first pivot that
differs); the paths, the length fields and the goal paths with the oracle's reconstruct_path on the oracle's arrays -- every point, and
the length as its float64 bits; the speculative solve's fast mode is held to test_gpu_long_solves' validity checks."""
import numpy as np
import pytest

import edge_solves as es
from test_gpu_long_solves import UNL32, _check_cut_plan, _device_results_equal, _fetch, _same
from test_gpu_planner_paths import _bits
from test_gpu_planner_paths import _check as _check_paths
from test_gpu_planner_tree import KINDS, _fields_device, _goals_device
from test_gpu_planner_tree import _same as _same_fields
from test_gpu_speculative import _check_valid_plan, _union_of_the_pivots_fields

pytestmark = pytest.mark.gpu

CHUNK = 64   # queries per batch call


@pytest.fixture(scope="module")
def vhp():
    import torch  # noqa: F401
    import vhp_amd
    return vhp_amd


def _ctx(vhp, occ, kernel=0):
    c = vhp.Context(0)
    c.set_map(np.ascontiguousarray(occ))
    if kernel:
        c.set_option("kernel", kernel)
    return c


def _orc(oracle, occ, q, thr, max_iter):
    return es.solve_on(oracle, occ, q[:2], q[2:], thr, max_iter)


# ---- what the path and tree calls must give, from the oracle's arrays alone

_walks = {}


def _oracle_walks(oracle, o):
    """(length float64 [ny, nx] with -1.0 where a cell has no label, n_path uint32 [ny, nx] with 0 there, {(x, y): points}) of an oracle
    solve: reconstruct_path from every labelled cell, computed once per process"""
    if id(o) not in _walks:
        came = o["came_from"]
        length = np.full(came.shape, -1.0, np.float64)
        cnt = np.zeros(came.shape, np.uint32)
        pts = {}
        for y, x in np.argwhere(came != es.UNL64):
            d, path = oracle.reconstruct_path(came, o["pivots"], (int(x), int(y)))
            length[y, x], cnt[y, x], pts[(int(x), int(y))] = d, len(path), path.tolist()
        _walks[id(o)] = (o, length, cnt, pts)   # (o itself: its id stays its own)
    return _walks[id(o)][1:]


def _want_goal(vhp, oracle, o, x, y):
    """(status, n_path, length bits, points) of the path to cell (x, y): the oracle's walk where the cell is labelled, else VHP_ERR_ARG"""
    length, cnt, pts = _oracle_walks(oracle, o)
    if (x, y) not in pts:
        return (vhp.VHP_ERR_ARG, 0, _bits(0.0), [])
    return (vhp.VHP_OK, int(cnt[y, x]), _bits(length[y, x]), pts[(x, y)])


def _tuple(p):
    return (p["status"], p["n_path"], _bits(p["length"]), p["path"].tolist())


def _check_consumers(vhp, oracle, c, solve, orc, queries, goal_cells, what, device_forms=False):
    """after a solve whose results equal orc: the path call at every query's end, the length fields at every cell, the goal paths at
    goal_cells of every query -- host forms, and the device forms (into buffers that start as NaN / -7) where asked for"""
    n = len(orc)
    ny, nx = orc[0]["came_from"].shape
    ends = [_want_goal(vhp, oracle, o, q[2], q[3]) for o, q in zip(orc, queries)]
    paths = {"plain": lambda: [c.planner_path()], "batch": c.planner_batch_paths, "maps": c.planner_maps_batch_paths}[solve]()
    assert [_tuple(p) for p in paths] == ends, what + ": paths to the ends"
    wl = np.stack([_oracle_walks(oracle, o)[0] for o in orc])
    wc = np.stack([_oracle_walks(oracle, o)[1] for o in orc])
    gl, gc = c.planner_length_fields(solve)
    _same_fields(gl, gc, wl, wc, what + ": length fields")
    goals = [(q, x, y) for q in range(n) for x, y in goal_cells]
    want = [_want_goal(vhp, oracle, orc[q], x, y) for q, x, y in goals]
    got = c.planner_goal_paths(goals, solve)
    for g, p, w in zip(goals, got, want):
        assert _tuple(p) == w, "%s: goal %r: %r vs the oracle's %r" % (what, g, _tuple(p)[:3], w[:3])
    if device_forms:
        lib = c.lib
        host, dev = {"plain": (lib.vhp_planner_path, lib.vhp_planner_path_device), "batch": (lib.vhp_planner_batch_paths, lib.vhp_planner_batch_paths_device),
                     "maps": (lib.vhp_planner_maps_batch_paths, lib.vhp_planner_maps_batch_paths_device)}[solve]
        cap = max(o["n_pivots"] for o in orc) + 3
        _check_paths(vhp, c, host, dev, ends, cap, what + ": paths, both forms")
        for shift in (0, 1):
            dl, dc = _fields_device(vhp, c, KINDS[solve], 0, n, nx, ny, shift=shift)
            _same_fields(dl, dc, wl, wc, "%s: length fields, device form, shift %d" % (what, shift))
        assert _goals_device(vhp, c, KINDS[solve], goals, cap) == want, what + ": goal paths, device form"
    return ends, want


def _all_cells(nx, ny):
    return [(x, y) for y in range(ny) for x in range(nx)]


def _cases_by_map(group):
    by = {}
    for name in es.case_names(group):
        by.setdefault(es.CASES[name]["map"], []).append(name)
    return by


# ---- a. the plain solve, under both kernel choices

@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("group", ["W", "B", "Z"])
def test_plain_solve(vhp, oracle, group, kernel):
    """every case of a group: status, pivots, came_from, vis_global and vis_local; then the path and tree calls on what it left"""
    for m, names in _cases_by_map(group).items():
        occ = es.map_of(m)
        c = _ctx(vhp, occ, kernel)
        nx, ny = occ.shape[1], occ.shape[0]
        for k, name in enumerate(names):
            case = es.CASES[name]
            got = c.planner_solve(case["start"], case["end"], case["thr"], case["max_iter"])
            assert c.last_sweep_kernel() == (1 if kernel else 4), name
            o = es.solve(oracle, name)
            _same(got, o, "case %s, kernel %d" % (name, kernel))
            assert (got["status"], got["n_pivots"]) == (case["status"], case["n_pivots"])
            _check_consumers(vhp, oracle, c, "plain", [o], [es.query(name)], es.border_cells(nx, ny), "case %s, kernel %d" % (name, kernel),
                             device_forms=k == 0)


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("nx,ny", es.T_PLAIN_GRIDS)
def test_plain_solve_tiny(vhp, oracle, nx, ny, kernel):
    """every pair of free cells of the all-free grid and of each grid with one blocked cell, thresholds 0.0 and 0.5"""
    counts = {}
    for k, occ in enumerate(es.t_maps(nx, ny)):
        c = _ctx(vhp, occ, kernel)
        for thr in es.T_THRESHOLDS:
            for j, q in enumerate(es.t_queries(occ)):
                got = c.planner_solve(q[:2], q[2:], thr, es.T_MAX_ITER)
                o = _orc(oracle, occ, q, thr, es.T_MAX_ITER)
                what = "%d x %d, map %d, query %r, threshold %g, kernel %d" % (nx, ny, k, q, thr, kernel)
                _same(got, o, what)
                assert c.last_sweep_kernel() == (1 if kernel else 4)
                n, ok, one, cut = counts.get(thr, (0, 0, 0, 0))
                counts[thr] = (n + 1, ok + (got["status"] == vhp.VHP_OK), one + (got["status"] == vhp.VHP_OK and got["n_pivots"] == 1),
                               cut + (got["status"] == vhp.VHP_ERR_MAX_ITER))
                if j % 7 == 0:
                    _check_consumers(vhp, oracle, c, "plain", [o], [q], _all_cells(nx, ny), what, device_forms=j == 0 and k < 2)
    for thr in es.T_THRESHOLDS:
        assert counts[thr] == es.T_COUNTS[(nx, ny, thr)]


@pytest.mark.parametrize("name", es.case_names("B") + es.case_names("Z"))
def test_plain_solve_device_results(vhp, oracle, name):
    case = es.CASES[name]
    o = es.solve(oracle, name)
    c = _ctx(vhp, es.map_of(case["map"]))
    rc, n_piv, ptr = c.planner_solve_device(case["start"], case["end"], case["thr"], case["max_iter"])
    assert (rc, n_piv) == (o["status"], o["n_pivots"]) == (case["status"], case["n_pivots"])
    assert c.last_sweep_kernel() == 4
    _device_results_equal(ptr, o, "case %s, device results" % name)
    assert int((_fetch(ptr["labels"], o["came_from"].shape, np.uint32) == UNL32).sum()) == int((o["came_from"] == vhp.UNLABELLED).sum())


# ---- b. the speculative solve, exact mode

@pytest.mark.parametrize("k", [2, 8])
@pytest.mark.parametrize("group", ["W", "B", "Z"])
def test_speculative_exact(vhp, oracle, group, k):
    for m, names in _cases_by_map(group).items():
        c = _ctx(vhp, es.map_of(m))
        for name in names:   # (one context per map: a case starts on the cache slots the one before it left)
            case = es.CASES[name]
            got = c.planner_solve_speculative(case["start"], case["end"], case["thr"], case["max_iter"], k=k, mode=0)
            assert c.last_sweep_kernel() == 4
            _same(got, es.solve(oracle, name), "case %s, exact mode, k=%d" % (name, k))


@pytest.mark.parametrize("k", [2, 8])
@pytest.mark.parametrize("m", ["B130x9", "B17x17", "B7x64"])
def test_speculative_slots_from_column_0_lit_to_unswept(vhp, oracle, m, k):
    """one context: a solve from (0, 0) -- the slots of its first pivot hold a lit row 0 and column 0 --, one whose pivots all lie off
    row 0 and column 0 -- the same slots, those cells now unswept --, and the first again"""
    c = _ctx(vhp, es.map_of(m))
    assert es.CASES[m + "_3"]["border"][:2] == (0, 0) and es.CASES[m + "_0"]["start"] == (0, 0)
    for rep, name in enumerate((m + "_0", m + "_3", m + "_0")):
        case = es.CASES[name]
        got = c.planner_solve_speculative(case["start"], case["end"], case["thr"], case["max_iter"], k=k, mode=0)
        _same(got, es.solve(oracle, name), "solve %d (%s) of the sequence, k=%d" % (rep, name, k))
        o = es.solve(oracle, name)
        nx, ny = o["came_from"].shape[1], o["came_from"].shape[0]
        _check_consumers(vhp, oracle, c, "plain", [o], [es.query(name)], es.border_cells(nx, ny), "solve %d (%s) of the sequence" % (rep, name))


# ---- c. the speculative solve, fast mode

@pytest.mark.parametrize("k", [2, 8])
@pytest.mark.parametrize("name", es.case_names("B"))
def test_speculative_fast(vhp, oracle, name, k):
    """the validity properties of test_gpu_long_solves.test_speculative_fast: a valid plan (or a cut one), and the union, the labels and
    the last local field are those of the oracle's sweeps of exactly the committed pivots, in commit order"""
    case = es.CASES[name]
    occ = es.map_of(case["map"])
    thr, max_iter = case["thr"], case["max_iter"]
    c = _ctx(vhp, occ)
    r = c.planner_solve_speculative(case["start"], case["end"], thr, max_iter, k=k, mode=1)
    assert c.last_sweep_kernel() == 4
    assert r["status"] in (vhp.VHP_OK, vhp.VHP_ERR_MAX_ITER)
    assert r["n_pivots"] <= max_iter + 8
    if r["status"] == vhp.VHP_OK:
        _check_valid_plan(vhp, occ, r, case["start"], case["end"], thr)
    else:
        _check_cut_plan(vhp, occ, r, case["start"])
    union, label, last = _union_of_the_pivots_fields(oracle, occ, r, thr, case["start"])
    assert np.array_equal(r["vis_global"], union)
    assert np.array_equal(r["vis_local"], last)
    got = np.where(r["came_from"] == vhp.UNLABELLED, -1, r["came_from"].astype(np.int64))
    assert np.array_equal(got, label), "%d labels differ" % int((got != label).sum())


# ---- d. the batch solve

def _batch_chunks(vhp, oracle, c, solve, solve_call, queries, thr, max_iter, occ_of, what, goal_cells, consumers_every=1):
    """queries in calls of up to CHUNK; each query against the oracle's solve; the path and tree calls after every consumers_every-th call.
    Returns the GPU results of all queries."""
    out = []
    for at in range(0, len(queries), CHUNK):
        qs = queries[at: at + CHUNK]
        res = solve_call(qs, at)
        orc = [_orc(oracle, occ_of(at + j), q, thr[at + j] if isinstance(thr, (list, tuple)) else thr, max_iter[at + j] if isinstance(max_iter, (list, tuple)) else max_iter)
               for j, q in enumerate(qs)]
        for j, (r, o) in enumerate(zip(res, orc)):
            _same(r, o, "%s, query %d %r" % (what, at + j, qs[j]))
        if (at // CHUNK) % consumers_every == 0:
            _check_consumers(vhp, oracle, c, solve, orc, qs, goal_cells, "%s, queries from %d" % (what, at), device_forms=at == 0)
        out += res
    return out


@pytest.mark.parametrize("group_opt", [1, 0])
@pytest.mark.parametrize("nx,ny", es.T_GRIDS)
def test_batch_tiny(vhp, oracle, nx, ny, group_opt):
    """group T in full: every pair of free cells of every map of a grid, both thresholds, planner_batch_group 1 and automatic; the
    all-free grid's queries also against the plain solve"""
    counts = {thr: [0, 0, 0, 0] for thr in es.T_THRESHOLDS}
    for k, occ in enumerate(es.t_maps(nx, ny)):
        c = _ctx(vhp, occ)
        c.set_option("planner_batch_group", group_opt)
        queries = es.t_queries(occ)
        for thr in es.T_THRESHOLDS if queries else ():   # (1 x 1 with its cell blocked has no query)
            what = "%d x %d, map %d, threshold %g, group %d" % (nx, ny, k, thr, group_opt)
            res = _batch_chunks(vhp, oracle, c, "batch", lambda qs, at: c.planner_solve_batch(qs, thr, es.T_MAX_ITER), queries, thr, es.T_MAX_ITER,
                                lambda q: occ, what, _all_cells(nx, ny), consumers_every=1 if group_opt == 0 else 4)
            assert c.last_sweep_kernel() == 4
            assert c.planner_batch_group() == 1 if group_opt else c.planner_batch_group() >= 1
            for r in res:
                counts[thr][0] += 1
                counts[thr][1] += r["status"] == vhp.VHP_OK
                counts[thr][2] += r["status"] == vhp.VHP_OK and r["n_pivots"] == 1
                counts[thr][3] += r["status"] == vhp.VHP_ERR_MAX_ITER
            if k == 0 or group_opt == 0:   # (every map under the automatic group, the all-free one under both)
                ref = _ctx(vhp, occ)
                for q, r in zip(queries, res):
                    _same(ref.planner_solve(q[:2], q[2:], thr, es.T_MAX_ITER), r, what + ": plain solve of %r vs the batch" % (q,))
    for thr in es.T_THRESHOLDS:
        assert tuple(counts[thr]) == es.T_COUNTS[(nx, ny, thr)]


@pytest.mark.parametrize("group_opt", [1, 0])
@pytest.mark.parametrize("group", ["W", "B", "Z"])
def test_batch(vhp, oracle, group, group_opt):
    """all queries of a map in one call (each under its own max_iter's call), against the oracle's solves and the plain solve's"""
    for m, names in _cases_by_map(group).items():
        occ = es.map_of(m)
        nx, ny = occ.shape[1], occ.shape[0]
        c = _ctx(vhp, occ)
        c.set_option("planner_batch_group", group_opt)
        ref = _ctx(vhp, occ)
        for max_iter in sorted({es.CASES[n]["max_iter"] for n in names}):
            # (a batch has one max_iter: the cut corner starts of a B map also run under the (0, 0) start's 200)
            queries = [es.query(n) for n in names]
            thr = es.CASES[names[0]]["thr"]
            what = "map %s, max_iter %d, group %d" % (m, max_iter, group_opt)
            res = _batch_chunks(vhp, oracle, c, "batch", lambda qs, at: c.planner_solve_batch(qs, thr, max_iter), queries, thr, max_iter, lambda q: occ, what,
                                es.border_cells(nx, ny))
            assert c.last_sweep_kernel() == 4
            if group_opt:
                assert c.planner_batch_group() == 1
            for n, q, r in zip(names, queries, res):
                if es.CASES[n]["max_iter"] == max_iter:
                    assert (r["status"], r["n_pivots"]) == (es.CASES[n]["status"], es.CASES[n]["n_pivots"]), n
                _same(ref.planner_solve(q[:2], q[2:], thr, max_iter), r, what + ": plain solve of %s vs the batch" % n)


# ---- e. the maps batch

@pytest.mark.parametrize("nx,ny", es.T_GRIDS)
def test_maps_batch_tiny(vhp, oracle, nx, ny):
    """the all-free grid and each one-blocked-cell variant as one stack; every query of every map, shuffled across the maps"""
    stack = es.t_maps(nx, ny)
    c = vhp.Context(0)
    c.set_maps(stack)
    pairs = [(k, q) for k in range(len(stack)) for q in es.t_queries(stack[k])]
    order = np.random.default_rng(nx * 100 + ny).permutation(len(pairs))
    pairs = [pairs[i] for i in order]
    queries, idx = [p[1] for p in pairs], [p[0] for p in pairs]
    for thr in es.T_THRESHOLDS:
        what = "maps batch %d x %d, threshold %g" % (nx, ny, thr)
        res = _batch_chunks(vhp, oracle, c, "maps", lambda qs, at: c.planner_solve_maps_batch(qs, idx[at: at + len(qs)], thr, es.T_MAX_ITER), queries, thr,
                            es.T_MAX_ITER, lambda q: stack[idx[q]], what, _all_cells(nx, ny), consumers_every=2)
        assert c.last_sweep_kernel() == 4
        n_ok = sum(r["status"] == vhp.VHP_OK for r in res)
        n_one = sum(r["status"] == vhp.VHP_OK and r["n_pivots"] == 1 for r in res)
        n_cut = sum(r["status"] == vhp.VHP_ERR_MAX_ITER for r in res)
        assert (len(res), n_ok, n_one, n_cut) == es.T_COUNTS[(nx, ny, thr)]


def _transposed(name):
    """a case's query on its map's transpose"""
    sx, sy, ex, ey = es.query(name)
    return (sy, sx, ey, ex)


@pytest.mark.parametrize("members", [("B130x9", "B9x130"), ("B9x130", "B130x9"), ("B17x17", "B17x17"), ("B65x13", None), ("B7x64", None)])
def test_maps_batch_border_solves(vhp, oracle, members):
    """the B maps of one size as a stack: a map, and the transpose of the map whose transposed size agrees; the four corner queries of
    each (transposed on the transposed map), shuffled across the maps, in one call per max_iter"""
    own, other = members
    maps_ = [np.ascontiguousarray(es.map_of(own))] + ([np.ascontiguousarray(es.map_of(other).T)] if other else [])
    assert all(m.shape == maps_[0].shape for m in maps_)
    stack = np.stack(maps_)
    ny, nx = stack.shape[1:]
    c = vhp.Context(0)
    c.set_maps(stack)
    pairs = [(0, es.query(n), es.CASES[n]) for n in es.case_names("B") if es.CASES[n]["map"] == own]
    if other:
        pairs += [(1, _transposed(n), None) for n in es.case_names("B") if es.CASES[n]["map"] == other]
    order = np.random.default_rng(len(own) + nx).permutation(len(pairs))
    pairs = [pairs[i] for i in order]
    queries, idx = [p[1] for p in pairs], [p[0] for p in pairs]
    ref = vhp.Context(0)
    for max_iter in (es.B_MAX_ITER_CUT, es.B_MAX_ITER):
        what = "maps batch of %s and %s transposed, max_iter %d" % (own, other, max_iter)
        res = _batch_chunks(vhp, oracle, c, "maps", lambda qs, at: c.planner_solve_maps_batch(qs, idx[at: at + len(qs)], es.B_THRESHOLD, max_iter), queries,
                            es.B_THRESHOLD, max_iter, lambda q: stack[idx[q]], what, es.border_cells(nx, ny))
        assert c.last_sweep_kernel() == 4
        for (k, q, case), r in zip(pairs, res):
            if case is not None and case["max_iter"] == max_iter:
                assert (r["status"], r["n_pivots"]) == (case["status"], case["n_pivots"])
        for k in range(len(stack)):   # ... and the plain solve on set_map(that map)
            ref.set_map(stack[k])
            for (kk, q, _), r in zip(pairs, res):
                if kk == k:
                    _same(ref.planner_solve(q[:2], q[2:], es.B_THRESHOLD, max_iter), r, what + ": plain solve of %r on map %d vs the maps batch" % (q, k))
