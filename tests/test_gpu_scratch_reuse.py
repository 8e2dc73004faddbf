"""One context driven through a growing, shrinking and regrowing sequence of calls gives what fresh state gives: the grow-only
scratch of the context, the planner states and the path, tree and queue scratch (csrc/vhp_devbuf.hpp buffers, all of them) are
REUSED here, where the other GPU tests mostly make a context per case.

Map A (96 x 80), then map B (131 x 77: an odd width, another cell count), then A again; on each the small calls and then the larger
ones (on the last A the small ones only), every call on the same context:
  host and device sweeps of 1 source, then 9 (the front sweep's order scratch: n_src >= 8), then 3, each under four option sets -- the
    default, the front sweep in rounds of 64 rows against sides of 96 and 131 (the round scratch), the pool sweep, the latency sweep;
  the queue variant's sweep of 1 source, then 3;
  planner_solve with max_iter 4, then 40, then 4 (the pivot list grows and is then reused);
  planner_solve_batch and, on a stack of 3 maps, planner_solve_maps_batch of 2 queries, then 5, then 2;
  after each solve planner_path / planner_[maps_]batch_paths, planner_length_fields and planner_goal_paths.
Sweeps and solves are held to the oracle bit for bit; the path, tree and queue calls to the same call after the same solve on a
fresh Context (their parity with the oracle on fresh contexts is test_gpu_planner_paths.py's, test_gpu_planner_tree.py's and
test_gpu_planner.py's).  Failed allocations are tests/test_devbuf.py's, on the CPU: nothing here provokes one."""
import numpy as np
import pytest

import maps

pytestmark = pytest.mark.gpu

THR = 0.5
GRIDS = {"A": (96, 80, 31), "B": (131, 77, 47)}   # nx, ny, seed
OPTION_SETS = [dict(), dict(kernel=1, rows_per_lane=1, strips=1, multi_round=1), dict(kernel=3), dict(kernel=4)]
SWEPT_BY = [4, 1, 3, 4]   # vhp_last_sweep_kernel under each (tests/golden/kernel_choice.json's rules: these batches take the latency sweep)
SMALL = dict(sources=[1], queue=[1], max_iter=[4], queries=[2])
LARGER = dict(sources=[9, 3], queue=[3], max_iter=[40, 4], queries=[5, 2])
SEQUENCE = [("A", [SMALL, LARGER]), ("B", [SMALL, LARGER]), ("A", [SMALL])]


@pytest.fixture(scope="module")
def vhp():
    import torch  # noqa: F401  (first, so the extension shares torch's HIP runtime)
    import vhp_amd
    return vhp_amd


def _stack(name):
    """Three maps of grid `name`; the first is the single map of set_map."""
    nx, ny, seed = GRIDS[name]
    return np.stack([maps.random_rect_map(nx, ny, 40, 3, 20, 3, 20, seed + 17 * k) for k in range(3)])


def _queries(stack, on):
    """One query (sx, sy, ex, ey) per entry of `on`, the map it runs on: between two free cells of that map."""
    pts = [maps.free_sources(m, 2 * len(on), 5 + k).tolist() for k, m in enumerate(stack)]
    return [tuple(pts[k].pop(0)) + tuple(pts[k].pop(0)) for k in on]


def _same_arrays(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d elements differ, first at %r: %r vs %r" % (what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def _same_solve(got, want, what):
    assert (got["status"], got["n_pivots"]) == (want["status"], want["n_pivots"]), "%s: status, pivots %r vs %r" % (
        what, (got["status"], got["n_pivots"]), (want["status"], want["n_pivots"]))
    for name in ("pivots", "came_from", "vis_global", "vis_local"):
        _same_arrays(got[name], want[name], "%s: %s" % (what, name))


def _same_paths(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g["status"], g["n_path"]) == (w["status"], w["n_path"]) and np.float64(g["length"]).tobytes() == np.float64(w["length"]).tobytes(), \
            "%s row %d: %r vs %r" % (what, k, (g["status"], g["n_path"], g["length"]), (w["status"], w["n_path"], w["length"]))
        assert g["path"].tolist() == w["path"].tolist(), "%s row %d: points differ" % (what, k)


def _goals(stack_or_occ, n_queries):
    """Per query three goals (q, x, y) on free cells of the first map."""
    occ = stack_or_occ if stack_or_occ.ndim == 2 else stack_or_occ[0]
    cells = maps.free_sources(occ, 3, 77)
    return np.array([(q, int(x), int(y)) for q in range(n_queries) for x, y in cells], np.int32)


def _after_solve(c, solve, n_queries, goals_on):
    """The path and tree calls that read a solve's state: (paths, length fields, point counts, goal paths)."""
    paths = [c.planner_path()] if solve == "plain" else c.planner_batch_paths() if solve == "batch" else c.planner_maps_batch_paths()
    length, count = c.planner_length_fields(solve=solve)
    return paths, length, count, c.planner_goal_paths(_goals(goals_on, n_queries), solve=solve)


def _same_after_solve(got, want, what):
    _same_paths(got[0], want[0], what + ": paths")
    _same_arrays(got[1], want[1], what + ": length fields")
    _same_arrays(got[2], want[2], what + ": point counts")
    _same_paths(got[3], want[3], what + ": goal paths")


def _device_sweep(torch, c, src, shape):
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    d_src = torch.from_numpy(src).cuda()
    d_out = torch.full((len(src),) + shape, -1.0, dtype=torch.float64, device="cuda")
    c.sweep_batch_device(d_src.data_ptr(), len(src), d_out.data_ptr())
    c.sync()
    c.set_stream(None)
    return d_out.cpu().numpy()


def test_one_context_reused_gives_what_fresh_state_gives(vhp, oracle):
    import torch
    stacks = {name: _stack(name) for name in GRIDS}
    memo = {}

    def once(key, make):
        if key not in memo:
            memo[key] = make()
        return memo[key]

    def fresh(name):
        f = vhp.Context(0)
        f.set_map(stacks[name][0])
        f.set_maps(stacks[name])
        return f

    solved = set()
    c = vhp.Context(0)
    for stage, (name, phases) in enumerate(SEQUENCE):
        stack = stacks[name]
        occ = stack[0]
        c.set_map(occ)
        c.set_maps(stack)
        sources = maps.free_sources(occ, 9, 3)
        for phase in phases:
            # the sweeps: host and device form, under each option set
            for n in phase["sources"]:
                src = np.ascontiguousarray(sources[:n])
                want = once(("sweep", name, n), lambda: np.stack([oracle.sweep_full(occ, int(x), int(y)) for x, y in src]))
                for options, kernel in zip(OPTION_SETS, SWEPT_BY):
                    what = "stage %d map %s, %d sources, options %r" % (stage, name, n, options)
                    for key in ("kernel", "rows_per_lane", "strips", "multi_round"):
                        c.set_option(key, options.get(key, 0))
                    _same_arrays(c.sweep_batch(src), want, what + ", host form")
                    assert c.last_sweep_kernel() == kernel, what
                    _same_arrays(_device_sweep(torch, c, src, occ.shape), want, what + ", device form")
                    assert c.last_sweep_kernel() == kernel, what
            for key in ("kernel", "rows_per_lane", "strips", "multi_round"):
                c.set_option(key, 0)
            for n in phase["queue"]:
                src = np.ascontiguousarray(sources[:n])
                want = once(("queue", name, n), lambda: fresh(name).sweep_batch(src, variant=vhp.SWEEP_QUEUE))
                _same_arrays(c.sweep_batch(src, variant=vhp.SWEEP_QUEUE), want, "stage %d map %s, queue sweep of %d" % (stage, name, n))
            # the plain solve, and what reads its state
            (query,) = _queries(stack, [0])
            for max_iter in phase["max_iter"]:
                what = "stage %d map %s, planner_solve max_iter %d" % (stage, name, max_iter)
                want = once(("solve", name, max_iter), lambda: oracle.solve(occ, query[:2], query[2:], THR, max_iter))
                _same_solve(c.planner_solve(query[:2], query[2:], THR, max_iter), want, what)
                solved.add(want["status"])

                def fresh_plain():
                    f = fresh(name)
                    f.planner_solve(query[:2], query[2:], THR, max_iter)
                    return _after_solve(f, "plain", 1, occ)
                _same_after_solve(_after_solve(c, "plain", 1, occ), once(("plain after", name, max_iter), fresh_plain), what)
            # the batches on the single map and on the stack
            for n in phase["queries"]:
                for solve in ("batch", "maps"):
                    what = "stage %d map %s, %s solve of %d queries" % (stage, name, solve, n)
                    on = [0] * n if solve == "batch" else [q % 3 for q in range(n)]
                    queries = _queries(stack, on)
                    got = c.planner_solve_batch(queries, THR, 40) if solve == "batch" else c.planner_solve_maps_batch(queries, on, THR, 40)
                    for q in range(n):
                        want = once(("solve", name, on[q], queries[q]), lambda: oracle.solve(stack[on[q]], queries[q][:2], queries[q][2:], THR, 40))
                        _same_solve(got[q], want, "%s, query %d" % (what, q))

                    def fresh_batch():
                        f = fresh(name)
                        if solve == "batch":
                            f.planner_solve_batch(queries, THR, 40, outputs=False)
                        else:
                            f.planner_solve_maps_batch(queries, on, THR, 40, outputs=False)
                        return _after_solve(f, solve, n, stack)
                    _same_after_solve(_after_solve(c, solve, n, stack), once((solve + " after", name, n), fresh_batch), what)
    # (not vacuous: the short solves ran out of iterations, the long ones arrived)
    assert solved == {vhp.VHP_OK, vhp.VHP_ERR_MAX_ITER}
