"""What tests/edge_solves.py says about its maps and solves, pinned with the CPU oracle alone -- no GPU.  The GPU tests of
test_gpu_edge_solves.py reach the planner's behaviour at the grid's edge only because these numbers are what they are: if a change to a
generator or to the oracle turns a border solve into one that never leaves row 0, or a blocked pivot into a free one, this file fails
before a GPU test passes for the wrong reason.
It also runs every step of the productive border solves and of the threshold-0 solves through the stand-alone CPU driver of the
per-cell step (tests/planner_cell_driver.cpp, plain and sanitized, as test_planner_cell_cpu.py builds it), with 1.0 in every cell the
step's pivot does not sweep."""
import zlib

import numpy as np
import pytest

import edge_solves as es
import planner_cell_lib as pcl


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    return pcl.build_drivers(str(tmp_path_factory.mktemp("edge_planner_cell_driver")))


@pytest.mark.parametrize("name", sorted(es.MAPS))
def test_maps(name):
    m = es.MAPS[name]
    occ = es.map_of(name)
    assert occ.shape == (m["ny"], m["nx"]) and occ.dtype == np.uint8
    assert zlib.crc32(occ.tobytes()) == m["crc"], "%s: crc32 %08x" % (name, zlib.crc32(occ.tobytes()))
    assert int(occ.sum()) == m["n_free"]
    assert all(occ[y, x] == 1 for x, y in es.corners(m["nx"], m["ny"]))
    if m["kind"] == "salt_w":
        assert all(occ[y, x] == 1 for x, y in es.mid_borders(m["nx"], m["ny"]))
    assert np.array_equal(es.map_of("Z9x9t"), es.map_of("Z9x9").T)


def test_sizes_are_the_awkward_ones():
    assert {max(s) for s in es.W_SIZES} == {63, 64, 65, 129} and {min(s) for s in es.W_SIZES} == {1, 2, 3}   # around the 64-bit words
    assert all(nx * ny < 64 for nx, ny in es.T_GRIDS)   # less than one wavefront of cells, let alone one epilogue workgroup's 512 threads
    assert set(es.T_PLAIN_GRIDS) == {g for g in es.T_GRIDS if max(g) <= 7}
    assert sorted((es.MAPS[m]["nx"], es.MAPS[m]["ny"]) for m in es.MAPS if m[0] == "B") == [(7, 64), (9, 130), (17, 17), (65, 13), (130, 9)]


@pytest.mark.parametrize("nx,ny", es.T_GRIDS)
def test_tiny_grids(oracle, nx, ny):
    for thr in es.T_THRESHOLDS:
        n = ok = one = cut = 0
        for occ in es.t_maps(nx, ny):
            for q in es.t_queries(occ):
                r = es.solve_on(oracle, occ, q[:2], q[2:], thr, es.T_MAX_ITER)
                assert r["status"] in (es.OK, es.MAX_ITER)
                n += 1
                ok += r["status"] == es.OK
                one += r["status"] == es.OK and r["n_pivots"] == 1
                cut += r["status"] == es.MAX_ITER
                if r["status"] == es.MAX_ITER:
                    assert r["n_pivots"] == es.T_MAX_ITER + 1
        assert (n, ok, one, cut) == es.T_COUNTS[(nx, ny, thr)], (nx, ny, thr, (n, ok, one, cut))
        assert n == sum(int(occ.sum()) ** 2 for occ in es.t_maps(nx, ny))


def test_every_status_class_occurs_in_the_tiny_grids():
    """solved after one pivot, solved after several, cut by max_iter -- on the grids the plain solve runs and on all of them"""
    for grids in (es.T_PLAIN_GRIDS, es.T_GRIDS):
        n, ok, one, cut = (sum(es.T_COUNTS[(nx, ny, thr)][k] for nx, ny in grids for thr in es.T_THRESHOLDS) for k in range(4))
        assert one > 0 and ok - one > 0 and cut > 0 and ok + cut == n
    assert sum(v[0] for v in es.T_COUNTS.values()) == 24752


@pytest.mark.parametrize("name", sorted(es.CASES))
def test_cases(oracle, name):
    c = es.CASES[name]
    occ = es.map_of(c["map"])
    r = es.solve(oracle, name)
    piv = r["pivots"]
    assert r["status"] == c["status"]
    assert r["n_pivots"] == c["n_pivots"] and len(piv) == c["n_pivots"] + 1
    assert len({(int(x), int(y)) for x, y in piv}) == c["distinct"]
    assert es.border_counts(r) == c["border"]
    later = piv[1:-1] if r["status"] == es.OK else piv[1:]
    assert sum(int(occ[y, x] == 0) for x, y in later.tolist()) == c["blocked"]
    assert tuple(piv[0]) == c["start"] and occ[c["start"][1], c["start"][0]] == 1 and occ[c["end"][1], c["end"][0]] == 1
    ex, ey = c["end"]
    if c["thr"] > 0.0:
        assert (r["came_from"][ey, ex] != es.UNL64) == (c["status"] == es.OK)
    elif c["status"] == es.MAX_ITER:   # threshold 0.0 labels a dark end where it is swept (v >= 0); the loop goes on while its value is <= 0
        assert r["vis_global"][ey, ex] == 0.0
    if c["status"] == es.MAX_ITER:
        assert c["n_pivots"] == c["max_iter"] + 1
    if name[0] == "W":
        assert (c["start"], c["end"]) in es.w_queries(occ.shape[1], occ.shape[0])


def test_the_case_table_is_complete():
    for nx, ny in es.W_SIZES:
        names = [n for n in es.CASES if es.CASES[n]["map"] == "W%dx%d" % (nx, ny)]
        assert [(es.CASES[n]["start"], es.CASES[n]["end"]) for n in names] == es.w_queries(nx, ny)
    for m in es.MAPS:
        if m[0] == "B":
            nx, ny = es.MAPS[m]["nx"], es.MAPS[m]["ny"]
            assert [es.CASES["%s_%d" % (m, k)]["start"] for k in range(4)] == es.corners(nx, ny)
            assert all(es.CASES["%s_%d" % (m, k)]["end"] == (nx - 1 - s[0], ny - 1 - s[1]) for k, s in enumerate(es.corners(nx, ny)))
    assert len(es.case_names("W")) == 52 and len(es.case_names("B")) == 20 and len(es.case_names("Z")) == 25


def test_what_the_gpu_tests_rely_on(oracle):
    cases = es.CASES
    # B: only the start (0, 0) sees its end; the other three corners are cut, because an end on row 0 / column 0 is never lit from off it
    for m in ("B130x9", "B9x130", "B65x13", "B7x64", "B17x17"):
        assert [cases["%s_%d" % (m, k)]["status"] for k in range(4)] == [es.OK, es.MAX_ITER, es.MAX_ITER, es.MAX_ITER]
        c = cases[m + "_0"]
        r = es.solve(oracle, m + "_0")
        piv = r["pivots"][: r["n_pivots"]]
        assert len({tuple(p) for p in piv.tolist()}) == c["n_pivots"] >= 15, "productive: every pivot a new cell"
        assert c["border"][0] == 1 and c["border"][1] == 1, "the start alone lies on column 0 and on row 0 ..."
        assert c["border"][2] + c["border"][3] >= 2, "... and later pivots on the far borders"
        # the stale-field hazard: the last pivot is off row 0 and column 0, so its sweep leaves them alone, while the start's lit them
        assert not r["vis_local"][:, 0].any() and not r["vis_local"][0, :].any()
        assert r["vis_global"][:, 0].any() and r["vis_global"][0, :].any()
        assert (r["came_from"][0, :] == 0).sum() + (r["came_from"][:, 0] == 0).sum() >= 3   # labelled by the start, by nobody else
        assert set(r["came_from"][0, :].tolist()) <= {0, es.UNL64} and set(r["came_from"][:, 0].tolist()) <= {0, es.UNL64}
    assert [cases[m + "_0"]["n_pivots"] for m in ("B130x9", "B9x130", "B65x13", "B7x64", "B17x17")] == [47, 57, 30, 31, 15]
    # pivots AFTER the start on row 0 or column 0: no B case has one, and no productive solve can.  Row 0 is pushed only by a pivot on row 0,
    # whose sweep leaves 1.0 or 0.0 there (an axis copies its neighbour's value), while scale * g outweighs the distances: any lit cell
    # off the axes with g < 1 is picked before a cell of row 0.  Where every lit cell holds 1.0 the start's own cell wins (d_parent = 0,
    # and d_end(c) + d(c, start) >= d_end(start); on equality the start is pushed first) and the solve repeats it.  So the condition is
    # met by the thin grids and the serpentines, where a later pivot's own d_parent > 0 lets a neighbour on the border win
    on_later = [n for n, c in cases.items() if c["border"][0] + c["border"][1] > (c["start"][0] == 0) + (c["start"][1] == 0)]
    assert not [n for n in on_later if n[0] == "B"]
    assert {"W64x1_0", "W1x65_1", "W63x2_1", "W65x3_6", "Z9x9_1", "Z9x9t_3"} <= set(on_later)
    # ... and one that then leaves it: the start on row 0 and column 0, two more cells visited
    assert cases["W63x2_0"]["distinct"] == 3 and cases["W65x3_0"]["distinct"] == 5 and cases["W3x65_2"]["distinct"] == 5
    # Z: at threshold 0.0 every pivot after the start is a blocked cell (in six queries all but one)
    cut = [c for n, c in cases.items() if n.startswith("Z9x9") and c["status"] == es.MAX_ITER]
    assert len(cut) == 20 and all(c["blocked"] >= 40 for c in cut) and sum(c["blocked"] == 41 for c in cut) == 14
    assert cases["Z9x9_1"]["blocked"] == 41 == cases["Z9x9_1"]["n_pivots"]
    assert (cases["Z130x9_0"]["status"], cases["Z130x9_0"]["n_pivots"]) == (es.OK, 2)
    # a case whose pivots all lie off row 0 and column 0, for the speculative solve's slot sequence
    assert cases["B130x9_3"]["border"][:2] == (0, 0) and cases["B17x17_3"]["border"][:2] == (0, 0)


@pytest.mark.parametrize("name", ["B130x9_0", "B9x130_0", "B65x13_0", "B7x64_0", "B17x17_0", "B17x17_1", "W63x2_0", "W65x3_0", "W3x65_2",
                                  "Z9x9_1", "Z9x9_2", "Z9x9t_0", "Z9x9t_9", "Z130x9_0"])
def test_every_step_through_the_cell_driver(oracle, drivers, name):
    """the oracle's solve replayed step by step: each step's pivot, the state the oracle left before it, 1.0 in the cells it does not
    sweep; the driver's pick is the next pivot of the list"""
    c = es.CASES[name]
    occ = np.ascontiguousarray(es.map_of(c["map"]))
    r = es.solve(oracle, name)
    steps, came, vg = pcl.replay(oracle, occ, c["start"], c["end"], c["thr"], r)
    got = pcl.compare(oracle, drivers, steps)
    last = r["n_pivots"] - (1 if r["status"] == es.OK else 0)   # (a solved query's last entry is `end`, not the pick)
    assert [g[0] for g in got[:last]] == [tuple(p) for p in r["pivots"][1: last + 1].tolist()]
    assert came.tobytes() == r["came_from"].tobytes() and vg.tobytes() == r["vis_global"].tobytes()
