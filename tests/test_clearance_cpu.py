"""The clearance field of vhp_map_clearance / vhp_maps_clearance, without a GPU: csrc/vhp_clearance.hpp -- the per-line distance and
the combining scan that vhp_clearance_stack runs for every cell -- run by tests/clearance_driver.cpp.  clearance_cell on both packed
copies (the column-packed one with x and y exchanged must give the transposed field) is held three ways: to the definition evaluated
cell by cell in the driver, to the numpy field of clearance_cases.clearance here, and to the inflation: (clearance > p) must be
inflate_cases.inflate(p) for every p of clearance_cases.witness_ps -- a statement written without any notion of a distance.
Border off and on.  Sides: inflate_cases.SIDES x SIDES for the p_max of reach up to 3; each of the six p_max of reach 63 and 64 takes
four size pairs, chosen so that every side is a width and a height under at least two of them.  The driver is a stand-alone program,
built plain and under the address and undefined-behaviour sanitizers (a shift by 64, a count of zeros of 0, a read outside the packed
copies are theirs to catch), and every case runs through both."""
import functools
import os
import subprocess

import numpy as np
import pytest

import clearance_cases as cc
import cpu_driver
import inflate_cases as ic
import window_cases as wc


def _large_pairs(i):
    """the size pairs of large p_max i: sides 2i and 2i + 1 of SIDES against sides 2i + 5 and 2i + 6, both ways round"""
    s, n = cc.SIDES, len(cc.SIDES)
    pairs = [(s[(2 * i + j) % n], s[(2 * i + 5 + j) % n]) for j in (0, 1)]
    return pairs + [(b, a) for a, b in pairs]


def p_max_for(nx, ny):
    return cc.SMALL + tuple(f for i, f in enumerate(cc.LARGE) if (nx, ny) in _large_pairs(i))


@pytest.fixture(scope="module", params=["plain", "san"])
def driver(request, tmp_path_factory):
    san = request.param == "san"
    return cpu_driver.build(os.path.join(cpu_driver.HERE, "clearance_driver.cpp"), str(tmp_path_factory.mktemp("clearance")),
                            "clearance_driver_" + request.param, flags=() if san else ("-O2",), sanitized=san)


@functools.lru_cache(maxsize=None)
def _cases(nx, ny):
    """(maps [M, ny, nx], [(shape, p_max, border)], the fields [case, M, ny, nx]) -- computed once, shared by both builds of the
    driver; every field is held to the inflation here, before any driver is"""
    stack = np.stack([m for _, m in cc.case_maps(nx, ny, seed=1000 * nx + ny)])
    todo = [(s, p, b) for s, p in p_max_for(nx, ny) for b in (0, 1)]
    fields = []
    for s, p_max, b in todo:
        field = cc.clearance(stack, s, p_max, bool(b))
        for p in cc.witness_ps(s, p_max):
            assert np.array_equal(field > p, ic.inflate(stack, s, p, bool(b)) != 0), (nx, ny, s, p_max, b, p)
        fields.append(field)
    return stack, todo, np.stack(fields)


def test_large_p_max_see_every_side():
    assert len(cc.LARGE) == 6 and {ic.reach(*f) for f in cc.LARGE} == {63, 64} and all(ic.reach(*f) <= 3 for f in cc.SMALL)
    for axis in (0, 1):
        seen = [pair[axis] for i in range(len(cc.LARGE)) for pair in _large_pairs(i)]
        assert all(seen.count(side) >= 2 for side in cc.SIDES), (axis, seen)
        assert all(len(_large_pairs(i)) == 4 for i in range(len(cc.LARGE)))
    assert set(cc.witness_ps(cc.DISC, 4224)) == {0, 1, 2, 8, 9, 3969, 4096, 4224} and cc.witness_ps(cc.SQUARE, 3) == [0, 1, 2, 3]


def test_reference_is_the_definition():
    """the numpy field on cases small enough to write down"""
    one = np.ones((5, 7), np.uint8)
    one[2, 3] = 0
    F = cc.FAR
    assert cc.clearance(one, cc.DISC, 0).tolist() == np.where(one == 0, 0, F).tolist()
    disc = cc.clearance(one, cc.DISC, 5)
    assert disc[:, 1:6].tolist() == [[F, 5, 4, 5, F], [5, 2, 1, 2, 5], [4, 1, 0, 1, 4], [5, 2, 1, 2, 5], [F, 5, 4, 5, F]]
    assert disc[:, 0].tolist() == [F, F, F, F, F] and disc[:, 6].tolist() == [F, F, F, F, F]
    assert cc.clearance(one, cc.SQUARE, 2)[:, 1:6].tolist() == [[2, 2, 2, 2, 2], [2, 1, 1, 1, 2], [2, 1, 0, 1, 2], [2, 1, 1, 1, 2], [2, 2, 2, 2, 2]]
    assert cc.clearance(one, cc.DIAMOND, 2)[:, 1:6].tolist() == [[F, F, 2, F, F], [F, 2, 1, 2, F], [2, 1, 0, 1, 2], [F, 2, 1, 2, F], [F, F, 2, F, F]]
    free = np.ones((4, 6), np.uint8)
    assert (cc.clearance(free, cc.DISC, 4224) == F).all()                       # the edge is no wall ...
    ring = cc.clearance(free, cc.SQUARE, 64, border=True)                        # ... unless asked for
    assert ring.tolist() == [[1] * 6, [1, 2, 2, 2, 2, 1], [1, 2, 2, 2, 2, 1], [1] * 6]
    assert cc.clearance(free, cc.DISC, 3, border=True).tolist() == [[1] * 6, [1, F, F, F, F, 1], [1, F, F, F, F, 1], [1] * 6]
    assert (cc.clearance(np.full((3, 3), 7, np.uint8), cc.DISC, 9) == F).all()   # (any non-zero byte is free)
    assert not cc.clearance(np.zeros((3, 3), np.uint8), cc.DIAMOND, 64).any()


def test_refused_p_max(driver):
    p = subprocess.run([driver, "refuse"], capture_output=True, check=False)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])


def _run(driver, tmp_path, stack, nx, ny, todo):
    path = os.path.join(str(tmp_path), "packed_%dx%d.bin" % (nx, ny))
    with open(path, "wb") as f:
        for m in stack:
            f.write(wc.pack_lines(m).astype("<u8").tobytes())
            f.write(wc.pack_lines(m.T).astype("<u8").tobytes())
    p = subprocess.run([driver, "cells", path, str(nx), str(ny), str(len(stack))], input="".join("%d %d %d\n" % t for t in todo).encode(),
                       capture_output=True, check=False)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    got = np.frombuffer(p.stdout, "<u2")
    assert got.size == len(todo) * len(stack) * 2 * nx * ny
    got = got.reshape(len(todo), len(stack), 2, nx * ny)
    return got[:, :, 0].reshape(len(todo), len(stack), ny, nx), got[:, :, 1].reshape(len(todo), len(stack), nx, ny)


@pytest.mark.parametrize("ny", cc.SIDES)
@pytest.mark.parametrize("nx", cc.SIDES)
def test_clearance_cell_equals_numpy(driver, tmp_path, nx, ny):
    stack, todo, want = _cases(nx, ny)
    by_rows, by_cols = _run(driver, tmp_path, stack, nx, ny, todo)
    names = [name for name, _ in cc.case_maps(nx, ny, seed=1000 * nx + ny)]
    for i, (s, p_max, b) in enumerate(todo):
        for k, name in enumerate(names):   # name the first case that differs
            what = "map %s of %d x %d, shape %d p_max %d border %d" % (name, nx, ny, s, p_max, b)
            assert np.array_equal(by_rows[i, k], want[i, k]), what + ": the row-packed copy"
            assert np.array_equal(by_cols[i, k], want[i, k].T), what + ": the column-packed copy, x and y exchanged"


def test_the_check_has_teeth(driver, tmp_path):
    """on this map neighbouring p_max, the shapes and the border flag all give different fields"""
    occ = wc.random_map(65, 64, seed=5, blocked=0.02)
    todo = [(cc.DISC, 1, 0), (cc.DISC, 2, 0), (cc.DISC, 2, 1), (cc.DIAMOND, 2, 0), (cc.SQUARE, 2, 0)]
    by_rows, _ = _run(driver, tmp_path, occ[None], 65, 64, todo)
    assert len({g.tobytes() for g in by_rows}) == len(todo)
