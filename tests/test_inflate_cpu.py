"""The inflation of vhp_inflate_map / vhp_inflate_maps, without a GPU: csrc/vhp_inflate.hpp -- what vhp_inflate_stack calls for every
word -- run by tests/inflate_driver.cpp.  The half-width tables of every valid footprint are held to the shape's predicate, in the
driver and again here; packed maps inflated word by word are held, pads and tail bits included, to the definition evaluated cell by
cell in the driver and to the numpy packing of inflate_cases.inflate here, on both packed copies, with the border flag off and on.
Sides: inflate_cases.SIDES x SIDES for the footprints of reach up to 3; the five footprints of reach 63 and 64 cost 127 and 129 line
erosions a word, so each of them takes four of the size pairs, chosen so that every side is a width and a height under two of them.
The driver is built plain and under the address and undefined-behaviour sanitizers (a shift by 64, a read outside the packed copies
are theirs to catch), and every case runs through both."""
import functools
import os
import subprocess

import numpy as np
import pytest

import cpu_driver
import inflate_cases as ic
import window_cases as wc

SMALL = tuple(f for f in ic.FOOTPRINTS if ic.reach(*f) <= 3)
LARGE = tuple(f for f in ic.FOOTPRINTS if ic.reach(*f) > 3)


def _large_pairs(i):
    """the size pairs of large footprint i: sides 2i and 2i + 1 of SIDES against sides 2i + 5 and 2i + 6, both ways round"""
    s, n = ic.SIDES, len(ic.SIDES)
    pairs = [(s[(2 * i + j) % n], s[(2 * i + 5 + j) % n]) for j in (0, 1)]
    return pairs + [(b, a) for a, b in pairs]


def footprints_for(nx, ny):
    return SMALL + tuple(f for i, f in enumerate(LARGE) if (nx, ny) in _large_pairs(i))


@pytest.fixture(scope="module", params=["plain", "san"])
def driver(request, tmp_path_factory):
    san = request.param == "san"
    return cpu_driver.build(os.path.join(cpu_driver.HERE, "inflate_driver.cpp"), str(tmp_path_factory.mktemp("inflate")),
                            "inflate_driver_" + request.param, flags=() if san else ("-O2",), sanitized=san)


@functools.lru_cache(maxsize=None)
def _cases(nx, ny):
    """(maps [M, ny, nx], [(shape, p, border)], the words the driver should print) -- computed once, shared by both builds of the driver"""
    stack = np.stack([m for _, m in ic.case_maps(nx, ny, seed=1000 * nx + ny)])
    todo = [(s, p, b) for s, p in footprints_for(nx, ny) for b in (0, 1)]
    want = []
    for s, p, b in todo:
        grown = ic.inflate_stack(stack, s, p, bool(b))
        rows = wc.pack_lines(grown).reshape(len(stack), -1)
        cols = wc.pack_lines(grown.transpose(0, 2, 1)).reshape(len(stack), -1)
        want.append(np.concatenate([rows, cols], axis=1).reshape(-1))
    return stack, todo, np.concatenate(want)


def test_large_footprints_see_every_side():
    assert len(LARGE) == 5 and {ic.reach(*f) for f in LARGE} == {63, 64}
    for axis in (0, 1):
        seen = [pair[axis] for i in range(len(LARGE)) for pair in _large_pairs(i)]
        assert all(seen.count(side) == 2 for side in ic.SIDES), (axis, seen)
    for nx in ic.SIDES:
        for ny in ic.SIDES:
            assert set(SMALL) <= set(footprints_for(nx, ny))


def test_reference_is_the_definition():
    """the numpy inflation on cases small enough to write down"""
    one = np.ones((5, 7), np.uint8)
    one[2, 3] = 0
    assert ic.inflate(one, ic.DISC, 0).tolist() == one.tolist()
    plus = ic.inflate(one, ic.DISC, 1)
    assert sorted(map(tuple, np.argwhere(plus == 0).tolist())) == [(1, 3), (2, 2), (2, 3), (2, 4), (3, 3)]
    assert ic.inflate(one, ic.DIAMOND, 1).tolist() == plus.tolist()
    assert (ic.inflate(one, ic.SQUARE, 1) == 0).sum() == 9 and (ic.inflate(one, ic.DISC, 2) == 0).sum() == 9
    assert (ic.inflate(one, ic.DISC, 4) == 0).sum() == 13 and (ic.inflate(one, ic.DIAMOND, 2) == 0).sum() == 13
    free = np.ones((4, 6), np.uint8)
    assert ic.inflate(free, ic.SQUARE, 1).all()                       # the edge is no wall ...
    ring = ic.inflate(free, ic.SQUARE, 1, border=True)                # ... unless asked for
    assert ring[1:-1, 1:-1].all() and not ring[0].any() and not ring[-1].any() and not ring[:, 0].any() and not ring[:, -1].any()
    assert ic.inflate(np.full((3, 3), 7, np.uint8), ic.DISC, 9).all()   # (any non-zero byte is free)
    assert len(ic.offsets(ic.DISC, 4096)) > len(ic.offsets(ic.DISC, 3969)) and ic.reach(ic.DISC, 4224) == 64


def test_half_width_tables(driver):
    p = subprocess.run([driver, "table"], capture_output=True, check=False)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    lines = p.stdout.decode().splitlines()
    assert len(lines) == 4225 + 65 + 65
    seen = set()
    d = np.arange(0, ic.MAX_INFLATE + 3)
    dx, dy = np.meshgrid(d, d)
    for line in lines:
        shape, p_, reach, *hw = (int(v) for v in line.split())
        seen.add((shape, p_))
        assert len(hw) == reach + 1 and reach <= ic.MAX_INFLATE, line
        table = np.zeros(len(d), np.int64) - 1          # (past the reach: no cell, not even dx = 0)
        table[:reach + 1] = hw
        assert np.array_equal(dx <= table[dy], ic.in_footprint(shape, p_, dx, dy)), (shape, p_)
    assert seen == {(ic.DISC, v) for v in range(4225)} | {(s, v) for s in (ic.SQUARE, ic.DIAMOND) for v in range(65)}


@pytest.mark.parametrize("ny", ic.SIDES)
@pytest.mark.parametrize("nx", ic.SIDES)
def test_inflate_word_equals_numpy(driver, tmp_path, nx, ny):
    stack, todo, want = _cases(nx, ny)
    path = os.path.join(str(tmp_path), "packed_%dx%d.bin" % (nx, ny))
    with open(path, "wb") as f:
        for m in stack:
            f.write(wc.pack_lines(m).astype("<u8").tobytes())
            f.write(wc.pack_lines(m.T).astype("<u8").tobytes())
    p = subprocess.run([driver, "words", path, str(nx), str(ny), str(len(stack))], input="".join("%d %d %d\n" % t for t in todo).encode(),
                       capture_output=True, check=False)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    got = np.frombuffer(p.stdout, "<u8")
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        per_map = ny * ((nx + 63) // 64 + 2) + nx * ((ny + 63) // 64 + 2)
        names = [name for name, _ in ic.case_maps(nx, ny, seed=1000 * nx + ny)]
        at = 0
        for s, p_, b in todo:   # name the first case that differs
            for name in names:
                assert np.array_equal(got[at:at + per_map], want[at:at + per_map]), "map %s of %d x %d, shape %d p %d border %d" % (name, nx, ny, s, p_, b)
                at += per_map


def test_the_check_has_teeth(driver, tmp_path):
    """on this map neighbouring footprints and the border flag all give different words"""
    occ = wc.random_map(65, 64, seed=5, blocked=0.02)
    path = os.path.join(str(tmp_path), "packed.bin")
    with open(path, "wb") as f:
        f.write(wc.pack_lines(occ).astype("<u8").tobytes())
        f.write(wc.pack_lines(occ.T).astype("<u8").tobytes())
    todo = [(ic.DISC, 1, 0), (ic.DISC, 2, 0), (ic.DISC, 2, 1), (ic.DIAMOND, 2, 0)]
    p = subprocess.run([driver, "words", path, "65", "64", "1"], input="".join("%d %d %d\n" % t for t in todo).encode(), capture_output=True, check=False)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    got = np.frombuffer(p.stdout, "<u8").reshape(4, -1)
    assert len({g.tobytes() for g in got}) == 4
