"""The cut of vhp_set_maps_windows, without a GPU: csrc/vhp_window.hpp -- what vhp_cut_rows_stack and vhp_cut_cols_stack call for every
word -- run by tests/window_driver.cpp over maps packed here in numpy from the layout's definition, and held word for word, pads and
tail bits included, to the numpy packing of the numpy-cut windows.  Every map side in MAP_SIDES x MAP_SIDES, every window size in
WINDOW_SIDES x WINDOW_SIDES and every origin of window_cases.origins in each axis: the windows that start on, before and past a word
boundary, hang over each edge, miss the grid, and sit at the ends of int32.  The driver is built plain and under the address and
undefined-behaviour sanitizers (a shift by 64 at a shift count of 0, a signed overflow at an extreme origin and a read outside the
packed copies are theirs to catch), and every case runs through both."""
import os
import subprocess

import numpy as np
import pytest

import cpu_driver
import window_cases as wc


@pytest.fixture(scope="module", params=["plain", "san"])
def driver(request, tmp_path_factory):
    san = request.param == "san"
    return cpu_driver.build(os.path.join(cpu_driver.HERE, "window_driver.cpp"), str(tmp_path_factory.mktemp("window")),
                            "window_driver_" + request.param, flags=() if san else ("-O2",), sanitized=san)


def _cut_by_driver(exe, occ, windows, tmp_path):
    """the driver's words for the windows (w, h, ox, oy) of occ, as one flat uint64 array"""
    ny, nx = occ.shape
    path = os.path.join(str(tmp_path), "packed_%dx%d.bin" % (nx, ny))
    with open(path, "wb") as f:
        f.write(wc.pack_lines(occ).astype("<u8").tobytes())
        f.write(wc.pack_lines(occ.T).astype("<u8").tobytes())
    p = subprocess.run([exe, path, str(nx), str(ny)], input="".join("%d %d %d %d\n" % t for t in windows).encode(), capture_output=True, check=False)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return np.frombuffer(p.stdout, "<u8")


def test_pack_lines_is_the_layout():
    """the numpy packing against the layout's definition, bit by bit, on a line that ends inside a word and one that fills it"""
    for n in (1, 64, 70):
        bits = wc.random_map(n, 3, seed=n, blocked=0.4)
        words = wc.pack_lines(bits)
        assert words.shape == (3, (n + 63) // 64 + 2) and words.dtype == np.uint64
        for y in range(3):
            assert words[y, 0] == 0 and words[y, -1] == 0
            for c in range(64 * (words.shape[1] - 2)):
                assert (int(words[y, 1 + (c >> 6)]) >> (c & 63)) & 1 == (int(bits[y, c]) if c < n else 0)


@pytest.mark.parametrize("ny", wc.MAP_SIDES)
@pytest.mark.parametrize("nx", wc.MAP_SIDES)
def test_cut_equals_numpy(driver, tmp_path, nx, ny):
    occ = wc.random_map(nx, ny, seed=1000 * nx + ny)
    ox, oy = wc.origins(nx), wc.origins(ny)
    windows, want = [], []
    for h in wc.WINDOW_SIDES:
        for w in wc.WINDOW_SIDES:
            wins = wc.cut(occ, ox, oy, w, h)                                     # [oy, ox, h, w]
            n = len(oy) * len(ox)
            rows = wc.pack_lines(wins).reshape(n, -1)
            cols = wc.pack_lines(wins.transpose(0, 1, 3, 2)).reshape(n, -1)
            want.append(np.concatenate([rows, cols], axis=1).reshape(-1))
            windows += [(w, h, x, y) for y in oy for x in ox]
    want = np.concatenate(want)
    got = _cut_by_driver(driver, occ, windows, tmp_path)
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        # name the first window that differs
        at = 0
        for (w, h, x, y) in windows:
            n = h * ((w + 63) // 64 + 2) + w * ((h + 63) // 64 + 2)
            assert np.array_equal(got[at:at + n], want[at:at + n]), "window %d x %d at (%d, %d) of the %d x %d map" % (w, h, x, y, nx, ny)
            at += n
    assert (want != 0).any()


def test_cut_lets_the_wrong_bits_show(driver, tmp_path):
    """the check has teeth: on these maps the windows one cell to either side differ from the right ones"""
    occ = wc.random_map(130, 65, seed=5)
    a, b = wc.cut(occ, [7], [3], 64, 64), wc.cut(occ, [8], [3], 64, 64)
    assert not np.array_equal(a, b)
    got = _cut_by_driver(driver, occ, [(64, 64, 7, 3), (64, 64, 8, 3)], tmp_path).reshape(2, -1)
    assert not np.array_equal(got[0], got[1])
