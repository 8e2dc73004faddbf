"""Windows of a map in numpy, for the tests of vhp_set_maps_windows (test_window_cut_cpu.py, test_gpu_windows.py): the cut, the packed
layout written out from its definition, and the grid of sizes and origins both tests cover."""
import numpy as np

MAP_SIDES = (1, 63, 64, 65, 130)
WINDOW_SIDES = (1, 63, 64, 65, 128, 129)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def origins(n):
    """the origins along an axis of n cells: around both edges, a word and two words before the grid, past it, and the ends of int32"""
    return (-129, -64, -63, -1, 0, 1, 63, 64, n - 1, n, n + 70, INT32_MIN, INT32_MAX)


def random_map(nx, ny, seed, blocked=0.05):
    """uint8 [ny, nx], 1 = free; about 5 % blocked, so that a bit shifted in from the wrong place is most likely a 1 where a 0 belongs"""
    rng = np.random.default_rng(seed)
    return (rng.random((ny, nx)) >= blocked).astype(np.uint8)


def cut(occ, ox, oy, w, h):
    """windows of w x h of occ (any values, != 0 is free) at every (oy[a], ox[b]): uint8 [len(oy), len(ox), h, w], blocked outside the grid"""
    ny, nx = occ.shape
    xs = np.asarray(ox, np.int64).reshape(-1, 1) + np.arange(w, dtype=np.int64)     # [B, w]
    ys = np.asarray(oy, np.int64).reshape(-1, 1) + np.arange(h, dtype=np.int64)     # [A, h]
    x_in, y_in = (xs >= 0) & (xs < nx), (ys >= 0) & (ys < ny)
    free = occ != 0
    got = free[np.where(y_in, ys, 0)[:, None, :, None], np.where(x_in, xs, 0)[None, :, None, :]]
    return (got & y_in[:, None, :, None] & x_in[None, :, None, :]).astype(np.uint8)


def cut_list(occ, origin_xy, w, h):
    """window k at origin_xy[k] = (ox, oy): uint8 [n, h, w]"""
    o = np.asarray(origin_xy, np.int64).reshape(-1, 2)
    return np.stack([cut(occ, [x], [y], w, h)[0, 0] for x, y in o]) if len(o) else np.zeros((0, h, w), np.uint8)


def pack_lines(bits):
    """[..., lines, n] of 0 / 1 -> uint64 [..., lines, (n + 63) // 64 + 2]: bit c & 63 of word 1 + (c >> 6) is cell c, word 0 and the
    last word are zero pads, the bits past n are 0 (the layout of DevMap::rows; the column-packed copy is pack_lines of the transpose)"""
    bits = np.asarray(bits, np.uint8)
    n = bits.shape[-1]
    words = (n + 63) // 64
    padded = np.zeros(bits.shape[:-1] + ((words + 2) * 64,), np.uint8)
    padded[..., 64:64 + n] = bits != 0
    return np.packbits(padded, axis=-1, bitorder="little").view("<u8").astype(np.uint64)
