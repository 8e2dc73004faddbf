"""Obstacles grown by a footprint in numpy, for the tests of vhp_inflate_map / vhp_inflate_maps (test_inflate_cpu.py,
test_gpu_inflate.py): the inflation written out from its definition in include/vhp.h -- enumerate the footprint's offsets by the
shape's predicate, pad the map by the reach with the border's value, OR the shifted blocked masks -- and the sizes, footprints and
maps both tests cover.  Nothing here knows of half-widths, packed words or erosions: it is a statement of its own."""
import numpy as np

DISC, SQUARE, DIAMOND = 0, 1, 2
MAX_INFLATE = 64

# the word edges, the last data word's mask, lines of one word
SIDES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 130)
# (shape, p): the identity, the first discs, discs that differ from the squares around them, reach 63 and 64; squares and diamonds to 64
FOOTPRINTS = ((DISC, 0), (DISC, 1), (DISC, 2), (DISC, 4), (DISC, 5), (DISC, 8), (DISC, 9), (DISC, 3969), (DISC, 4096),
              (SQUARE, 1), (SQUARE, 2), (SQUARE, 63), (SQUARE, 64), (DIAMOND, 1), (DIAMOND, 3), (DIAMOND, 64))
GPU_SIDES = ((1, 63, 64, 65, 130), (1, 64, 129))   # nx of, ny of
GPU_FOOTPRINTS = ((DISC, 0), (DISC, 1), (DISC, 2), (DISC, 8), (DISC, 4096), (SQUARE, 3), (DIAMOND, 2))


def in_footprint(shape, p, dx, dy):
    """the predicate of include/vhp.h, on integers or integer arrays"""
    if shape == DISC:
        return dx * dx + dy * dy <= p
    if shape == SQUARE:
        return np.maximum(np.abs(dx), np.abs(dy)) <= p
    if shape == DIAMOND:
        return np.abs(dx) + np.abs(dy) <= p
    raise ValueError(shape)


def offsets(shape, p):
    """every (dx, dy) of the footprint, found by trying all of a box that holds any footprint of a valid p and one cell more"""
    bound = MAX_INFLATE + 2
    d = np.arange(-bound, bound + 1)
    dx, dy = np.meshgrid(d, d)
    inside = in_footprint(shape, p, dx, dy)
    assert not inside[0].any() and not inside[-1].any() and not inside[:, 0].any() and not inside[:, -1].any(), "footprint larger than the box"
    return [(int(x), int(y)) for x, y in zip(dx[inside], dy[inside])]


def reach(shape, p):
    return max(abs(x) for x, _ in offsets(shape, p))


def inflate(occ, shape, p, border=False):
    """uint8 [ny, nx] (any values, != 0 is free; leading axes are so many maps) -> uint8 0 / 1: cell (x, y) is blocked exactly when
    some (x + dx, y + dy) of the footprint is blocked, cells outside the grid being free, or blocked with `border`."""
    occ = np.asarray(occ)
    ny, nx = occ.shape[-2:]
    offs = offsets(shape, p)
    r = max(max(abs(x), abs(y)) for x, y in offs)
    blocked = np.full(occ.shape[:-2] + (ny + 2 * r, nx + 2 * r), bool(border))
    blocked[..., r:r + ny, r:r + nx] = occ == 0
    out = np.zeros(occ.shape, bool)
    for dx, dy in offs:
        out |= blocked[..., r + dy:r + dy + ny, r + dx:r + dx + nx]
    return (~out).astype(np.uint8)


def inflate_stack(stack, shape, p, border=False):
    """the same for uint8 [n, ny, nx], every map by itself"""
    return inflate(stack, shape, p, border)


def special_cells(n):
    """the coordinates along an axis of n cells where a single blocked cell goes: both ends and around the first word's edge"""
    return sorted({c for c in (0, 62, 63, 64, 65, n - 1) if 0 <= c < n})


def case_maps(nx, ny, seed):
    """[(name, uint8 [ny, nx])]: one blocked cell at each corner and at each pair of special coordinates on the diagonal of the list,
    all free, all blocked, random at 2 % and 40 % blocked"""
    out = []
    for name, (x, y) in (("corner00", (0, 0)), ("corner10", (nx - 1, 0)), ("corner01", (0, ny - 1)), ("corner11", (nx - 1, ny - 1))):
        m = np.ones((ny, nx), np.uint8)
        m[y, x] = 0
        out.append((name, m))
    xs, ys = special_cells(nx), special_cells(ny)
    for i in range(max(len(xs), len(ys))):
        x, y = xs[i % len(xs)], ys[(i * 7 + 1) % len(ys)]   # (7 is coprime to every length here: each x and each y is taken)
        m = np.ones((ny, nx), np.uint8)
        m[y, x] = 0
        out.append(("cell_%d_%d" % (x, y), m))
    out.append(("free", np.ones((ny, nx), np.uint8)))
    out.append(("blocked", np.zeros((ny, nx), np.uint8)))
    rng = np.random.default_rng(seed)
    for share in (0.02, 0.4):
        out.append(("random_%g" % share, (rng.random((ny, nx)) >= share).astype(np.uint8)))
    return out
