"""The device route's path reconstruction (csrc/vhp_paths.hpp: the parent table and the walk that vhp_paths.hip.h's kernels wrap),
built with the host compiler into tests/paths_driver.cpp and held to vhp_reconstruct_path -- status, point count, every point and the
length's float64 bits -- on planner results of the CPU oracle and on constructed tables that are not planner results.  No GPU.
The driver is built twice: plain, and with the address and undefined-behaviour sanitizers (every buffer there has exactly the size the
header asks for); every case runs through both."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import cpu_driver
import maps

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "visibility-heuristic-path-planner_amd", "csrc")
DRIVER = os.path.join(HERE, "paths_driver.cpp")
SENTINEL = -777
UNL32 = 0xFFFFFFFF
OK, ERR_ARG, ERR_MAX_ITER, ERR_TOO_LARGE = 0, 1, 20, 102


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("paths_driver"))
    return [cpu_driver.build(DRIVER, d, "paths_driver_" + name, flags=("-ffp-contract=off", "-O2"), includes=(CSRC,), sanitized=san)
            for name, san in (("plain", False), ("san", True))]


@pytest.fixture(scope="module")
def vhp():
    import vhp_amd
    vhp_amd.build_library()
    vhp_amd.load_library()
    return vhp_amd


def _labels32(came):
    """the device's labels for the host's: uint32, 0xFFFFFFFF where the reference holds (size_t)1e15"""
    came = np.asarray(came, np.uint64)
    return np.where(came >= np.uint64(UNL32), np.uint64(UNL32), came).astype(np.uint32)


def _host(vhp, came, pivots, end, cap):
    """vhp_reconstruct_path itself: (status, n_path, length bits, the whole path buffer) -- n_path and length start at 0, as the
    driver reports them where the host leaves its outputs alone (VHP_ERR_ARG)."""
    lib = vhp.load_library()
    came = np.ascontiguousarray(came, np.uint64)
    ny, nx = came.shape
    piv = np.ascontiguousarray(pivots, np.int32).reshape(-1, 2)
    path = np.full((max(cap, 0), 2), SENTINEL, np.int32)
    n, d = C.c_uint32(0), C.c_double(0.0)
    rc = lib.vhp_reconstruct_path(came.ctypes.data_as(C.c_void_p), piv.ctypes.data_as(C.c_void_p), len(piv) - 1, nx, ny, int(end[0]), int(end[1]),
                                  path.ctypes.data_as(C.c_void_p) if cap >= 0 else None, max(cap, 0), C.byref(n), C.byref(d))
    return rc, n.value, struct.pack("<d", d.value).hex(), path.reshape(-1).tolist()


def _run(drivers, cases):
    """cases: [(labels uint32 [ny, nx], pivots [n + 1, 2], end, cap)] -> per driver the list of (status, n_path, length bits, buffer)"""
    blob = b""
    for lab, piv, end, cap in cases:
        lab = np.ascontiguousarray(lab, np.uint32)
        piv = np.ascontiguousarray(piv, np.int32).reshape(-1, 2)
        ny, nx = lab.shape
        blob += struct.pack("<6i", nx, ny, len(piv) - 1, int(end[0]), int(end[1]), cap) + lab.tobytes() + piv.tobytes()
    out = []
    for exe in drivers:
        p = subprocess.run([exe], input=blob, capture_output=True, check=False)
        assert p.returncode == 0, (exe, p.returncode, p.stderr.decode()[-2000:])
        rows = []
        for line in p.stdout.decode().splitlines():
            f = line.split()
            rows.append((int(f[0]), int(f[1]), struct.pack("<Q", int(f[2], 16)).hex(), [int(v) for v in f[3:]]))
        assert len(rows) == len(cases)
        out.append(rows)
    assert out[0] == out[1], "the sanitizer build and the plain build disagree"
    return out[0]


def _compare(vhp, drivers, tables):
    """tables: [(came_from uint64 [ny, nx], pivots, end, cap)]: the walk on the device's form of each against vhp_reconstruct_path."""
    got = _run(drivers, [(_labels32(c), p, e, cap) for c, p, e, cap in tables])
    want = [_host(vhp, c, p, e, cap) for c, p, e, cap in tables]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "table %d (end %r, cap %d): walk %r, vhp_reconstruct_path %r" % (k, tables[k][2], tables[k][3], g[:3], w[:3])
    return got


def test_maze6_config4(vhp, oracle, drivers):
    """BASELINE config 4: 64 pivots, the path the reference prints as 1529.55."""
    occ = maps.maze_6()
    ny = occ.shape[0]
    start, end = (345, ny - 1 - 391), (341, ny - 1 - 10)
    r = oracle.solve(occ, start, end, 0.1, 250)
    assert r["status"] == OK and r["n_pivots"] == 64
    cap = r["n_pivots"] + 3
    (st, n, bits, buf), = _compare(vhp, drivers, [(r["came_from"], r["pivots"], end, cap)])
    length = struct.unpack("<d", bytes.fromhex(bits))[0]
    assert st == OK and "%.6g" % length == "1529.55"
    d, path = oracle.reconstruct_path(r["came_from"], r["pivots"], end)
    assert d == length and path.reshape(-1).tolist() == buf[: 2 * n]
    assert buf[:2] == list(start) and buf[2 * n - 2: 2 * n] == list(end) and n >= 3
    assert set(buf[2 * n:]) <= {SENTINEL}


def _free_pairs(occ, n, seed):
    pts = maps.free_sources(occ, 2 * n, seed)
    return [(tuple(int(v) for v in pts[2 * k]), tuple(int(v) for v in pts[2 * k + 1])) for k in range(n)]


def test_oracle_solves_on_random_maps(vhp, oracle, drivers):
    """The C1 rnd_1 mask and 20 seeded random maps, several queries each, thresholds 0.1-0.3, max_iter small enough that some queries end
    in VHP_ERR_MAX_ITER: whatever table a solve leaves, the walk and the host agree, and on a solved query both agree with the oracle."""
    grids = [(maps.c1_rnd1_mask(), 60)]
    for seed in range(20):
        nx, ny = 60 + 7 * (seed % 5), 50 + 11 * (seed % 4)
        grids.append((maps.random_rect_map(nx, ny, 14, 3, 16, 3, 16, 300 + seed), 1 + seed % 3))
    tables, solved, stopped, by_oracle = [], 0, 0, []
    for i, (occ, max_iter) in enumerate(grids):
        occ = np.ascontiguousarray(occ, np.uint8)
        n_q = 3 if occ.size > 40000 else 4
        for k, (start, end) in enumerate(_free_pairs(occ, n_q, 900 + i)):
            thr = (0.1, 0.2, 0.3, 0.15)[k % 4]
            r = oracle.solve(occ, start, end, thr, max_iter)
            if r["status"] not in (OK, ERR_MAX_ITER):
                continue
            tables.append((r["came_from"], r["pivots"], end, r["n_pivots"] + 3))
            solved += r["status"] == OK
            stopped += r["status"] == ERR_MAX_ITER
            by_oracle.append(oracle.reconstruct_path(r["came_from"], r["pivots"], end) if r["status"] == OK else None)
    assert solved >= 30 and stopped >= 5, (solved, stopped)
    got = _compare(vhp, drivers, tables)
    long_paths = 0
    for (st, n, bits, buf), o in zip(got, by_oracle):
        if o is None:
            continue
        assert st == OK and struct.unpack("<d", bytes.fromhex(bits))[0] == o[0] and buf[: 2 * n] == o[1].reshape(-1).tolist()
        long_paths += n >= 3
    assert long_paths >= 15, long_paths
    assert any(g[0] == ERR_ARG for g in got), "no query that ran out of iterations left its end unlabelled"


def _table(nx, ny, pivots, parents, end, end_label):
    """came_from with pivot k's cell labelled parents[k] (None: unlabelled) and `end` labelled end_label"""
    came = np.full((ny, nx), 1000000000000000, np.uint64)
    for (x, y), t in zip(pivots, parents):
        if t is not None and 0 <= x < nx and 0 <= y < ny:
            came[y, x] = t
    if end_label is not None:
        came[end[1], end[0]] = end_label
    return came


def test_constructed_tables(vhp, drivers):
    nx, ny = 23, 17
    chain = [(1, 1), (5, 2), (9, 7), (14, 3), (20, 12)]           # pivot k lit by pivot k - 1, the start labels itself
    par = [0, 0, 1, 2, 3]
    end = (21, 15)
    n = len(chain) - 1
    good = _table(nx, ny, chain, par, end, 4)
    big = 70
    long_piv = [(1 + k % 20, 1 + 2 * (k // 20)) for k in range(big + 1)]
    assert len(set(long_piv)) == big + 1
    cases = {
        "good": (good, chain, end, n + 3),
        "cap exact": (good, chain, end, 6),
        "cap one too small": (good, chain, end, 5),
        "cap zero": (good, chain, end, 0),
        "no path buffer": (good, chain, end, -1),
        "unlabelled end": (_table(nx, ny, chain, par, end, None), chain, end, n + 3),
        "label above n_pivots": (_table(nx, ny, chain, par, end, 5), chain, end, n + 3),
        "label far above": (_table(nx, ny, chain, par, end, 0xFFFFFFFE), chain, end, n + 3),
        "unlabelled pivot": (_table(nx, ny, chain, [0, 0, None, 2, 3], end, 4), chain, end, n + 3),
        "two-cycle": (_table(nx, ny, chain, [0, 2, 1, 2, 3], end, 4), chain, end, n + 3),
        "long cycle": (_table(nx, ny, long_piv, [(k + 1) % (big + 1) for k in range(big + 1)], end, 3), long_piv, end, big + 3),
        "pivot outside the grid": (_table(nx, ny, [(1, 1), (5, 2), (nx, 7), (14, 3), (20, 12)], par, end, 4),
                                   [(1, 1), (5, 2), (nx, 7), (14, 3), (20, 12)], end, n + 3),
        "pivot at negative y": (_table(nx, ny, [(1, 1), (5, -1), (9, 7), (14, 3), (20, 12)], par, end, 4),
                                [(1, 1), (5, -1), (9, 7), (14, 3), (20, 12)], end, n + 3),
        "a pivot that labels itself": (_table(nx, ny, chain, [0, 0, 2, 2, 3], end, 4), chain, end, n + 3),
        "n_pivots = 0": (_table(nx, ny, [(3, 3)], [0], (8, 9), 0), [(3, 3)], (8, 9), 3),
        "start == end": (_table(nx, ny, [(3, 3)], [0], (3, 3), 0), [(3, 3)], (3, 3), 3),
        "longest consistent chain": (_table(nx, ny, long_piv, [max(k - 1, 0) for k in range(big + 1)], end, big), long_piv, end, big + 2),
    }
    names = sorted(cases)
    got = dict(zip(names, _compare(vhp, drivers, [cases[k] for k in names])))
    assert got["good"][:2] == (OK, 6) and got["good"][3] == [1, 1, 5, 2, 9, 7, 14, 3, 20, 12, 21, 15] + [SENTINEL] * 2
    assert got["cap exact"][0] == OK and SENTINEL not in got["cap exact"][3]
    for name in ("cap one too small", "cap zero"):
        st, n_path, bits, buf = got[name]
        assert st == ERR_TOO_LARGE and n_path == 6 and bits == got["good"][2] and set(buf) <= {SENTINEL}, name
    assert got["no path buffer"][:3] == got["good"][:3]
    for name in ("unlabelled end", "label above n_pivots", "label far above", "unlabelled pivot", "two-cycle", "long cycle",
                 "pivot outside the grid", "pivot at negative y"):
        st, n_path, bits, buf = got[name]
        assert st == ERR_ARG and n_path == 0 and set(buf) <= {SENTINEL}, (name, got[name][:3])
    # the walk stops at the first label that repeats: pivot 2 labels itself, the path starts there and not at pivot 0
    assert got["a pivot that labels itself"][:2] == (OK, 4) and got["a pivot that labels itself"][3][:2] == [9, 7]
    assert got["n_pivots = 0"][:2] == (OK, 2) and got["n_pivots = 0"][3] == [3, 3, 8, 9, SENTINEL, SENTINEL]
    assert got["start == end"][:2] == (OK, 2) and got["start == end"][3][:4] == [3, 3, 3, 3]
    assert got["start == end"][2] == struct.pack("<d", 0.0).hex()
    assert got["longest consistent chain"][:2] == (OK, big + 2)


def test_length_is_summed_from_the_start(vhp, drivers):
    """A chain whose segment lengths add up to a different double from the other end (found by search here): only a sum in path order,
    from the start, matches the host."""
    rng = np.random.default_rng(5)
    nx = ny = 200
    found = None
    for _ in range(2000):
        k = int(rng.integers(4, 9))
        pts = [(int(rng.integers(0, nx)), int(rng.integers(0, ny))) for _ in range(k + 1)]
        if len(set(pts)) != len(pts):
            continue
        seg = [float(np.sqrt(np.float64((a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2))) for a, b in zip(pts, pts[1:])]
        fwd = bwd = 0.0
        for s in seg:
            fwd += s
        for s in reversed(seg):
            bwd += s
        if fwd != bwd:
            found = (pts, fwd, bwd)
            break
    assert found, "no chain whose two summation orders differ"
    pts, fwd, bwd = found
    piv, end = pts[:-1], pts[-1]
    n = len(piv) - 1
    came = _table(nx, ny, piv, [max(k - 1, 0) for k in range(n + 1)], end, n)
    (st, n_path, bits, buf), = _compare(vhp, drivers, [(came, piv, end, n + 3)])
    length = struct.unpack("<d", bytes.fromhex(bits))[0]
    assert st == OK and n_path == len(pts) and buf[: 2 * n_path] == [v for p in pts for v in p]
    assert length == fwd and length != bwd
