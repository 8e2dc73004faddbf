"""ctypes binding of tests/sim/libvhp_lat_maps_sim.so -- TEST INFRASTRUCTURE ONLY.

The latency sweep on a stack of maps (csrc/vhp_band.hpp BandWorker, STACK build) on the CPU simulator of tests/sim: the library is
compiled here from tests/sim/vhp_lat_maps_sim.cpp, with the flags of tests/sim/Makefile.  Nothing in the product imports this.
"""
import ctypes as C
import os
import subprocess

import numpy as np

import sim_lib

SRC = os.path.join(sim_lib.SIM_DIR, "vhp_lat_maps_sim.cpp")
LIB = os.path.join(sim_lib.SIM_DIR, "libvhp_lat_maps_sim.so")
_lib = None


def _stale():
    if not os.path.exists(LIB):
        return True
    csrc = os.path.join(sim_lib.ROOT, "visibility-heuristic-path-planner_amd", "csrc")
    deps = [SRC, os.path.join(sim_lib.SIM_DIR, "vhp_pool_sim.cpp")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hpp", ".h"))]
    return max(os.path.getmtime(p) for p in deps) > os.path.getmtime(LIB)


def load():
    global _lib
    if _lib is None:
        if _stale():
            tmp = LIB + ".%d.tmp" % os.getpid()
            subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall",
                                   "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", tmp, SRC])
            os.replace(tmp, LIB)
        lib = C.CDLL(LIB)
        vp, i32 = C.c_void_p, C.c_int
        lib.vhp_sim_lat_maps_sweep.argtypes = [vp, i32, i32, i32, vp, vp, i32, vp, i32, i32, C.c_uint, vp]
        lib.vhp_sim_stack_diag_words.argtypes = [vp, i32, i32, i32, vp, vp]
        lib.vhp_sim_diag_words.argtypes = [i32, i32]
        lib.vhp_sim_diag_words.restype = C.c_ulonglong
        lib.vhp_sim_set_lat_halves.argtypes = [i32]
        _lib = lib
    return _lib


def lat_maps_sweep(stack, sources, map_index, W=12, policy=0, seed=1, halves=1):
    """Fields [n, ny, nx] float64 (pre-filled with NaN) of source k swept on map map_index[k] of stack [M, ny, nx], and the stats dict
    of sim_lib.lat_sweep.  halves: workgroups per unit (1: the one-workgroup build; 2: the build whose bands read across workgroups)."""
    lib = load()
    stack = np.ascontiguousarray(stack, np.uint8)
    m, ny, nx = stack.shape
    src = np.ascontiguousarray(sources, np.int32).reshape(-1, 2)
    idx = np.ascontiguousarray(map_index, np.int32).reshape(-1)
    assert len(idx) == len(src)
    out = np.full((len(src), ny, nx), np.nan, np.float64)
    stats = np.zeros(11, np.int64)
    lib.vhp_sim_set_lat_halves(int(halves))
    try:
        rc = lib.vhp_sim_lat_maps_sweep(stack.ctypes.data, m, nx, ny, src.ctypes.data, idx.ctypes.data, len(src), out.ctypes.data, W, policy, seed,
                                        stats.ctypes.data)
    finally:
        lib.vhp_sim_set_lat_halves(1)
    assert rc == 0, rc
    return out, dict(switches=int(stats[0]), progress=int(stats[1]), deadlock=int(stats[2]), err=int(stats[5]))


def stack_diag_words(stack):
    """The stack's diagonal maps [M, words]: (built from the row-packed words, built from each map's bytes)."""
    lib = load()
    stack = np.ascontiguousarray(stack, np.uint8)
    m, ny, nx = stack.shape
    words = int(lib.vhp_sim_diag_words(nx, ny))
    a = np.zeros((m, words), np.uint64)
    b = np.zeros((m, words), np.uint64)
    assert lib.vhp_sim_stack_diag_words(stack.ctypes.data, m, nx, ny, a.ctypes.data, b.ctypes.data) == 0
    return a, b
