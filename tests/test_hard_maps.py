"""The hard maps (tests/hard_maps.py) without a GPU: that the fixtures contain what they are for -- a condition on the inputs,
checked with the oracle alone, so that an edit cannot quietly turn them into easy maps --, and the CPU simulators of the latency and
the pool sweep's own source on them, against the oracle byte for byte.  The gfx950 builds: tests/test_gpu_hard_maps.py."""
import numpy as np
import pytest

import hard_maps
import sim_lib
from sim_lib import POOL_BURSTS, POOL_GREEDY, POOL_POINTS_ALWAYS, POOL_POINTS_RANDOM, POOL_RANDOM, POOL_ROUND_ROBIN
from test_pool_sim import SHAPES as POOL_SHAPES

F32_TINY = float(np.finfo(np.float32).tiny)
F64_TINY = float(np.finfo(np.float64).tiny)


def _fp32_subnormal(f):
    f32 = f.astype(np.float32)
    return int(((f32 > 0) & (f32 < np.float32(F32_TINY))).sum())


def _fp32_flushed(f):
    return int(((f > 0) & (f.astype(np.float32) == 0)).sum())


def _fp64_subnormal(f):
    return int(((f > 0) & (f < F64_TINY)).sum())


# ---- the generators ------------------------------------------------------------------------------------------------------------------

def test_generators_are_what_they_say():
    occ = hard_maps.corridor_star(41, 37, 20, 18, (5,))
    assert occ.dtype == np.uint8 and occ.shape == (37, 41) and occ[18, 20] == 1
    # octant x > y > 0: the corridor i - j = 5 is free, its two walls are blocked from j = 1 on
    for j in range(1, 13):
        assert occ[18 + j, 20 + j + 5] == 1 and occ[18 + j, 20 + j + 4] == 0 and occ[18 + j, 20 + j + 6] == 0
    assert occ[18, 20 + 4] == 1 and occ[18, 20 + 6] == 1   # (j = 0: no wall on the axis)
    # ... and the same in the seven others
    assert np.array_equal(occ[18:, 20:][:19, :21], occ[18::-1, 20:][:19, :21]) and np.array_equal(occ[18:, 20:][:19, :21], occ[18:, 20::-1][:19, :21])
    assert np.array_equal(occ[18:37, 20:39], occ[18:37, 20:39].T)
    # k = 1: the octant's own diagonal is a wall
    occ = hard_maps.corridor_star(30, 30, 10, 10, (1,))
    assert not occ[11:, 11:].diagonal().any() and occ[10, 10] == 1 and occ[12:, 11:].diagonal().all()
    occ = hard_maps.dot_lattice(20, 17, 3, 5)
    assert occ.sum() == 20 * 17 - 7 * 3 and occ[2, 1] == 0 and occ[7, 4] == 0 and occ[2, 2] == 1
    a, b = hard_maps.salt_walled(64, 50, 3, 0.15), hard_maps.salt_walled(64, 50, 3, 0.15)
    assert np.array_equal(a, b) and (a == 0).all(axis=1).any() and (a == 0).all(axis=0).any()


def test_cases_are_named_deterministic_and_free_at_their_sources():
    cases = hard_maps.CASES
    assert [c[0] for c in cases] == list(hard_maps.CASE_NAMES) and len(set(hard_maps.CASE_NAMES)) == len(cases) == 14
    for name, occ, src in cases:
        ny, nx = occ.shape
        assert occ.dtype == np.uint8 and src.dtype == np.int32 and src.shape[1] == 2 and len(src) >= 6
        assert len(set(map(tuple, src.tolist()))) == len(src)
        assert (src[:, 0] >= 0).all() and (src[:, 0] < nx).all() and (src[:, 1] >= 0).all() and (src[:, 1] < ny).all()
        assert occ[src[:, 1], src[:, 0]].all(), name
        assert hard_maps.case(name)[0] is occ   # (cached)
        for corner in ((0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1), (nx // 2, 0)):
            assert corner in set(map(tuple, src.tolist())), (name, corner)
    assert hard_maps.case("star1304")[0].shape == (1203, 1304) and tuple(hard_maps.case("star1304")[1][0]) == (1, 1)
    assert hard_maps.case("dots3x5_333")[0].shape == (301, 333)


# ---- the fixtures do what they are for -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", hard_maps.CASE_NAMES)
def test_fields_hold_what_the_case_is_for(oracle, name):
    occ, src = hard_maps.case(name)
    f = hard_maps.fields(oracle, name)
    assert f.shape == (len(src),) + occ.shape
    # every case, every source: a visibility, and no -0.0 (the kernels test bit patterns for +0.0)
    assert not np.isnan(f).any() and not (f < 0).any() and not np.signbit(f).any() and not (f > 1).any()
    first = f[0]
    positive = first[first > 0]
    print("%s: fp32-subnormal %d, > 0 in fp64 and 0 in fp32 %d, fp64-subnormal %d, smallest positive %r, in (0, 0.001] %d, in (0.001, 0.999) %d" % (
        name, _fp32_subnormal(first), _fp32_flushed(first), _fp64_subnormal(first), float(positive.min()),
        int(((first > 0) & (first <= 0.001)).sum()), int(((first > 0.001) & (first < 0.999)).sum())))
    if name in ("star401", "star400x363"):
        assert _fp32_subnormal(first) >= 500
    if name in ("star328_lo", "star328_hi"):
        assert _fp32_subnormal(first) >= 1500
        assert _fp32_flushed(first) >= 3500
    if name in ("star1304", "star1200"):
        assert _fp64_subnormal(first) >= 1500
        assert float(positive.min()) == 5e-324
    if name == "dots3x5":
        assert int(((first > 0) & (first <= 0.001)).sum()) >= 25000
        assert int(((first > 0.001) & (first < 0.999)).sum()) >= 12000


# ---- the simulators of the kernels' own source ---------------------------------------------------------------------------------------

SIM_CASES = ("star401", "star328_lo", "star_q1", "dots3x5")


def _assert_fields(got, want, src, what):
    for k, (sx, sy) in enumerate(src):
        if got[k].tobytes() != want[k].tobytes():
            bad = np.argwhere(~((got[k] == want[k]) | (np.isnan(got[k]) & np.isnan(want[k]))))
            y, x = bad[0]
            raise AssertionError("%s, source (%d,%d): %d cells differ, first at (x=%d,y=%d): got %r want %r" % (
                what, sx, sy, len(bad), x, y, got[k][y, x], want[k][y, x]))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", SIM_CASES)
def test_lat_sim_on_hard_maps(oracle, name, dtype):
    """csrc/vhp_band.hpp as the library launches it: two workgroup sizes (12: every band a wavefront of its own where they suffice; 3:
    rounds, a wavefront sweeps band after band, and dead bands are skipped), and an octant's bands dealt to two workgroups (death by
    decay passed on through the global record)."""
    occ, src = hard_maps.case(name)
    want = hard_maps.fields(oracle, name).astype(dtype)
    died = 0
    for W, policy, halves in [(12, POOL_ROUND_ROBIN | POOL_POINTS_ALWAYS, 1), (3, POOL_BURSTS | POOL_POINTS_RANDOM, 1),
                              (12, POOL_RANDOM | POOL_POINTS_RANDOM, 2), (3, POOL_GREEDY | POOL_POINTS_ALWAYS, 2)]:
        what = "%s %s W=%d policy=%d, %d workgroups per unit" % (name, np.dtype(dtype).name, W, policy, halves)
        got, st = sim_lib.lat_sweep(occ, src, dtype, W=W, policy=policy, seed=W + halves, halves=halves)
        assert st["deadlock"] == 0, "%s: every wavefront waiting %r" % (what, st)
        assert st["err"] == 0
        _assert_fields(got, want, src, what)
        died += st["died"]
    if name.startswith("star"):
        assert died > 0, "no band of %s died" % name


def test_lat_sim_star1304_two_workgroups_per_unit(oracle):
    """Sides above 1024, where the library deals an octant's bands to two workgroups by itself: the centre source and a far corner."""
    occ, src = hard_maps.case("star1304")
    pick = [0, 4]
    want = hard_maps.fields(oracle, "star1304")[pick]
    got, st = sim_lib.lat_sweep(occ, src[pick], np.float64, W=12, policy=POOL_ROUND_ROBIN, seed=1, halves=2)
    assert st["deadlock"] == 0 and st["err"] == 0 and st["died"] > 0, st
    _assert_fields(got, want, src[pick], "star1304, 2 workgroups per unit")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", SIM_CASES)
def test_pool_sim_on_hard_maps(oracle, name, dtype):
    """csrc/vhp_pool.hpp in the pool shapes of tests/test_pool_sim.py (its dtype column replaced by this test's)"""
    occ, src = hard_maps.case(name)
    want = hard_maps.fields(oracle, name).astype(dtype)
    for W, C, G, policy, _ in POOL_SHAPES:
        what = "%s %s W=%d C=%d G=%d policy=%d" % (name, np.dtype(dtype).name, W, C, G, policy)
        got, st = sim_lib.pool_sweep(occ, src, dtype, W=W, C=C, G=G, policy=policy, seed=W + C)
        assert st["deadlock"] == 0, "%s: every wavefront waiting %r" % (what, st)
        assert st["err"] == 0
        assert st["pulled"] >= 8 * len(src), "%s: %d units pulled of %d" % (what, st["pulled"], 8 * len(src))
        _assert_fields(got, want, src, what)
