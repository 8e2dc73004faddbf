"""The first round of a pool-sweep launch on the CPU simulator (tests/sim/vhp_pool_sim.cpp compiles the kernel body unchanged), at
the launch shape of a 256-CU device -- 256 workgroups of twelve wavefronts, three contexts each -- and on the batches of
tests/test_gpu_pool_launch_ends.py that need no source outside the map: the first batch on which every context's first unit comes
by workgroup index, the one below it where everything is pulled, and one with fewer units than workgroups."""
import numpy as np
import pytest

import pool_launch_ends_shapes as shapes
import sim_lib
from sim_lib import POOL_POINTS_RANDOM, POOL_RANDOM, POOL_ROUND_ROBIN


@pytest.mark.parametrize("name,static_round", [("96_static_round", 1), ("95_all_pulled", 0), ("9_fewer_units_than_groups", 0)])
def test_pool_sim_first_round_at_the_device_launch_shape(oracle, name, static_round):
    occ, src, _ = shapes.batch(name)
    want = shapes.oracle_fields(oracle, name)
    for policy, seed in ((POOL_ROUND_ROBIN, 1), (POOL_RANDOM | POOL_POINTS_RANDOM, 3)):   # (seeds whose launches keep the static round)
        got, st = sim_lib.pool_sweep(np.array(occ), np.array(src), np.float64, W=12, C=3, G=256, policy=policy, seed=seed)
        assert st["deadlock"] == 0 and st["err"] == 0, st
        assert st["static_round"] == static_round, st
        assert st["pulled"] >= 8 * len(src), st
        for k, (sx, sy) in enumerate(src):
            assert got[k].tobytes() == want[k].tobytes(), "%s policy %d: source %d (%d,%d) differs from the oracle" % (name, policy, k, sx, sy)
