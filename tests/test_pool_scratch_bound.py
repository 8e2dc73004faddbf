"""The pool sweep's scratch sizes (csrc/vhp_pool_scratch.hpp) hold what the sweep asks of them.  CPU only.

The launcher sizes the boundary-line scratch by line_blocks_per_source(nx, ny) blocks per source; the order pre-kernel lays the units'
lines out by the sum of UnitGeo::line_blocks().  Were a source ever to need more than the bound, the pre-kernel would set error bit 4
and the launch would sweep nothing.  tests/pool_scratch_driver.cpp sums line_blocks() over the 8 units of every source it is given:

  * every source of every grid of EXHAUSTIVE (sides up to 1025);
  * on the grids of SAMPLED, every 7th cell in row-major order and every cell with a coordinate in {0, 1, 15, 16, 63, 64, n/2, n-2,
    n-1}.  The last of them is VHP_MAX_SIDE squared: pool_supported() turns away any side above it, so it accepts nothing larger.

The need never exceeds the bound, the worst ratio is the one DESIGN.md quotes, head_bytes() holds the records, order and line bases that
launch_pool_t carves from it, and the driver gives the same answers under the address and undefined-behaviour sanitizers."""
import os
import re

import pytest

import pool_scratch_lib as lib

EXHAUSTIVE = [(1, 1), (2, 2), (64, 64), (65, 65), (129, 129), (130, 130), (130, 136), (136, 136), (257, 255), (255, 257), (1, 1025), (1025, 1),
              (1000, 1000), (1024, 1024), (1025, 1025)]
SAMPLED = [(2048, 1500), (3000, 2504), (4096, 4096), (8192, 130), (130, 8192), (513, 8192), (8192, 8192)]
REQUESTS = ["lines %d %d all" % g for g in EXHAUSTIVE] + ["lines %d %d sampled" % g for g in SAMPLED]
HEAD_SOURCES = [1, 1024, 1025, 4096]
SIZES = ["sizes %d 136 136" % n for n in HEAD_SOURCES]


@pytest.fixture(scope="module")
def answers():
    return lib.run(REQUESTS + SIZES)


def _lines(answers):
    return list(zip(EXHAUSTIVE + SAMPLED, answers[:len(REQUESTS)]))


def test_the_sampled_grids_reach_the_largest_side_the_library_takes():
    with open(os.path.join(lib.ROOT, "include", "vhp.h")) as f:
        max_side = int(re.search(r"#define VHP_MAX_SIDE (\d+)", f.read()).group(1))
    assert SAMPLED[-1] == (max_side, max_side)


def test_need_never_exceeds_the_bound(answers):
    for (nx, ny), (bound, need, sx, sy, units, sources) in _lines(answers):
        print("%dx%d: bound %d, need %d at (%d,%d), ratio %.4f, %d units with a line over %d sources" % (
            nx, ny, bound, need, sx, sy, need / bound, units, sources))
        assert sources >= (nx * ny if (nx, ny) in EXHAUSTIVE else nx * ny // 7)
        assert 0 <= need <= bound, "%dx%d: source (%d,%d) needs %d blocks of boundary lines, the scratch has %d" % (nx, ny, sx, sy, need, bound)
    # (not vacuous: a grid of more than 64 a side has units of two strips and more, one of at most 64 has none)
    by_grid = {g: a for g, a in _lines(answers)}
    assert by_grid[(64, 64)][1] == 0 and by_grid[(64, 64)][4] == 0
    assert by_grid[(65, 65)][1] > 0 and by_grid[(8192, 8192)][1] > 20000


def test_worst_ratio_is_the_one_in_the_design_notes(answers):
    ratio, (nx, ny) = max((need / bound, g) for g, (bound, need, *_) in _lines(answers))
    print("worst need / bound: %.3f at %dx%d" % (ratio, nx, ny))
    with open(os.path.join(lib.ROOT, "DESIGN.md")) as f:
        m = re.search(r"worst need / bound ratio[^0-9]*([0-9.]+[0-9]) at (\d+)x(\d+)", f.read())
    assert m, "DESIGN.md does not quote the worst need / bound ratio"
    assert (m.group(1), int(m.group(2)), int(m.group(3))) == ("%.3f" % ratio, nx, ny)


def test_head_holds_the_records_the_order_and_the_line_bases(answers):
    for n, (head, layout, diag, diag_stride) in zip(HEAD_SOURCES, answers[len(REQUESTS):]):
        # the pull counter's 16 ints, then 4 ints of record, one of order and one of line base for each of the 8 n units
        assert layout == 4 * (16 + 6 * 8 * n)
        assert head >= layout and head % 256 == 0, (n, head, layout)
        # (the diagonal scratch: 4 y-major units per source, a line of diag_stride doubles each; the boundary lines behind it stay aligned)
        assert diag >= n * 4 * diag_stride * 8 and diag % 256 == 0 and diag_stride >= 136 + 64


def test_the_large_gpu_batches_have_more_than_1024_units_with_a_line():
    """tests/test_gpu_large_batches.py would not see a wrong line base otherwise (large_batch_shapes.batch asserts it)"""
    import large_batch_shapes as shapes
    for grid, (nx, ny) in shapes.GRIDS.items():
        for name, (n, with_outside) in shapes.POOL.items():
            occ, src, outside = shapes.batch(grid, n, with_outside)
            assert occ.shape == (ny, nx) and src.shape == (n, 2) and len(outside) == (3 if with_outside else 0)
            inside = [k for k in range(n) if 0 <= src[k][0] < nx and 0 <= src[k][1] < ny]
            assert sorted(set(range(n)) - set(inside)) == sorted(outside)
            assert (shapes.ORDER_BODY[name] == "order_units_lds") == (n * 8 <= 8192)
            for corner in ((0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1)):
                assert corner in {tuple(int(v) for v in xy) for xy in src}
            assert len({tuple(int(v) for v in xy) for xy in src}) < n   # some positions twice


def test_driver_under_the_sanitizers_agrees(answers):
    assert lib.run(REQUESTS + SIZES, sanitized=True) == answers
