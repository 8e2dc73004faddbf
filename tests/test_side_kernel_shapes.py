"""Without a GPU: the inputs of tests/test_gpu_side_kernels.py (side_kernel_shapes.py) are past the sizes they are meant to pass, the
sources that cross a slice differ from their counterparts in the first slice, and the oracle answers the planner cases with the
statuses the GPU tests are there to reach.  The library's constants are restated in side_kernel_shapes.py with their source lines."""
import numpy as np
import pytest

import side_kernel_shapes as shapes


def test_staging_batches_cross_a_slice_with_other_sources():
    occ, src = shapes.stage_batch()
    n, cut = len(src), shapes.STAGE_SLICE
    assert occ.shape == (1024, 1024) and (cut, n) == (128, 131)
    assert n * shapes.STAGE_FIELD_BYTES > 2**30 >= cut * shapes.STAGE_FIELD_BYTES
    distinct = {(int(x), int(y)) for x, y in src}
    assert len(distinct) == 5 and cut % 5 != 0
    assert {(0, 0), (1023, 1023)} <= distinct and sum(1 for x, y in distinct if not occ[y, x]) == 1
    a, b = shapes.STAGE_REPEAT
    assert abs(a - b) == 1 and src[a].tolist() == src[b].tolist()
    for k in range(cut, n):   # every source of the second slice differs from the one a dropped `+ 2 * s0` would sweep
        assert src[k].tolist() != src[k - cut].tolist()

    occ2, src2, idx = shapes.stage_maps_batch()
    assert occ2.shape == (2, 1024, 1024) and len(src2) == len(idx) == n
    assert (occ2[0] != occ2[1]).any()
    assert idx.tolist() == [(i // 3) % 2 for i in range(n)]
    assert (idx[cut:] != idx[: n - cut]).any()
    for k in range(cut, n):
        assert src2[k].tolist() != src2[k - cut].tolist()


def test_staging_fields_tell_a_wrong_source_or_map_apart(oracle):
    """What a dropped offset would write is another field: the oracle's fields of the sources and maps either side of the slice differ."""
    occ, src = shapes.stage_batch()
    want = shapes.stage_oracle_fields(oracle)
    assert len(want) == 5
    cut = shapes.STAGE_SLICE
    for k in range(cut, len(src)):
        assert want[tuple(src[k].tolist())].tobytes() != want[tuple(src[k - cut].tolist())].tobytes()
    occ2, src2, idx = shapes.stage_maps_batch()
    want2 = shapes.stage_maps_oracle_fields(oracle)
    assert len(want2) <= 10
    crossed = [k for k in range(cut, len(src2)) if idx[k] != idx[k - cut]]
    assert crossed
    for k in crossed:   # the source of the second slice on the map a dropped `map_idx + s0` would give it
        x, y = src2[k].tolist()
        assert want2[(int(idx[k]), x, y)].tobytes() != oracle.sweep_full(np.array(occ2[idx[k - cut]]), x, y).tobytes()


def test_queue_batch_crosses_a_slice_with_other_sources(oracle):
    occ, src = shapes.queue_batch()
    cut = shapes.QUEUE_SLICE
    assert occ.shape == (300, 400) and cut == 271 and len(src) == 274
    assert cut == 2**30 // (33 * occ.size + 64) and len(src) > cut
    assert len(src) * occ.size * 8 < 2**30   # (one slice of the host staging: the queue's own loop is what repeats)
    distinct = {(int(x), int(y)) for x, y in src}
    assert len(distinct) == 12 and cut % 12 != 0
    assert {(0, 0), (399, 0), (0, 299), (399, 299)} <= distinct and sum(1 for x, y in distinct if not occ[y, x]) == 1
    want = shapes.queue_oracle_fields(oracle)
    for k in range(cut, len(src)):
        assert want[tuple(src[k].tolist())].tobytes() != want[tuple(src[k - cut].tolist())].tobytes()
    # floods that stay short: one lane walks each of them
    assert max(int((f > 0).sum()) for f in want.values()) < occ.size // 8

    small, small_src = shapes.queue_small()
    assert small.shape == (97, 120) and len(small_src) > 4


def test_union_grids_and_strides():
    # 256 CUs (MI355X): the GPU test asserts the same with the device's own count
    for nx, ny in shapes.UNION_GRIDS.values():
        assert nx * ny > 2 * shapes.UNION_CELLS_PER_CU_AND_PASS * 256
    assert shapes.UNION_CELLS_PER_CU_AND_PASS * 256 == 2097152
    nx, ny = shapes.UNION_GRIDS["odd"]
    assert nx * ny == 5257525 and nx * ny % 2 == 1
    nx, ny = shapes.UNION_GRIDS["even"]
    assert nx * ny % 2 == 0
    assert shapes.UNION_FIELDS // 4 == 1 and shapes.UNION_FIELDS % 4 == 2
    cuts = shapes.UNION_CUTS
    assert cuts[0][0] == 0 and cuts[-1][1] == shapes.UNION_FIELDS and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
    assert sorted(shapes.UNION_SLOTS) == [0, 1, 2] and list(shapes.UNION_SLOTS) != [0, 1, 2]
    cells = shapes.STRIDE_GRID[0] * shapes.STRIDE_GRID[1]
    assert (cells + shapes.STRIDE_PADS["pairs"]) % 2 == 0 and (cells + shapes.STRIDE_PADS["cells"]) % 2 == 1
    f = shapes.stride_fields(np.float32)
    flat = shapes.padded(f, 5)
    assert flat.size == len(f) * (cells + 5) and np.isinf(flat).sum() == len(f) * 5
    assert flat[cells + 5: 2 * cells + 5].tobytes() == f[1].tobytes()
    # ties in the inputs: the arg of a tied cell is the lowest index, and a pad read as a cell would win it
    wb, wa = shapes._numpy_union(f, 0)
    assert (f[3] == f[1]).all() and not (wa == 3).any() and (wb <= 1.1).all()


def test_variant_grids_reach_what_they_are_for():
    lds = shapes.variant_lds_bytes
    assert lds(2729, 1030) == 65520 <= shapes.LDS_DEFAULT_LIMIT < lds(2730, 1030) == 65544
    assert lds(4096, 1100) == lds(1100, 4096) == 98328
    assert shapes.VARIANT_GRIDS == [(1500, 1100), (2729, 1030), (2730, 1030), (4096, 1100), (1100, 4096)]
    for nx, ny in shapes.VARIANT_GRIDS:
        assert shapes.VARIANT_THREADS < min(nx, ny) and max(nx, ny) <= shapes.VARIANT_MAX_SIDE
        occ, src = shapes.variant_case(nx, ny)
        assert occ.shape == (ny, nx) and 0.3 < occ.mean() < 1.0
        assert src.tolist()[:3] == [[0, 0], [nx - 1, ny - 1], [nx - 1, 0]] and all(occ[y, x] for x, y in src)
        x, y = src[3]
        assert 0 < x < nx - 1 and 0 < y < ny - 1
    for occ in shapes.too_large_maps():
        assert max(occ.shape) == shapes.VARIANT_MAX_SIDE + 1 and min(occ.shape) == 8


@pytest.mark.parametrize("name", shapes.PLANNER_NAMES)
def test_planner_cases_reach_their_status(oracle, name):
    occ, start, end, thr, alpha, max_iter = shapes.planner_cases()[name]
    want = shapes.planner_want(oracle, name)
    if name in shapes.PLANNER_EXPECT:
        status, n_way = shapes.PLANNER_EXPECT[name]
        assert (want["status"], len(want["waypoints"])) == (status, n_way)
    if want["status"] == 20:
        assert len(want["waypoints"]) == max_iter + 2
    if name == "start walled in":
        x, y = start
        assert occ[y, x] == 1 and occ[y - 1:y + 2, x - 1:x + 2].sum() == 1
    if name == "blocked start":
        assert occ[start[1], start[0]] == 0
    if name == "start is end":
        assert start == end and occ[start[1], start[0]] == 1
    if name.startswith("203x150"):
        assert occ.shape == (150, 203) and want["status"] == 0 and len(want["waypoints"]) >= 3
    if name.startswith("1100x1040"):
        assert occ.shape == (1040, 1100) and max_iter == 12 and len(want["waypoints"]) >= 3


@pytest.mark.parametrize("name", list(shapes.PLANNER_TIES))
def test_planner_ties_lie_where_the_pick_has_to_break_them(oracle, name):
    same_wave, same_lane = shapes.PLANNER_TIES[name]
    occ = shapes.planner_cases()[name][0]
    nx = occ.shape[1]
    tied = shapes.first_pick_minima(oracle, name)
    assert len(tied) == 2, tied
    thread = [int(k) % shapes.PICK_THREADS for k in tied]
    assert thread[0] != thread[1]
    assert (thread[0] // 64 == thread[1] // 64) == same_wave and (thread[0] % 64 == thread[1] % 64) == same_lane
    # the oracle takes the lowest linear index, and the other one is a different waypoint
    want = shapes.planner_want(oracle, name)
    assert want["waypoints"][1].tolist() == [int(tied[0]) % nx, int(tied[0]) // nx]
