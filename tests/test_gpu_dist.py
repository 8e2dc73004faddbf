"""The multi-GPU source sharding with the HIP sweep as the per-rank compute, under torch.distributed's RCCL backend
("nccl") with a single rank: every code path of dist.py that the 8-GPU bench uses (map broadcast, block partition,
all-gather of fields, max-union + arg-source, chunked all-gather overlapped with the next chunk's sweeps) runs on one
MI355X, on device tensors, against the oracle.  World sizes 2 and 3 run on CPU with gloo (tests/test_dist_gloo.py)."""
import os
import socket

import numpy as np
import pytest

import maps

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_sharded_hip_sweep_under_rccl_single_rank(oracle):
    import torch
    import torch.distributed as dist
    import vhp_amd
    from importlib import import_module
    vd = import_module("visibility-heuristic-path-planner_amd.dist")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(_free_port())
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        occ = maps.random_rect_map(328, 300, 30, 3, 40, 3, 40, 5)
        n = 16
        src = maps.free_sources(occ, n, 8)
        full = np.stack([oracle.sweep_full(occ, int(x), int(y)) for x, y in src])
        # the map is broadcast as a device tensor and handed to the library without a host round trip
        d_occ = vd.broadcast_map(torch.from_numpy(occ).cuda(), 0)
        ctx = vhp_amd.Context(0)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.set_map_device(d_occ.data_ptr(), occ.shape[1], occ.shape[0])

        def compute(shard):
            d_src = torch.from_numpy(np.ascontiguousarray(shard, np.int32)).cuda()
            out = torch.empty((len(shard),) + occ.shape, dtype=torch.float64, device="cuda")
            if len(shard):
                ctx.sweep_batch_device(d_src.data_ptr(), len(shard), out.data_ptr())
            ctx.sync()
            return out

        local, lo = vd.sweep_sharded(compute, src, "none")
        assert lo == 0 and np.array_equal(local.cpu().numpy(), full)
        allf = vd.sweep_sharded(compute, src, "gather")
        assert np.array_equal(allf.cpu().numpy(), full)
        best, arg = vd.sweep_sharded(compute, src, "union")
        assert np.array_equal(best.cpu().numpy(), full.max(0))
        assert np.array_equal(arg.cpu().numpy(), (full == full.max(0)[None]).argmax(0))
        # chunked all-gather overlapped with the sweeps of the next chunk, on two streams
        d_src = torch.from_numpy(np.ascontiguousarray(src, np.int32)).cuda()
        out = torch.full((n,) + occ.shape, -1.0, dtype=torch.float64, device="cuda")

        def launch(a, b, dst):
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            ctx.sweep_batch_device(d_src[a:b].data_ptr(), b - a, dst.data_ptr())

        vd.sweep_gather_overlapped(launch, src, out, chunks=4)
        torch.cuda.synchronize()
        ctx.sync()
        rows = [vd.gathered_index(i, n, 1, 4) for i in range(n)]
        assert np.array_equal(out.cpu().numpy()[rows], full)
    finally:
        dist.destroy_process_group()


def test_bench_two_ranks_on_one_device():
    # bench.py's N > 1 path for real (not --dry-run): two ranks, both on cuda:0 (--share-device: gloo collectives, since RCCL refuses two
    # ranks on one device), the map broadcast from rank 0, both timed regions with their barriers, the collectives behind them, the
    # max over ranks, one JSON line from rank 0.  What the driver's 8-GPU run walks, minus RCCL itself (test above).
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1", "--nproc-per-node=2",
           os.path.join(root, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-device", "--steps", "3", "--warmup", "1",
           "--sources", "48", "--no-cpu-baseline"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["config"]["sources_per_gpu"] == 48 and d["config"]["sharding"] == "sources/2"
    assert d["value"] > 0 and abs(d["value"] - 2 * 48 * 3 / (d["ms_per_step"] * 3e-3)) < 1e-3 * d["value"]
    assert d["value_first_allocation"] == d["value"] and d["roofline"]["kernel"] in ("vhp_pool_sweep", "vhp_sweep_fronts", "vhp_lat_sweep")
    assert d["config"]["self_check"]["equal"] is True
    wc = d["value_with_collective"]
    assert "error" not in wc and wc["allgather_f32"]["value"] > 0 and wc["union_fields"]["value"] > 0, wc


class _single_rank_group:
    """a world-size-1 RCCL process group on cuda:0 for the duration of a with-block"""

    def __enter__(self):
        import torch
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(_free_port())
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        return self

    def __exit__(self, *exc):
        import torch.distributed as dist
        dist.destroy_process_group()
        return False


def _padded_sweep(ctx, occ, src, pad, tdt, vdt):
    """the batch swept into a buffer whose fields are nx*ny + pad elements apart (field_stride); returns the [n, ny, nx] view"""
    import torch
    ny, nx = occ.shape
    stride = nx * ny + pad
    ctx.set_option("field_stride", stride)
    buf = torch.full((len(src) * stride,), float("nan"), dtype=tdt, device="cuda")
    d_src = torch.from_numpy(np.ascontiguousarray(src, np.int32)).cuda()
    ctx.sweep_batch_device(d_src.data_ptr(), len(src), buf.data_ptr(), dtype=vdt)
    ctx.sync()
    return buf.as_strided((len(src), ny, nx), (stride, nx, 1))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_union_fields_reads_the_fields_stride_not_the_last_sweeps(oracle, dtype):
    # a sweep with a field_stride leaves it set on the context: dist.union_fields must read its tensor as laid out (packed, or
    # padded as the sweep wrote it), restore the option and the context's stream, and equal numpy's union of the oracle's fields
    import torch
    import vhp_amd
    from importlib import import_module
    from test_union import _numpy_union
    vd = import_module("visibility-heuristic-path-planner_amd.dist")
    tdt, vdt, npdt = (torch.float64, vhp_amd.F64, np.float64) if dtype == "f64" else (torch.float32, vhp_amd.F32, np.float32)
    occ = maps.random_rect_map(200, 163, 12, 3, 30, 3, 30, 3)
    ny, nx = occ.shape
    src = maps.free_sources(occ, 9, 4)
    want = np.stack([oracle.sweep_full(occ, int(x), int(y)) for x, y in src]).astype(npdt)
    wb, wa = _numpy_union(want, 5)
    with _single_rank_group():
        ctx = vhp_amd.Context(0)
        ctx.set_map(occ)
        side = torch.cuda.Stream()
        ctx.set_stream(side.cuda_stream)
        with torch.cuda.stream(side):
            fields = _padded_sweep(ctx, occ, src, 37, tdt, vdt)
        assert np.array_equal(fields.cpu().numpy(), want)
        for what, f in (("packed", fields.contiguous()), ("padded", fields), ("one field", fields[2:3]), ("every other field", fields[::2])):
            first = 5 + (2 if what == "one field" else 0)
            best, arg = vd.union_fields(f, first, 5 + len(src), ctx=ctx)
            torch.cuda.synchronize()
            sub = want[[2]] if what == "one field" else want[::2] if what == "every other field" else want
            eb, ea = _numpy_union(sub, first)
            if what in ("packed", "padded"):
                assert np.array_equal(eb, wb) and np.array_equal(ea, wa)
            assert np.array_equal(best.cpu().numpy(), eb), "%s %s: union differs" % (dtype, what)
            assert np.array_equal(arg.cpu().numpy(), ea.astype(np.int64)), "%s %s: arg-source differs" % (dtype, what)
            assert ctx.stream == side.cuda_stream and ctx.field_stride == nx * ny + 37, what
        # the context's own option still places the next sweep's fields where the caller asked
        with torch.cuda.stream(side):
            again = _padded_sweep(ctx, occ, src, 37, tdt, vdt)
        assert np.array_equal(again.cpu().numpy(), want)


def test_union_leaves_the_sweeps_elapsed_time():
    # vhp_last_elapsed_ms reports the most recent sweep or planner call (include/vhp.h): a union behind the sweep does not replace it
    import torch
    import vhp_amd
    from importlib import import_module
    vd = import_module("visibility-heuristic-path-planner_amd.dist")
    occ = maps.random_rect_map(328, 300, 30, 3, 40, 3, 40, 5)
    src = maps.free_sources(occ, 8, 8)
    with _single_rank_group():
        ctx = vhp_amd.Context(0)
        ctx.set_map(occ)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        out = torch.empty((len(src),) + occ.shape, dtype=torch.float64, device="cuda")
        d_src = torch.from_numpy(np.ascontiguousarray(src, np.int32)).cuda()
        ctx.sweep_batch_device(d_src.data_ptr(), len(src), out.data_ptr())
        ms = ctx.last_elapsed_ms()
        assert ms > 0
        best = torch.empty(occ.shape, dtype=torch.float64, device="cuda")
        arg = torch.empty(occ.shape, dtype=torch.int32, device="cuda")
        ctx.union_fields_device(out.data_ptr(), len(src), best.data_ptr(), arg.data_ptr())
        assert ctx.last_elapsed_ms() == ms
        vd.union_fields(out, 0, len(src), ctx=ctx)
        torch.cuda.synchronize()
        assert ctx.last_elapsed_ms() == ms


def test_union_fields_refuses_fields_that_do_not_fit_the_context():
    import torch
    import vhp_amd
    from importlib import import_module
    vd = import_module("visibility-heuristic-path-planner_amd.dist")
    with _single_rank_group():
        ctx = vhp_amd.Context(0)
        ctx.set_map(np.ones((30, 40), np.uint8))
        ok = torch.zeros((3, 30, 40), dtype=torch.float64, device="cuda")
        for bad in (torch.zeros((3, 40, 30), dtype=torch.float64, device="cuda"), torch.zeros((3, 30, 41), dtype=torch.float64, device="cuda"),
                    torch.zeros((30, 40), dtype=torch.float64, device="cuda"), ok.half(), ok.to(torch.int32), ok.bfloat16()):
            with pytest.raises(ValueError):
                vd.union_fields(bad, 0, 3, ctx=ctx)
        best, arg = vd.union_fields(ok, 0, 3, ctx=ctx)
        torch.cuda.synchronize()
        assert (best == 0).all() and (arg == 0).all()
