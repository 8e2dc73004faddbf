"""The multi-GPU source sharding, exercised on CPU with gloo at world_size 2 and 3.
The per-rank compute is injected (here: the oracle), the subject is the partition and the
collectives of dist.py."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import maps


def _worker(rank, world, port, n_sources, q):
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.dirname(here)):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import vhp_amd  # noqa: F401
    from importlib import import_module
    from oracle_lib import Oracle
    vd = import_module("visibility-heuristic-path-planner_amd.dist")
    occ = maps.random_rect_map(48, 40, 8, 2, 9, 2, 9, 3)
    src = maps.free_sources(occ, n_sources, 5)
    orc = Oracle()

    def compute(shard):
        if len(shard) == 0:
            return torch.zeros((0,) + occ.shape, dtype=torch.float64)
        return torch.from_numpy(np.stack([orc.sweep_full(occ, int(x), int(y)) for x, y in shard]))

    full = np.stack([orc.sweep_full(occ, int(x), int(y)) for x, y in src])
    local, lo = vd.sweep_sharded(compute, src, "none")
    ok = np.array_equal(local.numpy(), full[lo: lo + local.shape[0]])
    allf = vd.sweep_sharded(compute, src, "gather")
    ok &= np.array_equal(allf.numpy(), full)
    best, arg = vd.sweep_sharded(compute, src, "union")
    ok &= np.array_equal(best.numpy(), full.max(0))
    ok &= np.array_equal(arg.numpy(), (full == full.max(0)[None]).argmax(0))
    # shard arithmetic: blocks tile [0, n) exactly
    cover = sorted(sum((list(range(*vd.shard_bounds(n_sources, r, world))) for r in range(world)), []))
    ok &= cover == list(range(n_sources))
    q.put((rank, bool(ok)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_sources", [(2, 7), (2, 8), (3, 5), (2, 1)])
def test_sharded_sweep_gloo(world, n_sources):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 1000) + world * 7 + n_sources
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_sources, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok in res), res


def _worker_overlap(rank, world, port, q):
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.dirname(here)):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import vhp_amd  # noqa: F401
    from importlib import import_module
    from oracle_lib import Oracle
    vd = import_module("visibility-heuristic-path-planner_amd.dist")
    occ = maps.random_rect_map(40, 32, 6, 2, 8, 2, 8, 11)
    n, chunks = 8 * world, 2
    src = maps.free_sources(occ, n, 2)
    orc = Oracle()
    full = np.stack([orc.sweep_full(occ, int(x), int(y)) for x, y in src])
    # the map travels from rank 0
    t = torch.from_numpy(occ.copy()) if rank == 0 else torch.zeros(occ.shape, dtype=torch.uint8)
    vd.broadcast_map(t, 0)
    ok = np.array_equal(t.numpy(), occ)
    shard, lo = vd.shard_sources(src)

    def launch(a, b, dst):
        dst.copy_(torch.from_numpy(np.stack([orc.sweep_full(t.numpy(), int(x), int(y)) for x, y in shard[a:b]])))

    out = torch.full((n,) + occ.shape, -1.0, dtype=torch.float64)
    vd.sweep_gather_overlapped(launch, src, out, chunks)
    rows = [vd.gathered_index(i, n, world, chunks) for i in range(n)]
    ok &= sorted(rows) == list(range(n))
    ok &= np.array_equal(out.numpy()[rows], full)
    # equal shards: the no-copy all-gather lands every field in place
    local = torch.from_numpy(full[lo: lo + len(shard)])
    dst = torch.empty((n,) + occ.shape, dtype=torch.float64)
    got = vd.gather_fields(local, n, out=dst)
    ok &= got.data_ptr() == dst.data_ptr() and np.array_equal(got.numpy(), full)
    q.put((rank, bool(ok)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_overlapped_gather_and_map_broadcast_gloo(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29700 + (os.getpid() % 1000) + world * 13
    procs = [ctx.Process(target=_worker_overlap, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok in res), res


def test_union_fields_cpu_path_unchanged():
    # ctx=None (fields not on a GPU): the torch shim, whatever the tensor's strides or its float type; one rank of gloo
    from importlib import import_module
    from test_union import _numpy_union, _tied_fields
    vd = import_module("visibility-heuristic-path-planner_amd.dist")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        rng = np.random.RandomState(3)
        for npdt in (np.float64, np.float32):
            f = _tied_fields(rng, 8, 17, 23, npdt)
            pad = torch.full((8, 17 * 23 + 5), float("nan"), dtype=torch.from_numpy(f).dtype)
            pad[:, : 17 * 23] = torch.from_numpy(f.reshape(8, -1))
            for what, t, want in (("packed", torch.from_numpy(f), f), ("padded", pad[:, : 17 * 23].view(8, 17, 23), f),
                                  ("every other", torch.from_numpy(f)[::2], f[::2])):
                best, arg = vd.union_fields(t, 4, 12)
                wb, wa = _numpy_union(want, 4)
                assert best.dtype == t.dtype and arg.dtype == torch.int64, what
                assert np.array_equal(best.numpy(), wb) and np.array_equal(arg.numpy(), wa), what
    finally:
        dist.destroy_process_group()
