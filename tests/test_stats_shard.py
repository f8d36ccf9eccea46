"""shard.gather_chan_stats over world-2 gloo: the per-rank statistics tables (local channel order) become one table in global
channel order (c = l * world + r), with channel counts that differ from rank to rank.  The tables are model tables: what is under
test is the sharding logic."""
import os

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

from acarsdec_amd import _capi as K
from acarsdec_amd import shard
from test_shard_gloo import free_port


def table_of(global_channels):
    """a table whose every field says which GLOBAL channel the row belongs to"""
    g = np.asarray(global_channels, dtype=np.int64)
    st = np.zeros(len(g), dtype=K.CHAN_STATS_DTYPE)
    for k, (name, _) in enumerate(K.CHAN_STATS_DTYPE[:16]):
        st[name] = (1000 * k + g).astype(np.uint32)
    st["lvl_min"], st["lvl_max"], st["last_end_sample"] = g + 0.25, g + 0.5, (g << 33) - 1
    return st


def _worker(rank, world, port, nch, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    mine = table_of(shard.owned_channels(nch, rank, world))
    out = shard.gather_chan_stats(mine, rank, world, dst=0, dist=dist)
    assert (out is None) == (rank != 0)
    if rank == 0:
        q.put(out.tobytes())
    dist.barrier()
    dist.destroy_process_group()


def test_world2_gloo_gathers_the_tables_in_global_channel_order():
    world, nch = 2, 7                                                  # rank 0 owns 4 channels, rank 1 owns 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, nch, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = np.frombuffer(q.get(timeout=240), dtype=K.CHAN_STATS_DTYPE)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert got.tobytes() == table_of(range(nch)).tobytes()
    for c in range(nch):                                               # the c mod N map
        assert int(got["blocks"][c]) == c and shard.owner_of(c, world) == c % world and shard.local_index(c, world) == c // world


def test_one_rank_needs_no_collective():
    st = table_of(range(5))
    assert shard.gather_chan_stats(st, 0, 1).tobytes() == st.tobytes()
