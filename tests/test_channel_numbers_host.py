"""Sharded hosts, the parts that need no GPU: acg_channel_numbers_check (host arithmetic), shard.merge_keyed (a k-way merge of
sorted parts) and shard.gather_keyed over gloo with a world of three."""
import os

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from acarsdec_amd import shard
from test_shard_gloo import free_port              # the launcher's helper: imported, not copied


@pytest.fixture(scope="module")
def L():
    from acarsdec_amd import _capi as K
    return K.load()


def check(L, values):
    arr = np.ascontiguousarray(np.asarray(values, dtype=np.int32))
    return L.acg_channel_numbers_check(arr.ctypes.data if len(arr) else None, len(arr))


def test_channel_numbers_check(L):
    from acarsdec_amd import _capi as K
    top = (1 << 20) - 1
    assert check(L, [0]) == K.OK
    assert check(L, [top, 0]) == K.OK
    for world in (1, 2, 3, 8):
        for rank in range(world):
            m = shard.channel_numbers(5, rank, world)
            assert m.tolist() == [l * world + rank for l in range(5)]
            assert check(L, m) == K.OK
            assert np.array_equal(m, shard.owned_channels(5 * world, rank, world))          # the inverse of the partition
    assert np.array_equal(shard.flight_channel_map(4, 1, 3), shard.channel_numbers(4, 1, 3))   # the synonym stays
    assert check(L, [3, -1, 5]) == K.EINVAL
    assert check(L, [3, 1 << 20, 5]) == K.EINVAL
    assert check(L, [7, 7, 1, 2, 3]) == K.EINVAL             # a duplicate at the first position ...
    assert check(L, [1, 2, 3, 7, 7]) == K.EINVAL             # ... and at the last
    assert check(L, [7, 1, 2, 3, 7]) == K.EINVAL             # ... and far apart
    assert check(L, []) == K.OK                              # n = 0
    assert L.acg_channel_numbers_check(None, 2) == K.EINVAL and L.acg_channel_numbers_check(None, -1) == K.EINVAL


def test_merge_keyed_equals_sorted_union():
    rng = np.random.default_rng(20261020)
    for trial in range(1000):
        nparts = 1 + trial % 8
        n = int(rng.integers(0, 60))
        keys = rng.integers(0, 1 << 40, n).astype(np.uint64) << np.uint64(int(rng.integers(0, 24)))   # up to 63 bits
        keys = np.unique(keys)
        owner = rng.integers(0, nparts, len(keys))
        if trial % 5 == 0:
            owner[owner == nparts - 1] = 0                     # an empty part
        parts = []
        for p in range(nparts):
            k = np.sort(keys[owner == p])
            parts.append((k, [b"r%d" % int(v) for v in k]))
        assert shard.merge_keyed(parts) == [b"r%d" % int(v) for v in sorted(int(v) for v in keys)], trial
    assert shard.merge_keyed([]) == [] and shard.merge_keyed([([], []), (np.zeros(0, dtype=np.uint64), [])]) == []
    top = (1 << 64) - 1                                        # the whole key is compared, not its low bits
    assert shard.merge_keyed([([1, top], ["a", "z"]), ([1 << 63], ["m"])]) == ["a", "m", "z"]


def test_merge_keyed_refuses_what_has_no_order():
    with pytest.raises(ValueError):
        shard.merge_keyed([([1, 5], [b"a", b"b"]), ([2, 5], [b"c", b"d"])])          # one key in two parts
    with pytest.raises(ValueError):
        shard.merge_keyed([([4, 4], [b"a", b"b"])])                                  # ... and twice in one
    with pytest.raises(ValueError):
        shard.merge_keyed([([5, 1], [b"a", b"b"])])                                  # a part that is not sorted
    with pytest.raises(ValueError):
        shard.merge_keyed([([1, 2], [b"a"])])                                        # keys and records differ in number


def rank_part(rank, world):
    """what rank `rank` of `world` hands in: keys of its channels (c mod world) and records of every length, a NUL, a newline and
    an empty one among them; rank 1 has nothing"""
    if rank == 1:
        return np.zeros(0, dtype=np.uint64), []
    rng = np.random.default_rng(100 + rank)
    chn = shard.channel_numbers(4, rank, world).astype(np.uint64)
    keys = np.sort(np.array([(int(c) << 44) | int(e) for c in chn for e in rng.permutation(1 << 12)[:3 + rank] * 262139], dtype=np.uint64))
    recs = [bytes(rng.integers(0, 256, int(rng.integers(0, 700)), dtype=np.uint8)) for _ in keys]
    recs[0] = b""
    recs[1] = b"\0line\n\n"
    return keys, recs


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    keys, recs = rank_part(rank, world)
    merged = shard.gather_keyed(keys, recs, dst=2, dist=dist)
    empty = shard.gather_keyed([], [], dst=0, dist=dist)        # a round in which nobody has a record
    assert (merged is None) == (rank != 2) and (empty is None) == (rank != 0)
    if rank == 2:
        q.put(merged)
    if rank == 0:
        q.put(empty)
    dist.barrier()
    dist.destroy_process_group()


def test_gather_keyed_over_gloo_with_a_world_of_three():
    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=240), q.get(timeout=240)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    parts = [rank_part(r, world) for r in range(world)]
    want = shard.merge_keyed(parts)
    pairs = sorted((int(k), r) for keys, recs in parts for k, r in zip(keys, recs))
    assert want == [r for _, r in pairs] and len(want) == 3 * 4 + 5 * 4
    assert sorted(got, key=len) == [[], want]
    # without a process group the one part is merged alone
    keys, recs = parts[0]
    assert shard.gather_keyed(keys, recs) == recs
