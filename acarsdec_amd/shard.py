"""Channel sharding across the GPUs of a node.

Channels are independent units: a channel's down-converter and demodulator state never touches
another channel's, so the multi-GPU path is a pure partition -- rank r owns channels
{c : c mod world == r} (BASELINE.json configs[3]: "sharded round-robin"), generates/receives its
own input and keeps its own state.  There is NO data-path collective.  torch.distributed (RCCL on
GPUs, gloo in the CPU tests) carries only the trivial exchanges: the per-channel configuration from
rank 0 (ONE BROADCAST of the whole table, 32 B per channel, from which every rank keeps its own rows --
not an ncclSend/Recv scatter: 0.5 MB at 16 384 channels is not worth one), the barrier around the
timed region and the reduction/gather of counts, timings and decoded blocks -- and, where ONE flight
table is kept for all channels, each round's flight events (88 B per message that reaches addFlight())
on their way to the rank that owns the table, and each round's rendered records with their order keys (gather_keyed) on their
way to the rank that writes the one output stream.
"""
import numpy as np


def owned_channels(nch_total, rank, world):
    """Global channel ids owned by `rank` (round-robin)."""
    return np.arange(rank, nch_total, world, dtype=np.int64)


def owner_of(channel, world):
    return int(channel) % int(world)


def local_index(channel, world):
    return int(channel) // int(world)


def scatter_channel_config(cfg_rows, world, rank, dist=None, src=0, device=None, force=False):
    """Rank `src` holds one config row per GLOBAL channel (e.g. [offset_hz, phase, track, id]); every
    rank ends up with the rows of the channels it owns.  The name says what the caller gets; the transport is a BROADCAST:
    the table is tiny (32 B per channel), so it is sent whole with the most basic collective and sliced locally; the same code
    runs over gloo (CPU tests) and RCCL (device tensors).  cfg_rows may be None on other ranks.
    force: go through the collective even with world == 1 (bench.py --rccl-selftest: the RCCL path on a one-GPU box)."""
    if dist is None or (world == 1 and not force):
        rows = np.asarray(cfg_rows, dtype=np.float64)
        return rows[owned_channels(len(rows), rank, world)]
    import torch
    dev = device if device is not None else torch.device("cpu")
    shape = torch.zeros(2, dtype=torch.int64, device=dev)
    if rank == src:
        rows = np.ascontiguousarray(np.asarray(cfg_rows, dtype=np.float64))
        shape = torch.tensor(list(rows.shape), dtype=torch.int64, device=dev)
    dist.broadcast(shape, src=src)
    n, k = int(shape[0].item()), int(shape[1].item())
    table = torch.from_numpy(rows).to(dev) if rank == src else torch.empty((n, k), dtype=torch.float64, device=dev)
    dist.broadcast(table, src=src)
    return table.cpu().numpy()[owned_channels(n, rank, world)]


def gather_blocks(local_blocks, own_ids, world, rank, dist=None, dst=0):
    """Blocks decoded on this rank carry LOCAL channel indices; returns on `dst` the merged list
    with GLOBAL channel ids, ordered by (channel, end_bit) like the single-GPU drain."""
    fixed = [(int(own_ids[b[0]]),) + tuple(b[1:]) for b in local_blocks]
    if dist is None:
        return sorted(fixed, key=lambda b: (b[0], b[-1]))
    box = [None] * world if rank == dst else None
    dist.gather_object(fixed, box, dst=dst)
    if rank != dst:
        return None
    merged = [b for part in box for b in part]
    return sorted(merged, key=lambda b: (b[0], b[-1]))


def reduce_timing(seconds, count, world, dist=None, device=None):
    """max over ranks of the timed-region duration, sum of a per-rank count.  With a `dist` handle the collectives run
    whatever the world size (a world of one still exercises the backend)."""
    if dist is None:
        return float(seconds), float(count)
    import torch
    t = torch.tensor([float(seconds)], dtype=torch.float64, device=device)
    c = torch.tensor([float(count)], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dist.all_reduce(c, op=dist.ReduceOp.SUM)
    return float(t.item()), float(c.item())


def gather_scalars(x, world, dist=None, device=None):
    """every rank's scalar, in rank order, on every rank (per-GPU timings of the bench report)."""
    if dist is None:
        return [float(x)]
    import torch
    mine = torch.tensor([float(x)], dtype=torch.float64, device=device)
    box = [torch.zeros(1, dtype=torch.float64, device=device) for _ in range(world)]
    dist.all_gather(box, mine)
    return [float(b.item()) for b in box]


def channel_numbers(nch_local, rank, world):
    """The channel numbers a rank hands out (Decoder.set_channel_numbers; for the flight table alone: Decoder.set_flight_channels):
    local channel l of rank r is the global channel l * world + r, the inverse of owned_channels."""
    return np.arange(int(nch_local), dtype=np.int32) * np.int32(world) + np.int32(rank)


flight_channel_map = channel_numbers          # the name it had while only the flight table took a map


def merge_keyed(parts):
    """The records of several contexts as the ONE stream a single context over all channels hands out.  parts: [(keys, records), ...],
    one pair per context and sink call -- keys as Decoder.sink_keys gives them (ascending within a part), records the lines /
    text records / messages that belong to them, one per key.  Returns the records in ascending key order: a k-way merge of
    inputs that are already sorted (heapq.merge, nothing is sorted again).  Raises ValueError on a part whose keys and records
    differ in number or whose keys descend, and on a key that occurs twice (two contexts under one channel number)."""
    import heapq

    def walk(k, keys, recs):
        for i, key in enumerate(keys):
            yield int(key), k, i, recs[i]

    runs = []
    for k, (keys, recs) in enumerate(parts):
        if len(keys) != len(recs):
            raise ValueError("part %d: %d keys for %d records" % (k, len(keys), len(recs)))
        if any(int(keys[i]) > int(keys[i + 1]) for i in range(len(keys) - 1)):
            raise ValueError("part %d: its keys are not ascending" % k)
        runs.append(walk(k, keys, recs))
    out, last = [], None
    for key, _, _, rec in heapq.merge(*runs):
        if key == last:
            raise ValueError("key %#x occurs twice: two records under one (channel number, end_bit)" % key)
        last = key
        out.append(rec)
    return out


def split_lines(buf):
    """The JSON sink's packed lines as a list, each with its newline (a line holds no raw newline: cJSON escapes it)"""
    return [l + b"\n" for l in bytes(buf).split(b"\n")[:-1]]


def gather_keyed(keys, records, dst=0, dist=None, device=None):
    """Every rank's (keys, records) of one round moved to `dst` and merged there (merge_keyed): the one stream of the round.
    records: a list of bytes, one per key (JSON lines: split_lines(Decoder.drain_json()); text records as Decoder.drain_text gives
    them).  The counts differ from rank to rank, so they are exchanged first (records, bytes: two int64 per rank); then ONE
    gather carries, per rank and padded to the largest, the keys, the records' offsets and the packed bytes.  CPU tensors over
    gloo, device tensors (device = the rank's GPU) over RCCL, as gather_flight_events.  Returns the merged list on `dst`, None
    elsewhere."""
    keys = np.ascontiguousarray(np.asarray(keys, dtype=np.uint64))
    records = [bytes(r) for r in records]
    if len(keys) != len(records):
        raise ValueError("%d keys for %d records" % (len(keys), len(records)))
    if dist is None:
        return merge_keyed([(keys, records)])
    import torch
    rank, world = dist.get_rank(), dist.get_world_size()
    blob = b"".join(records)
    offs = np.zeros(len(records) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in records], dtype=np.uint64)
    mine = torch.tensor([len(records), len(blob)], dtype=torch.int64, device=device)
    counts = [torch.zeros(2, dtype=torch.int64, device=device) for _ in range(world)]
    dist.all_gather(counts, mine)
    counts = [(int(c[0].item()), int(c[1].item())) for c in counts]
    nmax, bmax = max(n for n, _ in counts), max(b for _, b in counts)
    head = 8 * nmax + 8 * (nmax + 1)                                  # keys, then offsets
    width = head + max(bmax, 1)
    packed = np.zeros(width, dtype=np.uint8)
    packed[: 8 * len(keys)] = keys.view(np.uint8)
    packed[8 * nmax: 8 * nmax + 8 * len(offs)] = offs.view(np.uint8)
    packed[head: head + len(blob)] = np.frombuffer(blob, dtype=np.uint8)
    row = torch.from_numpy(packed).to(device) if device is not None else torch.from_numpy(packed)
    box = [torch.zeros(width, dtype=torch.uint8, device=device) for _ in range(world)] if rank == dst else None
    dist.gather(row, box, dst=dst)
    if rank != dst:
        return None
    parts = []
    for b, (n, _) in zip(box, counts):
        raw = b.cpu().numpy().tobytes()
        k = np.frombuffer(raw[: 8 * n], dtype=np.uint64)
        o = np.frombuffer(raw[8 * nmax: 8 * nmax + 8 * (n + 1)], dtype=np.uint64)
        parts.append((k, [raw[head + int(o[i]): head + int(o[i + 1])] for i in range(n)]))
    return merge_keyed(parts)


def gather_flight_events(events, dst=0, dist=None, device=None):
    """Every rank's flight events (Decoder.drain_flight_events: a structured array of 88-byte records) moved to `dst` as bytes.
    The counts differ from rank to rank: they are exchanged first (one int64 per rank), then ONE gather carries the records, each
    rank's padded to the largest count.  CPU tensors over gloo, device tensors (device = the rank's GPU) over RCCL, as the other
    helpers here.  Returns on `dst` the concatenation in rank order (what Decoder.import_flight_events takes; the owner's own
    part is empty when it exports nothing), None elsewhere."""
    from . import _capi as K
    ev = np.ascontiguousarray(np.asarray(events, dtype=K.FLIGHT_EVENT_DTYPE))
    if dist is None:
        return ev
    import torch
    rank, world = dist.get_rank(), dist.get_world_size()
    rec = ev.dtype.itemsize
    mine = torch.tensor([len(ev)], dtype=torch.int64, device=device)
    counts = [torch.zeros(1, dtype=torch.int64, device=device) for _ in range(world)]
    dist.all_gather(counts, mine)
    counts = [int(c.item()) for c in counts]
    width = max(max(counts), 1) * rec
    row = torch.zeros(width, dtype=torch.uint8, device=device)
    if len(ev):
        row[: len(ev) * rec] = torch.from_numpy(ev.view(np.uint8).reshape(-1).copy()).to(row.device)
    box = [torch.zeros(width, dtype=torch.uint8, device=device) for _ in range(world)] if rank == dst else None
    dist.gather(row, box, dst=dst)
    if rank != dst:
        return None
    parts = [np.frombuffer(b.cpu().numpy()[: n * rec].tobytes(), dtype=ev.dtype) for b, n in zip(box, counts)]
    return np.concatenate(parts)


def gather_chan_stats(stats, rank, world, dst=0, dist=None, device=None):
    """Every rank's per-channel statistics (Decoder.stats: a structured array of 88-byte records in LOCAL channel order) as ONE
    table in GLOBAL channel order on `dst`: local channel l of rank r is global channel l * world + r (owned_channels), and the
    channels are disjoint, so there is nothing to merge -- rows only move.  The ranks may own different numbers of channels (a
    total that is no multiple of the world): the counts are exchanged first, then ONE gather carries the rows, padded to the
    largest count.  CPU tensors over gloo, device tensors over RCCL, like gather_flight_events.  None on the other ranks."""
    from . import _capi as K
    st = np.ascontiguousarray(np.asarray(stats, dtype=K.CHAN_STATS_DTYPE))
    if dist is None:
        assert world == 1 and rank == 0
        return st
    import torch
    rec = st.dtype.itemsize
    mine = torch.tensor([len(st)], dtype=torch.int64, device=device)
    counts = [torch.zeros(1, dtype=torch.int64, device=device) for _ in range(world)]
    dist.all_gather(counts, mine)
    counts = [int(c.item()) for c in counts]
    width = max(max(counts), 1) * rec
    row = torch.zeros(width, dtype=torch.uint8, device=device)
    if len(st):
        row[: len(st) * rec] = torch.from_numpy(st.view(np.uint8).reshape(-1).copy()).to(row.device)
    box = [torch.zeros(width, dtype=torch.uint8, device=device) for _ in range(world)] if rank == dst else None
    dist.gather(row, box, dst=dst)
    if rank != dst:
        return None
    total = sum(counts)
    out = np.zeros(total, dtype=st.dtype)
    for r, (b, n) in enumerate(zip(box, counts)):
        own = owned_channels(total, r, world)
        if len(own) != n:
            raise ValueError("rank %d holds %d channels, the round-robin map gives it %d of %d" % (r, n, len(own), total))
        out[own] = np.frombuffer(b.cpu().numpy()[: n * rec].tobytes(), dtype=st.dtype)
    return out
