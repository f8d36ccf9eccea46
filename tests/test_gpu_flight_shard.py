"""One flight table for the channels of several contexts (acg_flights_set_channels / _export / _import / _commit): N contexts on
one device, channels sharded `c mod N`, rank 0 the owner.  The owner's table, monitor text, route lines and `dropped` must be
those of ONE context over all channels -- on the flight fixture that is the reference program's own output --, the peers'
tables stay empty and what their message entry points hand out does not change.  GPU box only."""
import ctypes as C

import numpy as np
import pytest

import flight_model as FM
import flight_table_model as T
import monitor_model as MM
from test_gpu_flight_text import D, fix, filter_kw          # noqa: F401  (the fixture's loaders: imported, not copied)
from test_gpu_flights import LABELS_B, T0, model_kw, random_records, synthetic_traffic

pytestmark = pytest.mark.gpu

assert T0 == MM.T0


def shard_maps(nch, world):
    from acarsdec_amd import shard
    own = [shard.owned_channels(nch, r, world) for r in range(world)]
    return own, [shard.flight_channel_map(len(o), r, world) for r, o in enumerate(own)]


def make_decoder(D, nch, chunk, kw, fl, text=None):
    dec = D.Decoder(nch, decim=8, ntaps=8, max_blocks=chunk // 1024, repair=True, bitlog=False)
    if kw:
        dec.set_msg_filter(**kw)
    dec.enable_flights(**fl)
    if text is not None:
        dec.enable_flight_text(*text)
    return dec


class Sharded:
    """`world` contexts over the rows of x, rank 0 the owner (with the text renderer), ranks 1 .. exporting; beside every peer a
    twin with export off, whose message entry points must hand out the same bytes"""

    def __init__(self, D, nch, world, chunk, kw, fl, text):
        self.own, maps = shard_maps(nch, world)
        self.decs = [make_decoder(D, len(o), chunk, kw, fl, text if r == 0 else None) for r, o in enumerate(self.own)]
        self.twins = [None] + [make_decoder(D, len(o), chunk, kw, fl) for o in self.own[1:]]
        for d, m in zip(self.decs, maps):
            d.set_flight_channels(m)
        for d in self.decs[1:]:
            d.export_flights(True)
        self.owner = self.decs[0]
        self.exported = 0

    def round(self, xs, max_msgs=4096):
        """one round of the contract: a process call everywhere, the peers' message entry points and drains, the import, the
        owner's message entry point; returns the owner's messages"""
        for d, t, o in zip(self.decs, self.twins, self.own):
            d.demod_msk(xs[o])
            if t:
                t.demod_msk(xs[o])
        for d, t in zip(self.decs[1:], self.twins[1:]):
            mine = [bytes(m) for m in d.drain_msgs(max_msgs=max_msgs)]
            assert mine == [bytes(m) for m in t.drain_msgs(max_msgs=max_msgs)]
            ev = d.drain_flight_events()
            assert d.flights() == [] and d.drain_routes() == [] and d.flights_dropped == 0
            assert len({(int(e["end_sample"]), int(e["chn"])) for e in ev}) == len(ev)
            self.exported += len(ev)
            self.owner.import_flight_events(ev)
        return self.owner.drain_msgs(max_msgs=max_msgs)

    def close(self):
        for d in self.decs + self.twins[1:]:
            d.close()


# ---- 5: the fixture, end to end ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [3, 2])
@pytest.mark.parametrize("v", ["none", "A", "e", "b", "Aeb"])
def test_fixture_sharded_equals_the_single_context_and_the_reference(D, fix, v, world):
    """The 3-channel flight fixture by three 1-channel contexts and by two (channels 0, 2 and channel 1), in calls of 4096 samples.
    After EVERY round the owner's monitor frame and the route lines it drains are byte for byte the single context's -- and,
    masked where the reference stamps its wall clock, the reference's frame for each delivered message and its route lines."""
    x, fg, mg = fix
    nch, chunk, gv = mg["nch"], 4096, mg["variants"][v]
    kw = filter_kw(gv["args"], fg["label_list"])
    fl = dict(t0=T0, mdly=600, max_flights=64)
    station = mg["station"].encode("latin1") if v == "none" else b""
    want_routes = mg["station_routes"] if v == "none" else gv["routes"]
    head = MM.CLS + mg["header"].encode("latin1")
    ref = [head + b"".join(mg["rows"][i].encode("latin1") + b"\n" for i in ids) for ids in gv["frames"]]
    one = make_decoder(D, nch, chunk, kw, fl, (nch, station))
    sh = Sharded(D, nch, world, chunk, kw, fl, (nch, station))
    k, lines, idle = 0, b"", 0
    for s in range(0, x.shape[1], chunk):
        one.demod_msk(x[:, s:s + chunk])
        msgs = one.drain_msgs()
        mine = sh.round(x[:, s:s + chunk])
        idle += bool(msgs) and not mine                                   # the owner consumed nothing, the pass ran over imports alone
        hdr = msgs[0].soh_sample if msgs else -1
        got = sh.owner.monitor_text(hdr)
        assert got == one.monitor_text(hdr), (v, s)
        assert [bytes(f) for f in sh.owner.flights()] == [bytes(f) for f in one.flights()], (v, s)
        if msgs:
            assert len(msgs) == 1 and MM.mask_times(got) == ref[k], (v, k)
            k += 1
        part = sh.owner.drain_routes_json()
        assert part == one.drain_routes_json(), (v, s)
        lines += part
    sh.owner.commit_flights()                                              # nothing queued: a no-op
    assert sh.owner.monitor_text(-1) == one.monitor_text(-1)
    assert k == len(ref) and k > 0 and sh.exported > 0 and idle > 0, (v, k, sh.exported, idle)
    assert [MM.mask_route(ln + b"\n") for ln in lines.split(b"\n")[:-1]] == [r.encode("latin1") for r in want_routes], v
    one.close()
    sh.close()


# ---- 6, 7: records through acg_selftest_flights_sharded ------------------------------------------------------------------------------
def run_sharded(D, recs, sizes, nshards, cap, mdly, kw, timed=False):
    """([the owner's entries after every round], [its routes], [dropped after every round], pass_ms or None)"""
    from acarsdec_amd import _capi as K
    f = D.make_msg_filter(**kw)
    cfg = K.FlightConfig(T0[0], T0[1], mdly, cap)
    snap_cap, route_cap = min(cap, 1024) * len(sizes), sum(sizes)
    snaps, routes = (K.Flight * snap_cap)(), (K.Route * max(route_cap, 1))()
    nb = len(sizes)
    snap_n, nroutes, dropped, ms = (C.c_int * nb)(), C.c_int(0), (C.c_int * nb)(), (C.c_float * nb)()
    rc = K.load().acg_selftest_flights_sharded(recs, (C.c_int * nb)(*sizes), nb, nshards, C.byref(cfg), C.byref(f), snaps, snap_cap, snap_n,
                                               routes, route_cap, C.byref(nroutes), dropped, ms if timed else None)
    assert rc == K.OK, rc
    blob, out, at = bytes(snaps), [], 0
    for b in range(nb):
        out.append([blob[120 * i:120 * i + 120] for i in range(at, at + snap_n[b])])
        at += snap_n[b]
    return out, [bytes(routes[i]) for i in range(nroutes.value)], list(dropped), list(ms) if timed else None


def shuffle_rounds(K, rng, recs, sizes):
    out, at, sz = (K.Msg * max(sum(sizes), 1))(), 0, C.sizeof(K.Msg)
    for s in sizes:
        for j, i in enumerate(rng.permutation(s)):
            C.memmove(C.addressof(out) + (at + j) * sz, C.addressof(recs) + (at + int(i)) * sz, sz)
        at += s
    return out


def test_random_traffic_through_four_tables_equals_the_list_walk(D):
    """20 000 random records over 64 global channels (about 13 000 events once -A, -b and the ETX-only blocks are off; 600
    aircraft, one with a third of the traffic), rounds of 1 .. 500 shuffled inside, mdly = 2, through four tables `c mod 4`: the
    owner's snapshot after every tenth round and the last, its routes and `dropped` are the list walk's bytes, and ALL snapshots
    are those of the single-table self test.  Round 7 has no record of the owner's (its pass is acg_flights_commit's, over the
    imports alone); rounds 3 and 4 are empty and a single record."""
    from acarsdec_amd import _capi as K
    rng = np.random.default_rng(20261021)
    n, nsh = 20000, 4
    recs = random_records(K, rng, n, 600, 64)
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(int(rng.integers(1, 501)), n - sum(sizes)))
    sizes[int(np.argmax(sizes))] -= 1
    sizes[3:3] = [0, 1]
    assert sum(sizes) == n and max(sizes) <= 500 and sizes[7] > 20
    at7 = sum(sizes[:7])
    for i in range(at7, at7 + sizes[7]):                                  # round 7: nothing on the owner's channels
        if recs[i].chn % nsh == 0:
            recs[i].chn += 1 + int(rng.integers(0, 3))
    kw = dict(downlink_only=True, skip_empty=True, labels=LABELS_B)
    shuffled = shuffle_rounds(K, rng, recs, sizes)
    got = run_sharded(D, shuffled, sizes, nsh, 2048, 2, kw, timed=True)
    single = run_sharded(D, shuffled, sizes, 1, 2048, 2, kw)
    assert got[:3] == single[:3]
    assert set(got[2]) == {0} and all(t > 0 for t in got[3])
    walk = FM.ListWalk(2)
    at = nev = imported = 0
    for b, s in enumerate(sizes):
        evs = [e for e in (FM.event_of(recs[i], T0, **model_kw(kw)) for i in range(at, at + s)) if e is not None]
        at += s
        nev += len(evs)
        imported += sum(e.chn % nsh != 0 for e in evs)
        if b == 7:
            assert len(evs) > 10 and all(e.chn % nsh for e in evs)
        for e in FM.batch_order(evs):
            walk.add(e)
        if b % 10 == 0 or b in (7, len(sizes) - 1):
            assert got[0][b] == [FM.flight_bytes(x) for x in walk.entries()], b
    assert nev > 10000 and imported > nev // 2 and len(walk.routes) > 50 and walk.recreated > 100
    assert got[1] == [FM.route_bytes(r) for r in walk.routes]


def crowd_traffic():
    """120 aircraft one per round, 5 ms apart, all live; then ONE round with 100 new aircraft (2 .. 4 events each) and 40 events
    of the 120, over 64 channels, i.e. over all four shards.  In a table of 128 slots every window is the whole table: 8 free
    slots for 100 claims, some of them the owner's own and most of them imported."""
    rng = np.random.default_rng(79)
    S = [b"A%05d" % i for i in range(220)]
    batches, _ = T._crowd(rng, S, 120, S[120:220], lambda: int(rng.integers(2, 5)), [S[int(i)] for i in rng.integers(0, 120, 40)])
    recs = T.build_records(rng, [it for b in batches for it in b], soh_back=(600, 1200))
    return T.Traffic(recs, [len(b) for b in batches], S=S)


def test_pressure_a_hundred_new_aircraft_of_four_shards_for_eight_slots(D):
    """Exactly 92 are dropped and 128 present (nobody placeable is dropped: every free slot is taken); who is present has its
    complete entry -- the list walk with the absent left out, byte for byte, routes included; before that round nothing is dropped
    and every snapshot is the plain list walk's.  WHO gets the 8 slots is unspecified and not asserted."""
    from acarsdec_amd import _capi as K
    tr = crowd_traffic()
    S, a8 = tr.S, T.addr8
    last = tr.batches[120]
    new_by_shard = [len({e.addr for e in last if e.chn % 4 == r and e.addr in {a8(a) for a in S[120:]}}) for r in range(4)]
    assert all(c > 10 for c in new_by_shard), new_by_shard                # own and imported claims contend
    recs = tr.shuffled(np.random.default_rng(95))
    got = run_sharded(D, recs, tr.sizes, 4, 128, T.MDLY, T.filter_kw())
    whole = T.expect_without(dict(mdly=T.MDLY), tr.batches, [()] * 121)
    assert got[2] == [0] * 120 + [92]
    assert got[0][:120] == whole[0][:120]
    present = {b[:8]: b for b in got[0][120]}
    assert len(present) == len(got[0][120]) == 128 and set(present) >= {a8(a) for a in S[:120]} and set(present) <= {a8(a) for a in S}
    gone = [a for a in S[120:] if a8(a) not in present]
    assert len(gone) == 92
    want = T.expect_without(dict(mdly=T.MDLY), tr.batches, [()] * 120 + [gone])
    assert got[0][120] == want[0][120] and got[1] == want[1] and want[2] == 92


def test_pressure_contended_claims_of_one_window_across_four_shards(D):
    """tests/test_gpu_flight_pressure.py's contended traffic (a hundred claims for the hundred free slots of ONE probe window of a
    1024-slot table, then five that cannot fit and forty from elsewhere) with its records spread over four shards: every
    snapshot, the routes and `dropped` (0 .. 0, 5) as determined there."""
    tr = T.contended_traffic()
    want = T.expect_without(dict(mdly=T.MDLY), tr.batches, tr.gone)
    assert len({e.chn % 4 for e in tr.batches[28]}) == 4
    got = run_sharded(D, tr.shuffled(np.random.default_rng(96)), tr.sizes, 4, T.CAP, T.MDLY, T.filter_kw())
    assert got[0] == want[0] and got[1] == want[1]
    assert got[2] == [0] * 29 + [5] and want[2] == 5


# ---- 8: real signal -------------------------------------------------------------------------------------------------------------------
def test_real_signal_two_contexts_equal_one(D):
    """8 channels of synthetic 12.5 kHz audio, 6.5 s, four aircraft heard on channels of both shards, through the demodulator in
    five calls of 16 384 samples: one context of 8 channels against two of 4 (`c mod 2`).  After every round monitor text,
    route lines and snapshot are identical."""
    nch, chunk = 8, 16384
    x = synthetic_traffic(nch, 5 * chunk, 4, 15, per_channel=6)
    kw = dict(downlink_only=True, skip_empty=True, labels=LABELS_B)
    fl = dict(t0=T0, mdly=600, max_flights=64)
    one = make_decoder(D, nch, chunk, kw, fl, (nch, b"ST1"))
    sh = Sharded(D, nch, 2, chunk, kw, fl, (nch, b"ST1"))
    nmsgs = 0
    for s in range(0, x.shape[1], chunk):
        one.demod_msk(x[:, s:s + chunk])
        msgs = one.drain_msgs()
        nmsgs += len(msgs)
        sh.round(x[:, s:s + chunk])
        assert sh.owner.monitor_text(-1) == one.monitor_text(-1), s
        assert [bytes(f) for f in sh.owner.flights()] == [bytes(f) for f in one.flights()], s
        assert sh.owner.drain_routes_json() == one.drain_routes_json(), s
    fl_one = one.flights()
    both = [f for f in fl_one if f.chm & 0x55 and f.chm & 0xAA]           # heard on even (owner) and odd (peer) channels
    print("messages", nmsgs, "events exported", sh.exported, "entries", len(fl_one), "on both shards", len(both))
    assert nmsgs > 10 and sh.exported > 3 and len(fl_one) >= 2 and both and sum(f.nbm for f in fl_one) > sh.exported
    one.close()
    sh.close()


# ---- 9: states ------------------------------------------------------------------------------------------------------------------------
def test_states_and_queues(D):
    from acarsdec_amd import _capi as K
    L = K.load()
    nch, chunk = 8, 16384
    x = synthetic_traffic(nch, 2 * chunk, 6, 16, per_channel=3)
    ev3, n = np.zeros(3, dtype=K.FLIGHT_EVENT_DTYPE), C.c_int(-1)
    dec = D.Decoder(nch, decim=8, ntaps=8, max_blocks=chunk // 1024, repair=True, bitlog=False)
    # the table off: everything is ACG_ESTATE
    good = np.zeros(2, dtype=K.FLIGHT_EVENT_DTYPE)
    good["addr"], good["chn"], good["end_sample"] = b"N1", (1, 2), (40000, 40001)
    assert L.acg_flight_events_check(good.ctypes.data, 2) == K.OK
    assert L.acg_flights_import(dec.ctx, good.ctypes.data, 2) == K.ESTATE
    assert L.acg_flights_export(dec.ctx, 1) == K.ESTATE and L.acg_flights_commit(dec.ctx) == K.ESTATE
    assert L.acg_drain_flight_events(dec.ctx, ev3.ctypes.data, 3, C.byref(n)) == K.ESTATE and n.value == 0
    assert L.acg_flights_set_channels(dec.ctx, None) == K.ESTATE
    dec.enable_flights(t0=T0, mdly=600, max_flights=64)
    # the table on, export off: no event queue to drain; a map outside 20 bits is refused
    assert L.acg_drain_flight_events(dec.ctx, ev3.ctypes.data, 3, C.byref(n)) == K.ESTATE
    bad_map = np.arange(nch, dtype=np.int32)
    bad_map[5] = 1 << 20
    assert L.acg_flights_set_channels(dec.ctx, bad_map.ctypes.data) == K.EINVAL
    bad_map[5] = -1
    assert L.acg_flights_set_channels(dec.ctx, bad_map.ctypes.data) == K.EINVAL
    dec.set_flight_channels(np.arange(nch) * 2 + 1)
    # a rejected import queues nothing; an accepted one waits for the next pass
    bad = good.copy()
    bad["usec"][1] = 1000000
    assert L.acg_flights_import(dec.ctx, bad.ctypes.data, 2) == K.EINVAL
    dec.commit_flights()
    assert dec.flights() == []
    dec.import_flight_events(good)
    assert dec.flights() == []                                            # (not applied yet)
    dec.commit_flights()
    got = dec.flights()
    assert len(got) == 1 and got[0].nbm == 2 and got[0].addr == b"N1" and (got[0].first_chn, got[0].last_chn, got[0].chm) == (1, 2, 6)
    # acg_reset empties the import queue (and the table), and keeps the map
    dec.import_flight_events(good)
    dec.reset()
    dec.commit_flights()
    assert dec.flights() == []
    dec.demod_msk(x[:, :chunk])
    dec.drain_msgs()
    own = dec.flights()
    assert own and all(f.first_chn % 2 == 1 and f.chm & 0x5555 == 0 for f in own)      # the map: local l is recorded as 2 l + 1
    # disabling the table empties the queue as well
    dec.import_flight_events(good)
    dec.disable_flights()
    dec.enable_flights(t0=T0, mdly=600, max_flights=64)
    dec.commit_flights()
    assert dec.flights() == []
    dec.set_flight_channels(np.arange(nch) * 2 + 1)                       # (the new table has no map)
    # export: the table stays empty, an exporting context takes no imports, a 3-record buffer loses nothing
    dec.reset()
    dec.export_flights(True)
    assert L.acg_flights_import(dec.ctx, good.ctypes.data, 2) == K.ESTATE and L.acg_flights_commit(dec.ctx) == K.ESTATE
    dec.demod_msk(x[:, :chunk])
    dec.demod_msk(x[:, chunk:])
    msgs = dec.drain_msgs()
    want = sum(FM.event_of(m, T0) is not None for m in msgs)
    assert want > 6 and dec.flights() == []
    parts, calls = [], 0
    while True:
        rc = L.acg_drain_flight_events(dec.ctx, ev3.ctypes.data, 3, C.byref(n))
        parts.append(ev3[:n.value].copy())
        calls += 1
        assert rc in (K.OK, K.EAGAIN) and (n.value == 3 or rc == K.OK)
        if rc == K.OK:
            break
    got = np.concatenate(parts)
    assert len(got) == want and calls == (want + 2) // 3 and L.acg_flight_events_check(got.ctypes.data, len(got)) == K.OK
    model = sorted((e.end, e.chn, e.soh, e.sec, e.usec, e.addr, e.fid, int(e.e_ok), b"".join(x + b"\0" for x in e.fields))
                   for e in (FM.event_of(m, T0) for m in msgs) if e is not None)
    mine = sorted((int(e["end_sample"]), (int(e["chn"]) - 1) // 2, int(e["soh_sample"]), int(e["sec"]), int(e["usec"]), bytes(e["addr"]).ljust(8, b"\0"),
                   bytes(e["fid"]).ljust(7, b"\0"), int(e["e_ok"]), bytes(e["oooi"])[:35]) for e in got)
    assert mine == model and all(int(e["chn"]) % 2 == 1 for e in got)
    assert L.acg_drain_flight_events(dec.ctx, ev3.ctypes.data, 3, C.byref(n)) == K.OK and n.value == 0
    # reset empties the export queue; switching export off empties it too and the table works again
    dec.reset()
    dec.demod_msk(x[:, :chunk])
    dec.drain_msgs()
    dec.reset()
    assert len(dec.drain_flight_events()) == 0
    dec.demod_msk(x[:, :chunk])
    dec.drain_msgs()
    dec.export_flights(False)
    assert L.acg_drain_flight_events(dec.ctx, ev3.ctypes.data, 3, C.byref(n)) == K.ESTATE
    dec.export_flights(True)
    assert len(dec.drain_flight_events()) == 0
    dec.export_flights(False)
    dec.demod_msk(x[:, chunk:])
    dec.drain_msgs()
    assert dec.flights() and dec.flights()[0].first_chn % 2 == 1
    dec.close()
