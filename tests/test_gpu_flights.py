"""The flight table on the device (flight.hip) against the reference program's monitor frames and route lines for the flight
fixture, against the list-walk model (tests/flight_model.py) on random records and on synthetic traffic, and the contract of
the entry points that carry it.  GPU box only."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
import flight_model as FM
import label_model as LM

pytestmark = pytest.mark.gpu

T0 = (1700000000, 250000)
AIRPORTS = [b"KJFK", b"EGLL", b"LFPG", b"EDDF", b"KBOS", b"LEMD"]
LABELS_B = "QP:QA:QN:12:H1:Q1"                       # the -b list of these tests: QM and 2Z stay outside


@pytest.fixture(scope="module")
def D():
    from acarsdec_amd import decoder
    from acarsdec_amd import _capi as K
    assert K.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return decoder


def filter_kw(args, label_list):
    return dict(downlink_only="-A" in args, skip_empty="-e" in args, labels=label_list if "-b" in args else None)


def model_kw(kw):
    return dict(downlink_only=kw["downlink_only"], skip_empty=kw["skip_empty"], labels=LM.parse_label_filter(kw["labels"]) if kw["labels"] else ())


def label_text(rng, label):
    """a text that the label's decoder takes (or, now and then, does not); one airport in twenty starts with a NUL byte: such a
    field counts as empty (output.c:392-398 tests the first byte), whatever follows it"""
    ap = lambda: (b"\0" + AIRPORTS[int(rng.integers(0, len(AIRPORTS)))][1:]) if rng.random() < 0.05 else AIRPORTS[int(rng.integers(0, len(AIRPORTS)))]
    hhmm = lambda: b"%04d" % int(rng.integers(0, 2400))
    if label == b"QP":
        return ap() + ap() + hhmm()
    if label == b"QA":
        return ap() + hhmm()
    if label == b"QN":
        return b"XXXX" + ap() + hhmm()
    if label == b"QM":
        return ap() + b"ABCD" + ap()
    if label == b"12":
        return ap() + (b"," if rng.random() < 0.8 else b";") + ap() + b"REST"
    if label == b"2Z":
        return ap()
    return b"FREE TEXT %d" % int(rng.integers(0, 1000))


# ---- random records through acg_selftest_flights -----------------------------------------------------------------------------
def random_records(K, rng, n, naircraft, nch):
    """n split records in time order: a third from one aircraft, the rest from `naircraft`; uplinks, ETX-only blocks, empty
    texts, empty flight ids; about 10 ms between completions, with a 5 s silence now and then"""
    recs = (K.Msg * n)()
    gaps = np.where(rng.random(n) < 0.002, rng.uniform(2.0, 5.0, n), rng.exponential(0.01, n))
    end = 30000 + np.cumsum(np.rint(gaps * 12500).astype(np.int64) + 1)
    labels = [b"QP", b"QA", b"QN", b"QM", b"12", b"2Z", b"H1"]
    for i in range(n):
        m = recs[i]
        m.chn = int(rng.integers(0, nch))
        m.end_sample = int(end[i])
        m.end_bit = int(end[i]) // 5
        m.soh_sample = int(end[i]) - int(rng.integers(600, 10200))     # a block of 13 .. 241 bytes
        m.mode = b"2"
        m.addr = b"HOT1" if rng.random() < 1 / 3 else b"N%05d" % int(rng.integers(0, naircraft))
        down = rng.random() < 0.85
        m.bid = b"5" if down else b"A"
        m.down = b"\x01" if down else b"\x00"
        m.ack = b"!"
        lab = labels[int(rng.integers(0, len(labels)))]
        m.label = lab
        etx_only = rng.random() < 0.05
        m.bs = b"\x03" if etx_only else b"\x02"
        m.be = b"\x03"
        if down and not etx_only:
            m.no = b"M01A"
            m.fid = b"" if rng.random() < 0.1 else b"XY%04d" % int(rng.integers(0, 40))
        if not etx_only and rng.random() < 0.85:
            t = label_text(rng, lab)
            C.memmove(C.addressof(m) + K.Msg.txt.offset, t, len(t))
            m.txt_len = len(t)
    return recs


def test_selftest_flights_equals_the_list_walk_on_random_records(D):
    """180 000 records (at least 100 000 events once -A, -b and the ETX-only blocks are off, 5 000 aircraft, one of them with a
    third of the traffic; fields whose first byte is NUL among them) in batches of 1 .. 20 000,
    shuffled inside each batch, mdly = 2 so that entries expire inside batches and between them, all three filters: the
    snapshot after every batch (order and every byte) and the route list equal the list walk's."""
    from acarsdec_amd import _capi as K
    rng = np.random.default_rng(20261018)
    n = 180000
    recs = random_records(K, rng, n, 5000, 1024)
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(int(rng.integers(1, 20001)), n - sum(sizes)))
    sizes[int(np.argmax(sizes))] -= 4
    sizes[1:1] = [1, 0, 3]                                             # (and the smallest batches, an empty one among them)
    assert sum(sizes) == n and min(sizes) >= 0
    # the device gets each batch in an arbitrary order (as the block queue delivers it) and has to sort it itself
    shuffled = (K.Msg * n)()
    at = 0
    for s in sizes:
        for j, i in enumerate(rng.permutation(s)):
            C.memmove(C.addressof(shuffled) + (at + j) * C.sizeof(K.Msg), C.addressof(recs) + (at + int(i)) * C.sizeof(K.Msg), C.sizeof(K.Msg))
        at += s
    kw = dict(downlink_only=True, skip_empty=True, labels=LABELS_B)
    f = D.make_msg_filter(**kw)
    cfg = K.FlightConfig(T0[0], T0[1], 2, 8192)
    snap_cap, route_cap = 600000, n
    snaps, routes = (K.Flight * snap_cap)(), (K.Route * route_cap)()
    snap_n, nroutes, dropped = (C.c_int * len(sizes))(), C.c_int(0), C.c_int(0)
    rc = K.load().acg_selftest_flights(shuffled, (C.c_int * len(sizes))(*sizes), len(sizes), C.byref(cfg), C.byref(f), snaps, snap_cap, snap_n,
                                       routes, route_cap, C.byref(nroutes), C.byref(dropped))
    assert rc == K.OK, rc
    assert dropped.value == 0
    walk = FM.ListWalk(2)
    at = sat = nev = hot = 0
    for b, s in enumerate(sizes):
        evs = [e for e in (FM.event_of(recs[i], T0, **model_kw(kw)) for i in range(at, at + s)) if e is not None]
        at += s
        nev += len(evs)
        hot += sum(e.addr.startswith(b"HOT1") for e in evs)
        for e in FM.batch_order(evs):
            walk.add(e)
        want = [FM.flight_bytes(x) for x in walk.entries()]
        assert snap_n[b] == len(want), (b, snap_n[b], len(want))
        got = [bytes(snaps[sat + i]) for i in range(snap_n[b])]
        assert got == want, (b, next(i for i in range(len(want)) if got[i] != want[i]))
        sat += snap_n[b]
    nul_first = sum(1 for i in range(n) if recs[i].txt_len >= 8 and 0 in (recs[i].txt[0], recs[i].txt[4]))
    assert nev >= 100000 and hot > nev // 4 and len(walk.routes) > 500 and nul_first > 1000 and walk.recreated > 1000
    assert [bytes(routes[i]) for i in range(nroutes.value)] == [FM.route_bytes(r) for r in walk.routes]


# ---- synthetic traffic through the whole chain ------------------------------------------------------------------------------
def synthetic_traffic(nch, nsamp, naircraft, seed, per_channel=3, same_addr=False):
    """[nch, nsamp] float32 audio: per channel a few transmissions from `naircraft` aircraft (labels and texts as above,
    uplinks and empty texts among them), at random places"""
    from acarsdec_amd import synth as S
    rng = np.random.default_rng(seed)
    x = np.zeros((nch, nsamp), dtype=np.float32)
    labels = [b"QP", b"QA", b"QN", b"QM", b"12", b"H1"]
    for c in range(nch):
        pos = int(rng.integers(500, 3000))
        for _ in range(per_channel):
            lab = labels[int(rng.integers(0, len(labels)))]
            down = rng.random() < 0.85
            text = b"" if rng.random() < 0.1 else label_text(rng, lab)
            if down and text:
                text = b"M01A" + (b"XY%04d" % int(rng.integers(0, 40))) + text
            addr = b".HOT001" if same_addr else b".N%05d" % int(rng.integers(0, naircraft))
            fr = S.acars_frame(text=text, addr=addr, label=lab, bid=b"4" if down else b"B")
            a = S.msk_audio(S.frame_bits(fr), phase0=float(rng.uniform(0, 2 * np.pi)))
            if pos + a.size + 200 > nsamp:
                break
            x[c, pos:pos + a.size] = 0.06 * a
            pos += a.size + int(rng.integers(1500, 6000))
    return x


def play(D, x, chunk, lag, flights=None, filt=None, max_msgs=65536, oooi=False, max_lag=2):
    """x through a context in calls of `chunk` samples, collected with `lag` after every call and drained at the end:
    (decoder, messages per collect)"""
    nch = x.shape[0]
    dec = D.Decoder(nch, decim=8, ntaps=8, max_blocks=chunk // 1024, repair=True, bitlog=False, max_lag=max_lag)
    if filt:
        dec.set_msg_filter(**filt)
    if flights:
        dec.enable_flights(**flights)
    out = []
    for s in range(0, x.shape[1], chunk):
        dec.demod_msk(x[:, s:s + chunk])
        out.append(dec.collect_msgs(lag=lag, max_msgs=max_msgs, oooi=oooi))
    out.append(dec.drain_msgs(max_msgs=max_msgs, oooi=oooi))
    return dec, out


def model_of(msgs, kw, mdly, t0=T0):
    """the list walk over delivered-or-not messages in global (end_sample, chn) order.  msgs must be ALL messages the split
    hands out without -e (the pass sees them before -e drops any)."""
    evs = [e for e in (FM.event_of(m, t0, **model_kw(kw)) for m in msgs) if e is not None]
    walk = FM.ListWalk(mdly)
    for e in FM.batch_order(evs):
        walk.add(e)
    return walk, evs


FL = dict(t0=T0, mdly=600, max_flights=1024)
NOFILT = dict(downlink_only=False, skip_empty=False, labels=None)


def test_chunk_invariance_on_1024_channels(D):
    """1024 channels, about 300 aircraft, calls of 1024 / 4096 / 8192 samples, collected with lag 0 / 1 / 2 through buffers that
    never fill: the final snapshot and the route list are the same bytes in all nine runs and equal the list walk over the
    messages in (end_sample, chn) order."""
    nch, nsamp = 1024, 32768
    x = synthetic_traffic(nch, nsamp, 300, 11)
    kw = dict(downlink_only=True, skip_empty=True, labels=LABELS_B)
    # what the pass sees: everything -A / -b let through, -e not yet applied
    ref, out = play(D, x, 8192, 0, filt=dict(kw, skip_empty=False))
    ref.close()
    seen = [m for part in out for m in part]
    assert len(seen) > 1500
    walk, evs = model_of(seen, kw, FL["mdly"])
    want = ([FM.flight_bytes(f) for f in walk.entries()], [FM.route_bytes(r) for r in walk.routes])
    assert len(want[0]) > 250 and len(want[1]) > 50
    for chunk in (1024, 4096, 8192):
        for lag in (0, 1, 2):
            dec, out = play(D, x, chunk, lag, flights=FL, filt=kw)
            got = ([bytes(f) for f in dec.flights()], [bytes(r) for r in dec.drain_routes()])
            assert dec.flights_dropped == 0
            dec.close()
            assert got[0] == want[0], (chunk, lag)
            assert got[1] == want[1], (chunk, lag)


def test_delivered_records_do_not_change(D):
    """two contexts on the same input, one with the table: collect_msgs and collect_msgs_oooi hand out the same bytes"""
    x = synthetic_traffic(64, 32768, 20, 12)
    for filt in (None, dict(downlink_only=True, skip_empty=True, labels=LABELS_B)):
        for oooi in (False, True):
            a, out_a = play(D, x, 4096, 1, filt=filt, oooi=oooi)
            b, out_b = play(D, x, 4096, 1, flights=FL, filt=filt, oooi=oooi)
            flat = lambda out: [bytes(m) if not oooi else (bytes(m[0]), bytes(m[1])) for part in out for m in part]
            assert [len(p) for p in out_a] == [len(p) for p in out_b]
            assert flat(out_a) == flat(out_b) and len(flat(out_a)) > (30 if filt else 100)
            assert len(b.flights()) > 5
            a.close()
            b.close()


def test_eagain_loses_nothing(D):
    """drained through a 5-record buffer (every call ACG_EAGAIN until the queue is empty), mdly 600: every eligible message is
    counted in some entry, and the routes (as a set: a call that returns ACG_EAGAIN consumes an arbitrary oldest part of the
    queue, so only the per-call order is promised) are those of the large-buffer run"""
    x = synthetic_traffic(64, 32768, 20, 13)
    key = lambda r: (bytes(r.fid), bytes(r.sa), bytes(r.da), bytes(r.addr))
    big, out = play(D, x, 8192, 0, flights=FL)
    msgs = [m for part in out for m in part]
    eligible = sum(FM.event_of(m, T0) is not None for m in msgs)
    assert eligible > 100 and sum(f.nbm for f in big.flights()) == eligible
    routes_big = sorted(key(r) for r in big.drain_routes())
    big.close()
    small, out = play(D, x, 8192, 0, flights=FL, max_msgs=5)
    assert sum(len(p) for p in out) == len(msgs)
    assert sum(f.nbm for f in small.flights()) == eligible
    assert sorted(key(r) for r in small.drain_routes()) == routes_big and len(routes_big) > 3
    small.close()


def test_table_state_handling(D):
    """a table smaller than the aircraft count counts what it drops exactly and keeps what fitted; acg_reset empties table and
    routes; disable + enable starts empty; enable needs ACG_F_REPAIR"""
    from acarsdec_amd import _capi as K
    x = synthetic_traffic(64, 16384, 1000, 14, per_channel=2)
    full, out = play(D, x, 16384, 0, flights=dict(FL, max_flights=1024))
    msgs = [m for part in out for m in part]
    walk, evs = model_of(msgs, NOFILT, 600)
    aircraft = len(walk.entries())
    assert aircraft > 40 and full.flights_dropped == 0 and len(full.flights()) == aircraft
    by_addr = {FM.entry_key(f)[0]: FM.flight_bytes(f) for f in walk.entries()}
    # 16 slots: 16 aircraft fit, every other one is dropped once per call it turns up in (here: one call)
    small, _ = play(D, x, 16384, 0, flights=dict(FL, max_flights=16))
    got = small.flights()
    assert len(got) == 16 and small.flights_dropped == aircraft - 16
    for f in got:                                                        # whoever fitted has its complete entry
        assert bytes(f) == by_addr[bytes(f.addr).ljust(8, b"\0")]
    assert len(small.drain_routes()) <= len(walk.routes)
    small.close()
    # reset
    assert len(full.flights()) == aircraft
    full.reset()
    assert full.flights() == [] and full.drain_routes() == [] and full.flights_dropped == 0
    full.demod_msk(x)
    full.drain_msgs(max_msgs=65536)
    assert [bytes(f) for f in full.flights()] == [FM.flight_bytes(f) for f in walk.entries()]
    assert [bytes(r) for r in full.drain_routes()] == [FM.route_bytes(r) for r in walk.routes]
    # disable, enable: empty again, and the next messages build it anew
    full.disable_flights()
    n = C.c_int(0)
    assert full.L.acg_flight_snapshot(full.ctx, None, 0, C.byref(n), None) == K.ESTATE
    full.enable_flights(**FL)
    assert full.flights() == [] and full.drain_routes() == []
    # snapshot into a buffer that is too small: the number needed, nothing consumed
    full.reset()
    full.demod_msk(x)
    full.drain_msgs(max_msgs=65536)
    buf = (K.Flight * 3)()
    assert full.L.acg_flight_snapshot(full.ctx, buf, 3, C.byref(n), None) == K.EAGAIN and n.value == aircraft
    assert len(full.flights()) == aircraft
    full.close()
    plain = D.Decoder(4, decim=8, ntaps=8, max_blocks=1, repair=False, bitlog=False)
    cfg = K.FlightConfig(T0[0], T0[1], 600, 64)
    assert plain.L.acg_flights_enable(plain.ctx, C.byref(cfg)) == K.ESTATE
    for bad in (K.FlightConfig(0, 0, 0, 64), K.FlightConfig(0, 0, 600, 0)):
        assert plain.L.acg_flights_enable(plain.ctx, C.byref(bad)) == K.EINVAL
    plain.close()


# ---- the fixture: the reference program's own monitor frames and route lines -------------------------------------------------
def test_fixture_end_to_end_equals_the_reference_monitor_and_routes(D):
    """The 3-channel flight fixture through demodulator, framing, repair, split and flight pass in calls of 4096 samples (the
    reference reads its file in such chunks, and at most one block completes in any of them: both orders are the same
    order).  Per filter variant: flights() after each call that delivers a message equals the reference's monitor frame for
    that message, row by row, and drain_routes() equals the reference's route lines.  Nothing is skipped: every monitor
    frame of the fixture is compared."""
    pcm = np.load(os.path.join(GOLDEN, "flights_pcm16.npz"))["pcm"]
    with open(os.path.join(GOLDEN, "flights_golden.json")) as f:
        g = json.load(f)
    nch, chunk = 3, 4096
    assert pcm.shape[0] == nch
    x = pcm.astype(np.float32) / 32768.0
    x = np.concatenate([x, np.zeros((nch, (-x.shape[1]) % chunk), dtype=np.float32)], axis=1)
    for v, gv in g["variants"].items():
        kw = filter_kw(gv["args"], g["label_list"])
        dec = D.Decoder(nch, decim=8, ntaps=8, max_blocks=chunk // 1024, repair=True, bitlog=False)
        dec.set_msg_filter(**kw)
        dec.enable_flights(t0=T0, mdly=600, max_flights=64)
        frames, k = gv["frames"], 0
        for s in range(0, x.shape[1], chunk):
            dec.demod_msk(x[:, s:s + chunk])
            msgs = dec.drain_msgs()
            assert len(msgs) <= 1, (v, s)
            if msgs:
                fl = dec.flights()
                rows = D.monitor_rows(fl, nch)
                assert [parse_row(r, nch) for r in rows] == [g["rows"][i] for i in frames[k]], (v, k)
                k += 1
        assert k == len(frames) and k > 0, (v, k, len(frames))
        routes = [D.route_json(r) for r in dec.drain_routes()]
        assert [dict(flight=r["flight"], depa=r["depa"], dsta=r["dsta"]) for r in routes] == gv["routes"], v
        dec.close()


def parse_row(row, nbch):
    """monitor_rows()'s fixed columns back into (addr, fid, nbm, mask, DEP, ARR, ETA)"""
    return [row[1:9].strip(), row[10:17].strip(), int(row[18:21]), row[22:22 + nbch], row[40:44].strip(), row[46:50].strip(), row[52:56].strip()]
