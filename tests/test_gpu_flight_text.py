"""The flight table's text on the device (flight_text.hip): the monitor screen and the route lines against the Python model
(tests/monitor_model.py), byte for byte and whole buffers, and -- masked where the reference stamps its wall clock -- against the
bytes the reference program printed (tests/golden/monitor_golden.json); designed records no traffic produces through
acg_selftest_flight_text; the contract of the entry points; and that nothing else changes.  GPU box only."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
import monitor_model as MM

pytestmark = pytest.mark.gpu

T0 = MM.T0
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def D():
    from acarsdec_amd import decoder
    from acarsdec_amd import _capi as K
    assert K.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return decoder


@pytest.fixture(scope="module")
def fix():
    pcm = np.load(os.path.join(GOLDEN, "flights_pcm16.npz"))["pcm"]
    with open(os.path.join(GOLDEN, "flights_golden.json")) as f:
        fg = json.load(f)
    with open(os.path.join(GOLDEN, "monitor_golden.json")) as f:
        mg = json.load(f)
    chunk = 4096
    x = pcm.astype(np.float32) / 32768.0
    x = np.concatenate([x, np.zeros((x.shape[0], (-x.shape[1]) % chunk), dtype=np.float32)], axis=1)
    return x, fg, mg


def filter_kw(args, label_list):
    return dict(downlink_only="-A" in args, skip_empty="-e" in args, labels=label_list if "-b" in args else None)


def model_frame(dec, nbch, soh_sample):
    entries = [MM.entry_of(f) for f in dec.flights()]
    return MM.frame(entries, nbch, MM.header_tv(entries, T0, soh_sample)), entries


# ---- the fixture: the reference program's own bytes ---------------------------------------------------------------------------
@pytest.mark.parametrize("v", ["none", "A", "e", "b", "Aeb"])
def test_fixture_end_to_end_equals_model_and_reference(D, fix, v):
    """3 channels in calls of 4096 samples (at most one block completes in any of them).  After every call that delivers a
    message, monitor_text(that message's soh_sample) equals the model's frame of flights() at that moment, whole buffer, and,
    masked, the reference's frame k; every frame is compared and counted.  At the end drain_routes_json() equals the model's
    lines of the records a second decoder's acg_drain_routes hands out and, masked, the reference's lines ("none": with the
    station that needs an escape)."""
    x, fg, mg = fix
    nch, chunk, gv = mg["nch"], 4096, mg["variants"][v]
    station = mg["station"].encode("latin1") if v == "none" else b""
    want_routes = mg["station_routes"] if v == "none" else gv["routes"]
    head = MM.CLS + mg["header"].encode("latin1")
    ref = [head + b"".join(mg["rows"][i].encode("latin1") + b"\n" for i in ids) for ids in gv["frames"]]
    decs = []
    for text in (True, False):
        dec = D.Decoder(nch, decim=8, ntaps=8, max_blocks=chunk // 1024, repair=True, bitlog=False)
        dec.set_msg_filter(**filter_kw(gv["args"], fg["label_list"]))
        dec.enable_flights(t0=T0, mdly=600, max_flights=64)
        if text:
            dec.enable_flight_text(nch, station)
        decs.append(dec)
    a, b = decs
    k = 0
    for s in range(0, x.shape[1], chunk):
        a.demod_msk(x[:, s:s + chunk])
        b.demod_msk(x[:, s:s + chunk])
        msgs = a.drain_msgs()
        assert [bytes(m) for m in b.drain_msgs()] == [bytes(m) for m in msgs] and len(msgs) <= 1, (v, s)
        if msgs:
            got = a.monitor_text(msgs[0].soh_sample)
            want, entries = model_frame(a, nch, msgs[0].soh_sample)
            assert got == want, (v, k, got, want)
            assert a.monitor_rows_n == len(entries)
            assert MM.mask_times(got) == ref[k], (v, k)
            k += 1
    assert k == len(ref) == len(fg["variants"][v]["frames"]) and k > 0, (v, k, len(ref))
    lines = a.drain_routes_json()
    records = b.drain_routes()
    assert lines == b"".join(MM.route_line(MM.route_of(r), station) for r in records), v
    assert a.route_lines_n == len(records) == len(want_routes)
    assert [MM.mask_route(ln + b"\n") for ln in lines.split(b"\n")[:-1]] == [r.encode("latin1") for r in want_routes], v
    assert a.drain_routes_json() == b"" and a.route_lines_n == 0                     # the queue was emptied
    a.close()
    b.close()


# ---- designed records -------------------------------------------------------------------------------------------------------------
def flight_records(K, entries):
    out = (K.Flight * max(1, len(entries)))()
    for o, f in zip(out, entries):
        o.addr, o.fid, o.rt, o.nbm, o.first_chn, o.last_chn, o.chm = f["addr"], f["fid"], f["rt"], f["nbm"], f["first_chn"], f["last_chn"], f["chm"]
        o.ts_sample, o.tl_sample, (o.ts_sec, o.ts_usec), (o.tl_sec, o.tl_usec) = f["ts_sample"], f["tl_sample"], f["ts"], f["tl"]
        o.da, o.sa, o.eta, o.gout, o.gin, o.woff, o.won = f["fields"]
    return out


def route_records(K, routes):
    out = (K.Route * max(1, len(routes)))()
    for o, r in zip(out, routes):
        o.soh_sample, o.sec, o.usec, o.chn, o.fid, o.sa, o.da, o.addr = r["soh_sample"], r["sec"], r["usec"], r["chn"], r["fid"], r["sa"], r["da"], r["addr"]
    return out


def selftest(K, case, mon_cap, rts_cap):
    mon, rts = (C.c_ubyte * (mon_cap + 64))(), (C.c_ubyte * (rts_cap + 64))()
    C.memset(mon, SENTINEL, len(mon))
    C.memset(rts, SENTINEL, len(rts))
    nbm, nbr, nrows, nlines = C.c_size_t(0), C.c_size_t(0), C.c_int(-1), C.c_int(-1)
    fcfg, tcfg = K.FlightConfig(case["t0"][0], case["t0"][1], 600, 16), K.FlightTextConfig(case["nbch"], case["station"])
    rc = K.load().acg_selftest_flight_text(flight_records(K, case["entries"]), len(case["entries"]), route_records(K, case["routes"]), len(case["routes"]),
                                           C.byref(fcfg), C.byref(tcfg), case["hdr_soh"], mon, mon_cap, C.byref(nbm), C.byref(nrows),
                                           rts, rts_cap, C.byref(nbr), C.byref(nlines))
    return rc, bytes(mon), nbm.value, nrows.value, bytes(rts), nbr.value, nlines.value


@pytest.mark.parametrize("j", range(len(MM.ROW_COUNTS)))
def test_designed_records_equal_the_model(D, j):
    """acg_selftest_flight_text on records no traffic produces (tests/monitor_model.py designed_cases: row counts 0 .. 1025 across
    the scan's workgroups, nbm of 1 .. 10 digits, empty and short fields, a 7-character addr, every nbch, masks all set / none /
    only bits >= 16, the time values of the CPU test, header times past 2^31, 2^32 and 2^40 samples, routes in shuffled tag
    order with quotes, backslashes, control bytes and bytes >= 0x80, a station of 32 control characters): whole buffers against
    the model, the sentinel bytes behind *nbytes untouched; and one byte short is ACG_EAGAIN with both buffers untouched."""
    from acarsdec_amd import _capi as K
    case = MM.designed_cases()[j]
    want_mon = MM.frame(case["entries"], case["nbch"], MM.header_tv(case["entries"], case["t0"], case["hdr_soh"]))
    want_rts = b"".join(MM.route_line(r, case["station"]) for r in case["routes"])
    assert len(want_mon) <= MM.HDR_LEN + len(case["entries"]) * MM.ROW_MAX and len(want_rts) <= len(case["routes"]) * MM.LINE_MAX
    rc, mon, nbm, nrows, rts, nbr, nlines = selftest(K, case, len(want_mon), len(want_rts))
    assert rc == K.OK, rc
    assert (nbm, nrows, nbr, nlines) == (len(want_mon), len(case["entries"]), len(want_rts), len(case["routes"]))
    assert mon[:nbm] == want_mon, next(i for i in range(nbm) if mon[i] != want_mon[i])
    assert rts[:nbr] == want_rts, next(i for i in range(nbr) if rts[i] != want_rts[i])
    assert mon[nbm:] == bytes([SENTINEL]) * 64 and rts[nbr:] == bytes([SENTINEL]) * 64
    rc, mon, nbm, nrows, rts, nbr, nlines = selftest(K, case, len(want_mon) - 1, max(0, len(want_rts) - 1))
    assert rc == K.EAGAIN and nbm == len(want_mon) and set(mon) == {SENTINEL}
    assert nbr == len(want_rts) and set(rts) == {SENTINEL}


# ---- errors and state -------------------------------------------------------------------------------------------------------------
def synthetic(nch, nsamp, naircraft, seed, per_channel=3):
    """[nch, nsamp] float32 audio: per channel a few downlinks from `naircraft` aircraft, most with departure and destination"""
    from acarsdec_amd import synth as S
    rng = np.random.default_rng(seed)
    x = np.zeros((nch, nsamp), dtype=np.float32)
    ap = [b"KJFK", b"EGLL", b"LFPG", b"EDDF", b"KBOS", b"LEMD"]
    for c in range(nch):
        pos = int(rng.integers(500, 3000))
        for _ in range(per_channel):
            pick = lambda: ap[int(rng.integers(0, len(ap)))]
            lab, body = ((b"QP", pick() + pick() + b"0815"), (b"QA", pick() + b"0815"), (b"H1", b"FREE TEXT"), (b"QN", b"XXXX" + pick() + b"0930"))[int(rng.integers(0, 4))]
            down = rng.random() < 0.9
            text = (b"M01A" + (b"XY%04d" % int(rng.integers(0, 40))) + body) if down else b"UPLINK"
            fr = S.acars_frame(text=text, addr=b".N%05d" % int(rng.integers(0, naircraft)), label=lab, bid=b"4" if down else b"B")
            a = S.msk_audio(S.frame_bits(fr), phase0=float(rng.uniform(0, 2 * np.pi)))
            if pos + a.size + 200 > nsamp:
                break
            x[c, pos:pos + a.size] = 0.06 * a
            pos += a.size + int(rng.integers(1500, 6000))
    return x


def decoder(D, nch, flights=True, text=None, chunk=16384):
    dec = D.Decoder(nch, decim=8, ntaps=8, max_blocks=chunk // 1024, repair=True, bitlog=False, max_lag=2)
    if flights:
        dec.enable_flights(t0=T0, mdly=600, max_flights=1024)
    if text is not None:
        dec.enable_flight_text(*text)
    return dec


def raw_call(fn, cap, *lead):
    """an all-or-nothing entry point on a sentinel-filled buffer of cap bytes (+ 64 of room behind): (rc, buffer, nbytes, n)"""
    buf = (C.c_ubyte * (cap + 64))()
    C.memset(buf, SENTINEL, len(buf))
    nb, n = C.c_size_t(0), C.c_int(-1)
    rc = fn(*lead, buf, cap, C.byref(nb), C.byref(n))
    return rc, bytes(buf), nb.value, n.value


def test_errors_and_state(D):
    from acarsdec_amd import _capi as K
    x = synthetic(64, 16384, 60, 31)
    dec, twin = decoder(D, 64, text=(16, b"st1")), decoder(D, 64)
    for d in (dec, twin):
        d.demod_msk(x)
        d.drain_msgs(max_msgs=65536)
    L, before = dec.L, [bytes(f) for f in dec.flights()]
    records = twin.drain_routes()
    want_mon = model_frame(dec, 16, -1)[0]
    want_rts = b"".join(MM.route_line(MM.route_of(r), b"st1") for r in records)
    assert len(before) > 30 and len(records) > 5
    # ---- one byte short: ACG_EAGAIN, the bytes needed, the buffer untouched, nothing consumed
    mon = lambda cap: raw_call(lambda ctx, buf, c, nb, n: L.acg_flight_monitor_text(ctx, -1, buf, c, nb, n, None), cap, dec.ctx)
    rts = lambda cap: raw_call(L.acg_drain_routes_json, cap, dec.ctx)
    rc, buf, nb, n = mon(len(want_mon) - 1)
    assert rc == K.EAGAIN and nb == len(want_mon) and set(buf) == {SENTINEL}
    rc, buf, nb, n = mon(len(want_mon))
    assert rc == K.OK and nb == len(want_mon) and n == len(before) and buf[:nb] == want_mon and set(buf[nb:]) == {SENTINEL}
    rc, buf, nb, n = rts(len(want_rts) - 1)
    assert rc == K.EAGAIN and nb == len(want_rts) and n == len(records) and set(buf) == {SENTINEL}
    rc, buf, nb, n = rts(len(want_rts))
    assert rc == K.OK and nb == len(want_rts) and n == len(records) and buf[:nb] == want_rts and set(buf[nb:]) == {SENTINEL}
    rc, buf, nb, n = rts(len(want_rts))
    assert rc == K.OK and (nb, n) == (0, 0)                                           # consumed by the call that had room
    # ---- monitor_text consumes nothing
    assert dec.monitor_text() == want_mon and [bytes(f) for f in dec.flights()] == before
    # ---- ACG_EINVAL: the configuration, with the table on
    unterminated = K.FlightTextConfig(3, b"")
    C.memset(C.byref(unterminated, K.FlightTextConfig.station_id.offset), ord("S"), 33)
    for bad in (K.FlightTextConfig(-1, b""), K.FlightTextConfig(17, b""), unterminated):
        assert L.acg_flight_text_enable(dec.ctx, C.byref(bad)) == K.EINVAL
    assert dec.monitor_text() == want_mon                                             # (a refused configuration leaves the renderer as it was)
    # ---- acg_reset keeps the configuration: an empty table prints the header with t0
    dec.reset()
    assert dec.monitor_text() == MM.header(T0) and dec.monitor_rows_n == 0 and dec.drain_routes_json() == b""
    # ---- ACG_ESTATE: routes left pending on the host by acg_drain_routes
    dec.demod_msk(x)
    dec.drain_msgs(max_msgs=65536)
    one, n1 = (K.Route * 1)(), C.c_int(0)
    assert L.acg_drain_routes(dec.ctx, one, 1, C.byref(n1)) == K.EAGAIN and n1.value == 1
    assert rts(len(want_rts))[0] == K.ESTATE
    assert len(dec.drain_routes()) == len(records) - 1                                # behind an ACG_OK the other entry point works again
    assert rts(len(want_rts))[0] == K.OK
    # ---- ACG_ESTATE: the renderer off, the table off (switching the table off or on again switches the renderer off)
    dec.disable_flight_text()
    assert mon(4096)[0] == K.ESTATE and rts(4096)[0] == K.ESTATE
    dec.enable_flight_text(16)
    assert dec.monitor_text()[:MM.CLS_LEN] == MM.CLS
    dec.enable_flights(t0=T0, mdly=600, max_flights=1024)
    assert mon(4096)[0] == K.ESTATE and rts(4096)[0] == K.ESTATE
    dec.disable_flights()
    assert mon(4096)[0] == K.ESTATE and rts(4096)[0] == K.ESTATE
    assert L.acg_flight_text_enable(dec.ctx, C.byref(K.FlightTextConfig(3, b""))) == K.ESTATE
    dec.close()
    twin.close()


def test_nothing_else_changes(D):
    """64 channels of synthetic traffic from about 300 aircraft through two decoders, one with the renderer enabled and called
    after every call: acg_collect_msgs records, acg_flight_snapshot and `dropped` are byte-identical after every call, and each
    frame of more than 64 rows equals the model's"""
    nch, chunk = 64, 4096
    x = synthetic(nch, 49152, 300, 32, per_channel=5)
    a, b = decoder(D, nch, text=(16, b""), chunk=chunk), decoder(D, nch, chunk=chunk)
    big = total = 0
    for s in range(0, x.shape[1], chunk):
        a.demod_msk(x[:, s:s + chunk])
        b.demod_msk(x[:, s:s + chunk])
        ma, mb = a.collect_msgs(lag=0, max_msgs=65536), b.collect_msgs(lag=0, max_msgs=65536)
        assert [bytes(m) for m in ma] == [bytes(m) for m in mb], s
        total += len(ma)
        frame = a.monitor_text()
        fa, fb = a.flights(), b.flights()
        assert [bytes(f) for f in fa] == [bytes(f) for f in fb] and a.flights_dropped == b.flights_dropped == 0, s
        if len(fa) > 64:
            entries = [MM.entry_of(f) for f in fa]
            assert frame == MM.frame(entries, 16, MM.header_tv(entries, T0, -1)) and a.monitor_rows_n == len(fa), s
            big += 1
    assert total > 200 and big >= 3 and len(fa) > 100, (total, big, len(fa))
    assert a.drain_routes_json() == b"".join(MM.route_line(MM.route_of(r)) for r in b.drain_routes())
    a.close()
    b.close()
