"""Sharded hosts (acg_set_channel_numbers, acg_sink_keys, shard.merge_keyed): with a context-wide channel map the number handed out
appears wherever a channel is printed or ordered by, the slot stays the index of every per-slot table, and N contexts behind one
host give -- merged by the sinks' keys -- byte for byte what ONE context over all channels gives, in its order: frames, messages,
JSON lines, text records.  Fixtures and loaders are those of the JSON, text and flight-shard tests.  GPU box only."""
import ctypes as C
import re

import numpy as np
import pytest

import json_model as JM
import text_model as TM
import test_gpu_flight_shard as FS
import test_gpu_json_sink as JS
import test_gpu_text_sink as TS
from test_gpu_flights import LABELS_B, synthetic_traffic
from test_gpu_flights import T0 as FL_T0
from test_gpu_json_sink import D, fix                      # noqa: F401  (fixtures: imported, not copied)
from test_gpu_text_sink import fix as tfix                 # noqa: F401

pytestmark = pytest.mark.gpu

T0, CHUNK, VARIANTS = JS.T0, JS.CHUNK, JS.VARIANTS
FR = [131725000, 131525000, 129125000]                     # three distinct "freq" / "F:" tokens
TEXT_FULL = ((TM.ONELINE, TM.F_DATE), (TM.STD, TM.F_DATE | TM.F_FREQ), (TM.PP, 0), (TM.SV, 0))
OOOI_FIELDS = ("da", "sa", "eta", "gout", "gin", "woff", "won")
END_BITS = 44


def key_of(chn, end_bit):
    return (int(chn) << END_BITS) | int(end_bit)


def key_chn(k):
    return int(k) >> END_BITS


def key_end(k):
    return int(k) & ((1 << END_BITS) - 1)


def oo(o):
    return o.decoded not in (b"\x00", 0), {f: getattr(o, f) for f in OOOI_FIELDS}


def json_decoder(D, nch=3, numbers=None, station="STN1", app=("acarsdec", "3.7"), freqs=None, kw=None, chunk=CHUNK):
    dec = D.Decoder(nch, decim=8, ntaps=8, max_blocks=chunk // 1024, repair=True, bitlog=False) if chunk != CHUNK else JS.new_decoder(D, nch=nch, json_on=False)
    dec.enable_json(T0, station, app[0], app[1], freqs_hz=freqs)
    if kw:
        dec.set_msg_filter(**kw)
    if numbers is not None:
        dec.set_channel_numbers(numbers)
    return dec


def text_decoder(D, fmt, flags, nch=3, numbers=None, station="STN1", freqs=None, kw=None, chunk=CHUNK):
    dec = D.Decoder(nch, decim=8, ntaps=8, max_blocks=chunk // 1024, repair=True, bitlog=False) if chunk != CHUNK else TS.new_decoder(D, nch=nch)
    TS.enable(dec, fmt, flags, station=station, freqs_hz=freqs)
    if kw:
        dec.set_msg_filter(**kw)
    if numbers is not None:
        dec.set_channel_numbers(numbers)
    return dec


def plain_decoder(D, nch=3, numbers=None, kw=None):
    dec = JS.new_decoder(D, nch=nch, json_on=False)
    if kw:
        dec.set_msg_filter(**kw)
    if numbers is not None:
        dec.set_channel_numbers(numbers)
    return dec


@pytest.fixture(scope="module")
def base_calls(D, fix):
    """the fixture's (K.Msg, K.Oooi) per call of 4096 samples, from a decoder without a map and without a sink: computed once"""
    x, g, _ = fix
    dec = plain_decoder(D)
    calls = JS.play(dec, x, lambda: dec.drain_msgs(oooi=True))
    dec.close()
    assert sum(len(c) for c in calls) == len(g["sent"]) and {m.chn for c in calls for m, _ in c} == {0, 1, 2}
    return calls


def renumbered(group, numbers):
    """a call's base records in the order a context with the map `numbers` hands them out"""
    return sorted(group, key=lambda mo: (numbers[mo[0].chn], mo[0].end_bit))


def model_json(group, numbers, station, app, fr=None):
    return [JM.line(m, numbers[m.chn], JS.ts_token(m), station=station, freq=JM.freq_token(fr[m.chn]) if fr else b"0.000", app=app, oooi=oo(o))
            for m, o in renumbered(group, numbers)]


def model_text(group, numbers, fmt, flags, station, fr):
    return [TM.record(m, numbers[m.chn], fmt, flags, t0=T0, station=station, fr_hz=fr[m.chn], oooi=oo(o)) for m, o in renumbered(group, numbers)]


def sv_number(rec, station):
    """the channel token of an SV record: behind the padded station"""
    return int(re.match(rb" (\d+) ", rec[len(TM.pad(station, 8)):]).group(1)) - 1


def check_mapped_fixture(D, fix, base_calls, numbers):
    """the fixture in ONE context under `numbers`: JSON buffers and the four text formats' records equal the models run on the base
    messages with chn replaced and re-sorted; every record names the number handed out and the frequency of its SLOT; the order of
    every call is the numbers'; the keys carry them"""
    x, g, app = fix
    appb, station = tuple(a.encode() for a in app), g["station"].encode()
    slot_of = {n: s for s, n in enumerate(numbers)}
    dec = json_decoder(D, numbers=numbers, station=g["station"], app=app, freqs=FR)
    got = JS.play(dec, x, lambda: (dec.drain_json(), dec.sink_keys("json")))
    dec.close()
    seen = []
    for (blob, keys), group in zip(got, base_calls):
        want = model_json(group, numbers, station, appb, FR)
        assert blob == b"".join(want)
        lines = JS.split_lines(blob)
        chans = [JS.chn_of(ln) for ln in lines]
        assert chans == sorted(chans) and [key_chn(k) for k in keys] == chans
        assert [key_end(k) for k in keys] == [m.end_bit for m, _ in renumbered(group, numbers)]
        for ln, c in zip(lines, chans):
            assert b',"channel":%d,"freq":%s,' % (c, JM.freq_token(FR[slot_of[c]])) in ln
        seen += chans
    assert set(seen) == set(numbers)
    for fmt, flags in TEXT_FULL:
        dec = text_decoder(D, fmt, flags, numbers=numbers, station="STATION-9", freqs=FR)
        got = TS.play(dec, x, lambda: (dec.drain_text(), dec.sink_keys("text")))
        dec.close()
        for (recs, keys), group in zip(got, base_calls):
            assert recs == model_text(group, numbers, fmt, flags, b"STATION-9", FR), (fmt, flags)
            order = [numbers[m.chn] for m, _ in renumbered(group, numbers)]
            assert [key_chn(k) for k in keys] == order == sorted(order)
            if fmt in (TM.ONELINE, TM.STD):
                assert [TM.chn_of(r) for r in recs] == order                      # the token is the number + 1
            if fmt == TM.STD:
                for r, c in zip(recs, order):
                    assert r.startswith(b"\n[#%d (" % (c + 1) + TM.freq_token(FR[slot_of[c]]) + b"L:")
            if fmt == TM.SV:
                assert [sv_number(r, b"STATION-9") for r in recs] == order


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
def test_a_permutation_catches_a_lookup_by_the_wrong_index(D, fix, base_calls):
    """[2, 0, 1] over three slots with three distinct frequencies: indexing the frequency table by the number handed out, or the
    map by anything but the slot, yields a wrong but valid token here"""
    check_mapped_fixture(D, fix, base_calls, [2, 0, 1])


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
def test_the_whole_range_of_numbers(D, fix, base_calls):
    """[1048575, 0, 77]: the 7-digit number and its chn + 1 = 1048576 render, the key's 20-bit field is exact, the order is 0, 77,
    1048575; frames, messages and the _oooi records carry the numbers"""
    from acarsdec_amd import _capi as K
    x, g, app = fix
    numbers = [1048575, 0, 77]
    check_mapped_fixture(D, fix, base_calls, numbers)
    dec = json_decoder(D, numbers=numbers)
    lines = JS.split_lines(b"".join(JS.play(dec, x, dec.drain_json)))
    dec.close()
    assert any(b',"channel":1048575,' in ln for ln in lines)
    dec = text_decoder(D, TM.ONELINE, 0, numbers=numbers)
    recs = sum(TS.play(dec, x, dec.drain_text), [])
    dec.close()
    assert any(r.startswith(b"#1048576 (L:") for r in recs) and any(r.startswith(b"#78 (L:") for r in recs)
    # messages with their labels, messages without, frames
    with_oooi, plain, framed, unmapped = plain_decoder(D, numbers=numbers), plain_decoder(D, numbers=numbers), plain_decoder(D, numbers=numbers), plain_decoder(D)
    for s, group in zip(range(0, x.shape[1], CHUNK), base_calls):
        for d in (with_oooi, plain, framed, unmapped):
            d.demod_msk(x[:, s:s + CHUNK])
        want = []
        for m, o in renumbered(group, numbers):
            mm = K.Msg.from_buffer_copy(bytes(m))
            mm.chn = numbers[m.chn]
            want.append(bytes(mm) + bytes(o))
        got = with_oooi.drain_msgs(oooi=True)
        assert [bytes(m) + bytes(o) for m, o in got] == want
        assert [bytes(m) for m in plain.drain_msgs()] == [w[:C.sizeof(K.Msg)] for w in want]
        assert [m.chn for m, _ in got] == sorted(m.chn for m, _ in got)
        fw = []
        for f in unmapped.drain_frames():
            ff = K.Frame.from_buffer_copy(bytes(f))
            ff.chn = numbers[f.chn]
            fw.append(ff)
        fw.sort(key=lambda f: (f.chn, f.end_bit))
        assert [bytes(f) for f in framed.drain_frames()] == [bytes(f) for f in fw]
    for d in (with_oooi, plain, framed, unmapped):
        d.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def shards_of(nch, world):
    from acarsdec_amd import shard
    own = [shard.owned_channels(nch, r, world) for r in range(world)]
    return own, [shard.channel_numbers(len(o), r, world) for r, o in enumerate(own)]


class Host:
    """one output kind by `world` contexts (`c mod world`); world == 1: the single context over all channels, no map.  fetch(dec)
    returns (keys, records) of one call"""

    def __init__(self, make, fetch, nch, world):
        self.own, numbers = shards_of(nch, world)
        assert world == 1 or sorted(int(n) for m in numbers for n in m) == list(range(nch))
        self.decs = [make(len(o), None if world == 1 else m, o) for o, m in zip(self.own, numbers)]
        self.fetch = fetch

    def round(self, xs):
        from acarsdec_amd import shard
        for d, o in zip(self.decs, self.own):
            d.demod_msk(xs[o])
        parts = [self.fetch(d) for d in self.decs]
        for keys, recs in parts:
            assert len(keys) == len(recs) and all(int(a) < int(b) for a, b in zip(keys, keys[1:]))
        return shard.merge_keyed(parts)

    def close(self):
        for d in self.decs:
            d.close()


def fetch_json(d):
    blob = d.drain_json()
    return d.sink_keys("json"), JS.split_lines(blob)


def fetch_text(d):
    recs = d.drain_text()
    return d.sink_keys("text"), recs


def fetch_msgs(d):
    got = d.drain_msgs(oooi=True)
    return [key_of(m.chn, m.end_bit) for m, _ in got], [bytes(m) + bytes(o) for m, o in got]


def fetch_frames(d):
    got = d.drain_frames()
    return [key_of(f.chn, f.end_bit) for f in got], [bytes(f) for f in got]


@pytest.mark.parametrize("v", VARIANTS)
def test_sharded_equals_single_equals_reference(D, fix, tfix, v):
    """The fixture by three 1-channel contexts and by two (slots {0, 2} and {1}), calls of 4096 samples: after EVERY round the merge
    of the contexts' (sink_keys, records) is the single context's output of that round -- JSON, -o 1, -o 2, the two datagrams,
    messages with their labels, frames.  Over the run the merged JSON, -o 1 and -o 2 are the reference program's stdout (per channel;
    the time stamp's number cut out of the JSON lines, as in the sinks' own tests)."""
    x, g, app = fix
    gt = tfix[2]
    kw = JS.filter_kw(g, v)
    kinds = {"json": (lambda n, m, o: json_decoder(D, nch=n, numbers=m, station=g["station"], app=app, kw=kw), fetch_json)}
    for name, fmt in (("o1", TM.ONELINE), ("o2", TM.STD), ("pp", TM.PP), ("sv", TM.SV)):
        kinds[name] = (lambda n, m, o, fmt=fmt: text_decoder(D, fmt, 0, nch=n, numbers=m, kw=kw), fetch_text)
    kinds["msgs"] = (lambda n, m, o: plain_decoder(D, nch=n, numbers=m, kw=kw), fetch_msgs)
    if v == "none":                                              # (the frame entry points sit in front of the filters)
        kinds["frames"] = (lambda n, m, o: plain_decoder(D, nch=n, numbers=m), fetch_frames)
    for name, (make, fetch) in kinds.items():
        hosts = [Host(make, fetch, 3, world) for world in (1, 3, 2)]
        run = []
        for s in range(0, x.shape[1], CHUNK):
            single, three, two = [h.round(x[:, s:s + CHUNK]) for h in hosts]
            assert three == single and two == single, (v, name, s)
            run += three
        for h in hosts:
            h.close()
        if name == "json":
            ref = [ln.encode("ascii") + b"\n" for ln in g["variants"][v]["lines"]]
            assert len(run) == len(ref) > 0
            for c in range(3):
                assert [JM.cut_timestamp(ln)[0] for ln in run if JS.chn_of(ln) == c] == [JM.cut_timestamp(ln)[0] for ln in ref if JS.chn_of(ln) == c], (v, c)
        elif name in ("o1", "o2"):
            ref = (TM.split_oneline if name == "o1" else TM.split_std)(bytes.fromhex(gt["variants"][v][name]))
            assert len(run) == len(ref) == gt["variants"][v]["records"] > 0
            for c in range(3):
                assert [r for r in run if TM.chn_of(r) == c] == [r for r in ref if TM.chn_of(r) == c], (v, name, c)
        else:
            assert len(run) > 0, (v, name)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
def test_sixty_four_channels_by_four_contexts(D):
    """64 channels of synthetic traffic, eight calls of 16 384 samples, four contexts of 16 slots against one of 64: JSON lines and
    -o 2 records with date and the slot's "F:" token, merged per round, are the single context's"""
    nch, chunk, world = 64, 16384, 4
    x = synthetic_traffic(nch, 8 * chunk, 40, 15, per_channel=8)
    fr = np.array([118000000 + 25000 * c for c in range(nch)], dtype=np.int32)
    kinds = ((lambda n, m, o: json_decoder(D, nch=n, numbers=m, freqs=fr[o], chunk=chunk), fetch_json),
             (lambda n, m, o: text_decoder(D, TM.STD, TM.F_DATE | TM.F_FREQ, nch=n, numbers=m, freqs=fr[o], chunk=chunk), fetch_text))
    for make, fetch in kinds:
        one, four = Host(make, fetch, nch, 1), Host(make, fetch, nch, world)
        total, heard = 0, set()
        for s in range(0, x.shape[1], chunk):
            want = one.round(x[:, s:s + chunk])
            assert four.round(x[:, s:s + chunk]) == want, s
            total += len(want)
            heard |= {JS.chn_of(r) if fetch is fetch_json else TM.chn_of(r) for r in want}
        one.close()
        four.close()
        print("records", total, "channels heard", len(heard))
        assert total >= 300 and len(heard) > 48, (total, len(heard))       # an empty run cannot pass


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
def raw_keys(dec, sink, cap):
    buf = np.zeros(max(cap, 1), dtype=np.uint64)
    n = C.c_int(-1)
    rc = dec.L.acg_sink_keys(dec.ctx, sink, buf.ctypes.data if cap else None, cap, C.byref(n))
    return rc, n.value, buf[:max(min(n.value, cap), 0)].copy()


def test_sink_keys(D, fix):
    from acarsdec_amd import _capi as K
    x, g, app = fix
    numbers = [5, 1048575, 3]
    ncall = 6
    dec, plain = json_decoder(D, numbers=numbers, app=app), plain_decoder(D, numbers=numbers)
    assert raw_keys(dec, K.SINK_JSON, 8)[:2] == (K.OK, 0)                         # before any sink call
    assert raw_keys(dec, K.SINK_TEXT, 8)[:2] == (K.ESTATE, 0)                     # that sink is off
    assert raw_keys(dec, 3, 8)[0] == K.EINVAL and raw_keys(dec, 0, 8)[0] == K.EINVAL
    assert dec.max_lag + 1 >= ncall
    for d in (dec, plain):
        JS.play(d, x[:, :ncall * CHUNK])
    msgs = plain.drain_msgs()
    by_key = {key_of(m.chn, m.end_bit): m for m in msgs}
    assert len(by_key) == len(msgs) > 10
    got, codes = [], []
    for _ in range(len(msgs) + 2):
        rc, blob, nl = JS.raw_drain(dec, K, 5 * K.JSON_LINE_MAX)                  # five lines a call: ACG_EAGAIN until the last
        codes.append(rc)
        lines = JS.split_lines(blob)
        krc, n, keys = raw_keys(dec, K.SINK_JSON, 5)
        assert krc == K.OK and n == nl == len(lines) == len(keys)                 # the keys of the records handed out, also behind ACG_EAGAIN
        assert all(int(a) < int(b) for a, b in zip(keys, keys[1:]))
        for k, ln in zip(keys, lines):
            m = by_key[int(k)]                                                   # channel field and end_bit name the line's message
            assert key_chn(k) == JS.chn_of(ln) == m.chn and key_end(k) == m.end_bit
            assert ln == JM.line(m, m.chn, JS.ts_token(m), station=b"STN1", app=tuple(a.encode() for a in app))
        if n > 1:                                                                # too small a buffer: the count, nothing consumed
            assert raw_keys(dec, K.SINK_JSON, n - 1)[:2] == (K.EAGAIN, n) and raw_keys(dec, K.SINK_JSON, 0)[:2] == (K.EAGAIN, n)
            again = raw_keys(dec, K.SINK_JSON, n)
            assert again[:2] == (K.OK, n) and again[2].tolist() == keys.tolist()
        got += [int(k) for k in keys]
        if rc == K.OK:
            break
    assert codes[-1] == K.OK and codes.count(K.EAGAIN) == len(codes) - 1 >= 2
    assert sorted(got) == sorted(by_key) and 1048575 in {key_chn(k) for k in got}
    assert JS.raw_drain(dec, K, 5 * K.JSON_LINE_MAX) == (K.OK, b"", 0)
    assert raw_keys(dec, K.SINK_JSON, 8)[:2] == (K.OK, 0)                         # a call that handed out nothing
    # the wrapper that loops over ACG_EAGAIN keeps the keys of all its C calls
    dec.reset()
    JS.play(dec, x[:, :ncall * CHUNK])
    lines = JS.split_lines(dec.drain_json(max_lines=5))
    keys = dec.sink_keys("json")
    assert len(keys) == len(lines) > 5 and [key_chn(k) for k in keys] == [JS.chn_of(ln) for ln in lines]
    dec.close()
    plain.close()
    # the text sink's keys are its own
    tdec = text_decoder(D, TM.ONELINE, 0, numbers=numbers)
    assert raw_keys(tdec, K.SINK_TEXT, 8)[:2] == (K.OK, 0) and raw_keys(tdec, K.SINK_JSON, 8)[:2] == (K.ESTATE, 0)
    JS.play(tdec, x[:, :ncall * CHUNK])
    recs = tdec.drain_text()
    rc, n, keys = raw_keys(tdec, K.SINK_TEXT, len(recs))
    assert rc == K.OK and n == len(recs) == len(msgs) and [key_chn(k) for k in keys] == [TM.chn_of(r) for r in recs]
    assert keys.tolist() == sorted(by_key)
    tdec.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
def renumber_lines(blob, numbers):
    """a map-less context's JSON buffer as a context under `numbers` hands it out (no frequencies set: nothing else differs)"""
    lines = [re.sub(rb',"channel":(\d+),', lambda m: b',"channel":%d,' % numbers[int(m.group(1))], ln, count=1) for ln in JS.split_lines(blob)]
    return b"".join(sorted(lines, key=JS.chn_of))                                # (stable: per channel the order stays)


def test_map_states(D, fix):
    from acarsdec_amd import _capi as K
    x, g, app = fix
    numbers = [2, 0, 1]
    span = 5 * CHUNK                                                             # a phase: five calls queued, one drain
    feed = lambda d, k: JS.play(d, x[:, k * span:(k + 1) * span])
    fresh = json_decoder(D, app=app)
    base = []
    for k in range(3):
        feed(fresh, k)
        base.append(fresh.drain_json())
    fresh.close()
    assert all(len({JS.chn_of(ln) for ln in JS.split_lines(b)}) == 3 for b in base)          # every phase hears every channel
    dec = json_decoder(D, app=app)
    feed(dec, 0)                                                                 # queued under no map ...
    dec.set_channel_numbers(numbers)                                             # ... handed out under this one
    assert dec.drain_json() == renumber_lines(base[0], numbers) != base[0]
    for bad in ([-1, 0, 1], [1 << 20, 0, 1], [1, 0, 1]):                         # refused: the map in force stays in force
        arr = np.array(bad, dtype=np.int32)
        assert dec.L.acg_set_channel_numbers(dec.ctx, arr.ctypes.data) == K.EINVAL
    feed(dec, 1)
    assert dec.drain_json() == renumber_lines(base[1], numbers)
    dec.set_channel_numbers(None)                                                # the identity again: today's bytes
    feed(dec, 2)
    assert dec.drain_json() == base[2]
    dec.set_channel_numbers(numbers)
    dec.reset()                                                                  # acg_reset keeps the map
    feed(dec, 0)
    assert dec.drain_json() == renumber_lines(base[0], numbers)
    with pytest.raises(ValueError):
        dec.set_channel_numbers([0, 1])                                          # one number per slot
    dec.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
def test_flight_table_follows_the_context_map(D):
    """8 channels of synthetic traffic: the context's map alone gives the table acg_flights_set_channels gives with the same array;
    with both set the table follows the flight map and the sink the context's; the per-slot statistics do not move"""
    nch, chunk = 8, 16384
    x = synthetic_traffic(nch, 3 * chunk, 4, 15, per_channel=4)
    kw = dict(downlink_only=True, skip_empty=False, labels=LABELS_B)
    fl = dict(t0=FL_T0, mdly=600, max_flights=64)
    odd, other = np.arange(nch) * 2 + 1, np.arange(nch) * 3 + 2
    make = lambda: FS.make_decoder(D, nch, chunk, kw, fl, (16, b"ST1"))
    by_ctx, by_table, both, other_only, bare = make(), make(), make(), make(), make()
    by_ctx.set_channel_numbers(odd)
    by_table.set_flight_channels(odd)
    both.set_channel_numbers(odd)
    both.set_flight_channels(other)
    other_only.set_flight_channels(other)
    both.enable_json(T0, "ST1", "acarsdec", "3.7")
    for d in (by_ctx, bare):
        d.enable_stats()
    lines, routes = [], 0
    for s in range(0, x.shape[1], chunk):
        for d in (by_ctx, by_table, both, other_only, bare):
            d.demod_msk(x[:, s:s + chunk])
        mc, mt = by_ctx.drain_msgs(), by_table.drain_msgs()
        assert [m.chn for m in mc] == [int(odd[m.chn]) for m in mt]               # (the flight map leaves the messages' numbers alone)
        lines += JS.split_lines(both.drain_json())
        other_only.drain_msgs()
        bare.drain_msgs()
        for a, b in ((by_ctx, by_table), (both, other_only)):
            assert [bytes(f) for f in a.flights()] == [bytes(f) for f in b.flights()], s
            assert a.monitor_text(-1) == b.monitor_text(-1), s
            ra, rb = a.drain_routes_json(), b.drain_routes_json()
            assert ra == rb, s
            routes += a.route_lines_n
    table, table2 = by_ctx.flights(), both.flights()
    assert table and all(f.first_chn % 2 == 1 and f.last_chn % 2 == 1 and f.chm & 0x5555555555555555 == 0 for f in table)
    assert table2 and all(f.first_chn % 3 == 2 for f in table2)                  # the table: the flight map ...
    assert lines and {JS.chn_of(ln) for ln in lines} <= set(odd.tolist())       # ... the sink: the context's
    print("entries", len(table), len(table2), "route lines", routes, "JSON lines", len(lines))
    sa, sb = by_ctx.stats(), bare.stats()
    assert sa[0].tobytes() == sb[0].tobytes() and sa[1] == sb[1] and int(sa[0]["delivered"].sum()) > 0
    for d in (by_ctx, by_table, both, other_only, bare):
        d.close()
