"""The JSON sink on the device (json.hip): what acg_drain_json / acg_collect_json hand out against the lines the unmodified
reference program printed for the JSON fixture, byte for byte; random records through the lab entry against the Python model
(tests/json_model.py), whole buffer byte for byte; the drain / collect contract; the existing message paths untouched; the
level's text against the host-computed record.  GPU box only."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN
import json_model as JM
import label_model as LM

pytestmark = pytest.mark.gpu

VARIANTS = ("none", "A", "e", "b", "Aeb")
T0 = (1792301725, 269667)
CHUNK = 4096


@pytest.fixture(scope="module")
def D():
    from acarsdec_amd import decoder
    from acarsdec_amd import _capi as K
    assert K.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return decoder


@pytest.fixture(scope="module")
def fix():
    pcm = np.load(os.path.join(GOLDEN, "msgjson_pcm16.npz"))["pcm"]
    with open(os.path.join(GOLDEN, "msgjson_golden.json")) as f:
        g = json.load(f)
    x = pcm.astype(np.float32) / np.float32(32768.0)
    assert x.shape[0] == g["nch"] == 3 and x.shape[1] % CHUNK == 0
    j = json.loads(g["variants"]["none"]["lines"][0])
    return x, g, (j["app"]["name"], j["app"]["ver"])


def new_decoder(D, nch=3, json_on=True, app=("acarsdec", "3.7"), station="STN1", **kw):
    dec = D.Decoder(nch, decim=8, ntaps=8, max_blocks=CHUNK // 1024, repair=True, bitlog=False, **kw)
    if json_on:
        dec.enable_json(T0, station, app[0], app[1])
    return dec


def play(dec, x, per_call=None):
    out = []
    for s in range(0, x.shape[1], CHUNK):
        dec.demod_msk(x[:, s:s + CHUNK])
        if per_call:
            out.append(per_call())
    return out


@pytest.fixture(scope="module")
def base_msgs(D, fix):
    """the fixture's records from a decoder that never enables JSON: (K.Msg, K.Oooi) in drain order, drained after every call"""
    x, g, app = fix
    dec = new_decoder(D, json_on=False)
    got = sum(play(dec, x, lambda: dec.drain_msgs(oooi=True)), [])
    dec.close()
    assert len(got) == len(g["sent"])
    return got


def filter_kw(g, variant):
    args = g["variants"][variant]["args"]
    return dict(downlink_only="-A" in args, skip_empty="-e" in args, labels=g["label_list"] if "-b" in args else None)


def model_kw(g, variant):
    kw = filter_kw(g, variant)
    return dict(downlink_only=kw["downlink_only"], skip_empty=kw["skip_empty"], labels=LM.parse_label_filter(kw["labels"]))


def split_lines(blob):
    assert blob == b"" or blob.endswith(b"\n")
    return [ln + b"\n" for ln in blob.split(b"\n")[:-1]]


def chn_of(ln):
    return int(re.search(rb',"channel":(-?\d+),"freq":', ln).group(1))


def ts_token(m):
    return JM.print_number(JM.tv_double(*JM.tv(T0, m.soh_sample))).encode()


def test_drain_json_equals_the_reference_lines_byte_for_byte(D, fix, base_msgs):
    """Every filter variant: the fixture through demodulator, framing, repair, split, label pass and the JSON passes.  Per
    channel, drain_json()'s lines equal the reference program's, the time stamp's number cut out of both (the reference stamps
    its wall clock); that number equals the model's print of t0 + soh_sample / 12500 s, soh_sample from a second decoder."""
    x, g, app = fix
    for v in VARIANTS:
        dec = new_decoder(D, app=app, station=g["station"])
        dec.set_msg_filter(**filter_kw(g, v))
        lines = split_lines(b"".join(play(dec, x, dec.drain_json)))
        dec.close()
        ref = [ln.encode("ascii") + b"\n" for ln in g["variants"][v]["lines"]]
        assert len(lines) == len(ref), v
        kept = [m for m, _ in base_msgs if JM.keep(m, **model_kw(g, v))]
        for c in range(g["nch"]):
            mine = [JM.cut_timestamp(ln) for ln in lines if chn_of(ln) == c]
            want = [JM.cut_timestamp(ln)[0] for ln in ref if chn_of(ln) == c]
            assert [a for a, _ in mine] == want, (v, c)
            assert [t for _, t in mine] == [ts_token(m) for m in kept if m.chn == c], (v, c)


# ---- random records through the lab entry ---------------------------------------------------------------------------------
CTRL = np.array([1, 2, 4, 5, 6, 7, 0x0B, 0x0E, 0x1B, 0x1F], dtype=np.uint8)                 # \u00xx
TWO = np.frombuffer(b'"\\\b\f\n\r\t', dtype=np.uint8)
PLAIN = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789 ,./-abcxyz~\x7f\x80\xff", dtype=np.uint8)
ANY = np.concatenate([CTRL, TWO, PLAIN, np.zeros(3, dtype=np.uint8)])


def random_records(rng, n, K, nch):
    """n acg_msg records: texts of every length and escape class (all control characters: the longest line; all plain: the
    shortest; mixed with NULs), header strings with quotes, control characters and NULs, labels of DecodeLabel()'s table with
    texts that pass their checks, levels at ties and non-finite, records the repair dropped"""
    recs = np.zeros((n, C.sizeof(K.Msg)), dtype=np.uint8)
    M = K.Msg
    i32 = lambda v: np.frombuffer(np.int32(v).tobytes(), dtype=np.uint8)
    i64 = lambda v: np.frombuffer(np.int64(v).tobytes(), dtype=np.uint8)
    labels = [l for l, s in LM.TABLE.items() if s != "26"]
    ties = [0.05, -0.05, 0.25, -0.25, 0.35, -0.35, -0.04, 0.0, -0.0, np.inf, -np.inf, np.nan, -99.95, 3240.1, -3240.1]
    end_bits = rng.permutation(8 * n)[:n] if n > 3 else np.arange(n)
    for i in range(n):
        r = recs[i]
        r[M.chn.offset:M.chn.offset + 4] = i32(rng.integers(0, nch))
        r[M.err.offset:M.err.offset + 4] = i32(rng.choice([0, 0, 1, 2, 3, 12, 240]))
        lvl = np.float32(ties[i % len(ties)]) if i % 5 == 0 else np.float32(rng.uniform(-60, 10))
        r[M.lvl.offset:M.lvl.offset + 4] = np.frombuffer(lvl.tobytes(), dtype=np.uint8)
        # equal keys now and then: the sort is stable
        eb = int(end_bits[i]) if i % 11 else int(end_bits[i - 1 if i else 0])
        r[M.end_bit.offset:M.end_bit.offset + 8] = i64(eb)
        es = int(rng.integers(0, 10 ** 9)) if i % 3 else int(rng.integers(0, 4 * 10 ** 12))       # up to ten years: past 2^31 and 2^32 s
        r[M.end_sample.offset:M.end_sample.offset + 8] = i64(es)
        r[M.soh_sample.offset:M.soh_sample.offset + 8] = i64(es - int(rng.integers(0, 3000)))
        r[M.reserved2.offset] = 1 if rng.integers(0, 9) == 0 else 0                          # dropped by the repair
        hdr = lambda k: ANY[rng.integers(0, len(ANY), k)] if rng.integers(0, 3) == 0 else PLAIN[rng.integers(0, 36, k)]
        r[M.mode.offset] = hdr(1)[0]
        r[M.addr.offset:M.addr.offset + 7] = hdr(7)
        r[M.ack.offset] = rng.choice([0x21, 0x21, hdr(1)[0]])
        r[M.label.offset:M.label.offset + 2] = hdr(2)
        r[M.label.offset + 2] = rng.integers(0, 256)                                         # (not read)
        r[M.bid.offset] = rng.choice([0, 0x30 + rng.integers(0, 10), 0x41 + rng.integers(0, 26), hdr(1)[0]])
        r[M.no.offset:M.no.offset + 4] = hdr(4)
        r[M.fid.offset:M.fid.offset + 6] = hdr(6)
        r[M.bs.offset] = rng.choice([2, 3])
        r[M.be.offset] = rng.choice([3, 0x17])
        r[M.down.offset] = 1 if 0x30 <= r[M.bid.offset] <= 0x39 else 0
        kind = i % 8
        tl = int(rng.choice([rng.integers(0, 243), rng.integers(0, 20), 242, 64, 65, 128, 192, 63]))
        if kind == 0:
            txt = CTRL[rng.integers(0, len(CTRL), 242)]                                      # all \u00xx
            tl = 242 if i % 16 == 0 else tl
        elif kind == 1:
            txt = PLAIN[rng.integers(0, len(PLAIN), 242)]                                    # nothing to escape
        elif kind == 2:
            txt = TWO[rng.integers(0, len(TWO), 242)]
        elif kind == 3:                                                                      # a label that decodes
            lbl = labels[rng.integers(0, len(labels))]
            guards, copies, opt = LM.TABLE[lbl]
            txt = PLAIN[rng.integers(0, 36, 242)].copy()
            if txt[0] == ord("0"):
                txt[0] = ord("K")
            for off, alts in guards:
                txt[off:off + len(alts[0])] = np.frombuffer(alts[0], dtype=np.uint8)
            if rng.integers(0, 3) == 0:
                txt[rng.integers(0, 48)] = ANY[rng.integers(0, len(ANY))]                    # a quote, a control character or a NUL in a field
            r[M.label.offset:M.label.offset + 2] = np.frombuffer(lbl.encode(), dtype=np.uint8)
            tl = max(tl, 50)
        else:
            txt = ANY[rng.integers(0, len(ANY), 242)]
        r[M.txt.offset:M.txt.offset + 242] = txt                                             # (garbage behind txt_len stays)
        if rng.integers(0, 60) == 0:
            tl = int(rng.choice([-3, 300]))                                                  # clamped to 0 .. 242
        r[M.txt_len.offset:M.txt_len.offset + 4] = i32(tl)
    return recs


def model_buffer(K, recs, nch, cfg, fr, kw):
    """the lab entry's contract: kept records in (chn, end_bit) order (equal keys: input order), dropped records left out"""
    msgs = [K.Msg.from_buffer_copy(r.tobytes()) for r in recs]
    kept = [m for m in msgs if m.reserved2 in (b"\x00", 0) and JM.keep(m, **kw)]
    kept.sort(key=lambda m: (m.chn, m.end_bit))
    t0 = (cfg.t0_sec, cfg.t0_usec)
    lines = [JM.line(m, m.chn, JM.print_number(JM.tv_double(*JM.tv(t0, m.soh_sample))).encode(), station=cfg.station_id,
                     freq=JM.freq_token(fr[m.chn]), app=(cfg.app_name, cfg.app_ver)) for m in kept]
    return lines


SELFTEST_FILTERS = [dict(), dict(downlink_only=True), dict(skip_empty=True), dict(labels="Q1:44:QA:10:17:2Z:A\x01"),
                    dict(downlink_only=True, skip_empty=True, labels="Q1:44:QA:QT:8D:12:33")]


@pytest.mark.parametrize("n,filters", [(1, (0,)), (63, (1,)), (64, (2,)), (65, (3,)), (257, (0, 1, 2, 3, 4)), (5000, (0, 4))])
def test_random_records_render_like_the_model(D, n, filters):
    from acarsdec_amd import _capi as K
    L = K.load()
    rng = np.random.default_rng(1000 + n)
    nch = 7
    fr = [131725000, 131525000, 0, 129125000, 136975000, 1090000000, 131825000]
    hard = n >= 257                                              # the longest constant stretches: every byte a control character
    t0 = {1: (10 ** 9, 0), 63: (2 ** 30 - 20000, 999999), 65: (3999999999, 999920)}.get(n, (1700000000 + n, 80 * n))     # the domain's ends
    cfg = D.json_config(t0, b"\x01\x1f" * 16 if hard else b"S\"1" if n != 64 else b"",
                        b"\x02" * 16 if hard else b"acarsdec", b"\x03\"" * 8 if hard else b"3.7")
    recs = random_records(rng, n, K, nch)
    buf = (K.Msg * n).from_buffer_copy(recs.tobytes())
    fr_arr = np.array(fr, dtype=np.int32)
    for fi in filters:
        kw = SELFTEST_FILTERS[fi]
        f = D.make_msg_filter(**kw) if kw else None
        mkw = dict(downlink_only=kw.get("downlink_only", False), skip_empty=kw.get("skip_empty", False), labels=LM.parse_label_filter(kw.get("labels")))
        lines = model_buffer(K, recs, nch, cfg, fr, mkw)
        want = b"".join(lines)
        assert all(len(ln) <= K.JSON_LINE_MAX for ln in lines)
        cap = len(want) + 4096
        out = np.full(cap, 0xA5, dtype=np.uint8)
        nb, nl = C.c_size_t(0), C.c_int(0)
        rc = L.acg_selftest_msg_json(buf, n, C.byref(f) if f is not None else None, C.byref(cfg), fr_arr.ctypes.data, nch, out.ctypes.data, cap,
                                     C.byref(nb), C.byref(nl))
        assert rc == K.OK, (n, kw, rc)
        got = out[:nb.value].tobytes()
        if got != want:                                          # name the first line that differs
            gl, wl = split_lines_loose(got), lines
            k = next((i for i, (a, b) in enumerate(zip(gl + [None], wl + [None])) if a != b), None)
            assert False, (n, kw, k, gl[k] if k is not None and k < len(gl) else None, wl[k] if k is not None and k < len(wl) else None)
        assert nl.value == len(lines) and nb.value == len(want)
        assert (out[nb.value:] == 0xA5).all(), "bytes behind nbytes were written"
        if n == 5000 and fi == 0:
            offs = np.cumsum([0] + [len(ln) for ln in lines[:-1]])
            assert set((offs % 16).tolist()) == set(range(16))                         # every seam alignment occurs
            lens = [len(ln) for ln in lines]
            assert max(lens) > 1900 and min(lens) < 700, (max(lens), min(lens))         # all-control texts, short plain ones
        if len(want) > 1:                                        # too small a buffer: ACG_EAGAIN, the size, nothing written
            small = np.full(len(want), 0xA5, dtype=np.uint8)
            rc = L.acg_selftest_msg_json(buf, n, C.byref(f) if f is not None else None, C.byref(cfg), fr_arr.ctypes.data, nch, small.ctypes.data,
                                         len(want) - 1, C.byref(nb), C.byref(nl))
            assert rc == K.EAGAIN and nb.value == len(want) and (small == 0xA5).all()


def split_lines_loose(blob):
    """lines of a buffer that may be damaged (a text never holds a raw newline: it is escaped)"""
    return [ln + b"\n" for ln in blob.split(b"\n") if ln]


# ---- the contract ----------------------------------------------------------------------------------------------------------
def raw_drain(dec, K, cap, lag=None):
    buf = C.create_string_buffer(max(cap, 1))
    nb, nl = C.c_size_t(0), C.c_int(0)
    if lag is None:
        rc = dec.L.acg_drain_json(dec.ctx, buf, cap, C.byref(nb), C.byref(nl))
    else:
        rc = dec.L.acg_collect_json(dec.ctx, lag, buf, cap, C.byref(nb), C.byref(nl))
    return rc, buf.raw[:nb.value], nl.value


def test_state_and_argument_errors(D, fix):
    from acarsdec_amd import _capi as K
    x, g, app = fix
    plain = D.Decoder(3, decim=8, ntaps=8, max_blocks=4, repair=False, bitlog=False)
    cfg = D.json_config(T0, "STN1", "acarsdec", "3.7")
    assert plain.L.acg_json_enable(plain.ctx, C.byref(cfg), None) == K.ESTATE                # no ACG_F_REPAIR
    assert raw_drain(plain, K, 4 * K.JSON_LINE_MAX)[0] == K.ESTATE
    assert raw_drain(plain, K, 4 * K.JSON_LINE_MAX, lag=0)[0] == K.ESTATE
    plain.close()
    dec = new_decoder(D, json_on=False)
    dec.demod_msk(x[:, :CHUNK])
    assert raw_drain(dec, K, 4 * K.JSON_LINE_MAX)[0] == K.ESTATE                             # before acg_json_enable
    for bad in ((999999999, 0), (4000000000, 0), (1700000000, 1000000)):
        c = K.JsonConfig(bad[0], bad[1], b"", b"a", b"1")
        assert dec.L.acg_json_enable(dec.ctx, C.byref(c), None) == K.EINVAL
    dec.enable_json(T0, "STN1", *app)
    assert raw_drain(dec, K, K.JSON_LINE_MAX - 1)[0] == K.EINVAL
    assert raw_drain(dec, K, K.JSON_LINE_MAX - 1, lag=0)[0] == K.EINVAL
    first = dec.drain_json()                                                                 # nothing was consumed by the refused calls
    dec.disable_json()
    dec.demod_msk(x[:, CHUNK:2 * CHUNK])
    assert raw_drain(dec, K, 4 * K.JSON_LINE_MAX)[0] == K.ESTATE                             # disabled: off again, nothing consumed
    dec.enable_json(T0, "STN1", *app)                                                        # ... and on again
    second = dec.drain_json()
    dec.reset()                                                                              # acg_reset keeps the configuration
    dec.demod_msk(x[:, :CHUNK])
    again = dec.drain_json()
    dec.close()
    twin = new_decoder(D, app=app)
    twin.demod_msk(x[:, :CHUNK])
    a = twin.drain_json()
    twin.demod_msk(x[:, CHUNK:2 * CHUNK])
    b = twin.drain_json()
    twin.close()
    assert first == a and second == b and again == a and len(split_lines(a + b)) > 0


def test_small_buffer_says_again_and_loses_nothing(D, fix):
    """the whole fixture queued, then drained through a buffer of five lines: ACG_EAGAIN until the queue is empty; the union of
    what the calls hand out is what one big drain hands out, nothing lost, nothing repeated; each call's lines are ordered"""
    from acarsdec_amd import _capi as K
    x, g, app = fix
    small, big = new_decoder(D, app=app), new_decoder(D, app=app)
    ncall = 6                                                    # (the block queue holds the calls of acg_max_lag() + 1)
    assert small.max_lag + 1 >= ncall
    for dec in (small, big):
        play(dec, x[:, :ncall * CHUNK])
    whole = split_lines(big.drain_json())
    parts, codes = [], []
    for _ in range(len(whole) + 2):
        rc, blob, nl = raw_drain(small, K, 5 * K.JSON_LINE_MAX)
        codes.append(rc)
        lines = split_lines(blob)
        assert rc in (K.OK, K.EAGAIN) and nl == len(lines) <= 5
        keys = [(chn_of(ln), ln) for ln in lines]
        assert [k[0] for k in keys] == sorted(k[0] for k in keys)
        parts += lines
        if rc == K.OK:
            break
    assert codes[-1] == K.OK and codes.count(K.EAGAIN) == len(codes) - 1 >= 2
    assert len(whole) > 10 and sorted(parts) == sorted(whole)
    for c in range(3):                                           # per channel the order is completion order in both
        assert [ln for ln in parts if chn_of(ln) == c] == [ln for ln in whole if chn_of(ln) == c]
    assert raw_drain(small, K, 5 * K.JSON_LINE_MAX) == (K.OK, b"", 0)
    small.close()
    big.close()


def test_collect_with_lag_equals_drain(D, fix):
    x, g, app = fix
    lagging, draining = new_decoder(D, app=app, max_lag=1), new_decoder(D, app=app)
    got = b"".join(play(lagging, x, lambda: lagging.collect_json(lag=1))) + lagging.collect_json(lag=0)
    want = b"".join(play(draining, x, draining.drain_json))
    lagging.close()
    draining.close()
    assert len(split_lines(want)) == len(g["sent"])
    for c in range(3):
        assert [ln for ln in split_lines(got) if chn_of(ln) == c] == [ln for ln in split_lines(want) if chn_of(ln) == c]


def test_flight_table_is_updated_by_the_json_entry_points(D, fix):
    """with the flight table on, the snapshot and the routes after JSON drains equal those after drain_msgs drains"""
    x, g, app = fix
    by_json, by_msgs = new_decoder(D, app=app), new_decoder(D, json_on=False)
    for dec in (by_json, by_msgs):
        dec.enable_flights(t0=T0, mdly=600, max_flights=64)
    play(by_json, x, by_json.drain_json)
    play(by_msgs, x, by_msgs.drain_msgs)
    a, b = by_json.flights(), by_msgs.flights()
    ra, rb = by_json.drain_routes(), by_msgs.drain_routes()
    by_json.close()
    by_msgs.close()
    assert len(a) > 0 and [bytes(f) for f in a] == [bytes(f) for f in b]
    assert [bytes(r) for r in ra] == [bytes(r) for r in rb]


def test_existing_message_paths_are_untouched_by_an_enabled_sink(D, fix, base_msgs):
    """a context with JSON enabled hands out, through drain_msgs(oooi=True), records byte-identical to one that never enabled it"""
    x, g, app = fix
    dec = new_decoder(D, app=app)
    got = sum(play(dec, x, lambda: dec.drain_msgs(oooi=True)), [])
    dec.close()
    assert [bytes(m) + bytes(o) for m, o in got] == [bytes(m) + bytes(o) for m, o in base_msgs]


# ---- the level --------------------------------------------------------------------------------------------------------------
def level_of(ln):
    return re.search(rb',"level":([^,]*),"error":', ln).group(1).decode()


def test_level_text_equals_the_host_computed_record(D, fix, base_msgs):
    """The device takes log10 itself; the host's records carry glibc's.  On the fixture and on 1024 synthetic channels of varied
    amplitude every line's level equals '%2.1f' of the record's lvl; the assertion reports the guard counter (lines whose double
    lay within 8 ulp of a float rounding boundary, the only ones that could differ)."""
    from acarsdec_amd import synth as S
    x, g, app = fix
    dec = new_decoder(D, app=app)
    lines = split_lines(b"".join(play(dec, x, dec.drain_json)))
    guard = dec.json_level_guard()
    dec.close()
    for c in range(3):
        assert [level_of(ln) for ln in lines if chn_of(ln) == c] == ["%2.1f" % m.lvl for m, _ in base_msgs if m.chn == c], ("fixture", c, guard)
    rng = np.random.default_rng(3)
    nch, nsamp = 1024, 2 * CHUNK
    audio, frames = S.channel_audio(rng, 40000, nframes=8, gap=(600, 900), text_len=(5, 40))
    ends = np.flatnonzero(np.abs(audio) > 0)
    pieces, start = [], None
    for i in range(ends.size):                                   # the transmissions of the one track, cut apart at the silences
        if start is None:
            start = ends[i]
        if i + 1 == ends.size or ends[i + 1] - ends[i] > 300:
            pieces.append(audio[start:ends[i] + 1].astype(np.float32))
            start = None
    assert len(pieces) == len(frames) == 8
    y = np.zeros((nch, nsamp), dtype=np.float32)
    for c in range(nch):
        t = int(rng.integers(200, 1200))
        while True:
            a = pieces[rng.integers(0, len(pieces))]
            if t + a.size >= nsamp - 200:
                break
            y[c, t:t + a.size] = a * np.float32(rng.uniform(0.01, 0.9))
            t += a.size + int(rng.integers(500, 1200))
    decs = [new_decoder(D, nch=nch, app=app), new_decoder(D, nch=nch, json_on=False)]
    for d in decs:
        play(d, y)
    lines = split_lines(decs[0].drain_json(max_lines=8192))
    msgs = decs[1].drain_msgs(max_msgs=8192)
    guard = decs[0].json_level_guard()
    for d in decs:
        d.close()
    assert len(msgs) > nch and len(lines) == len(msgs)
    bad = [(m.chn, level_of(ln), "%2.1f" % m.lvl) for ln, m in zip(lines, msgs) if level_of(ln) != "%2.1f" % m.lvl or chn_of(ln) != m.chn]
    assert not bad, (bad[:5], len(bad), "guard counter: %d of %d" % (guard, len(lines)))
    assert len({level_of(ln) for ln in lines}) > 50                                        # the levels really vary
