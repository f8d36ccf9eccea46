"""The text sink on the device (text.hip): what acg_drain_text / acg_collect_text hand out against the bytes the unmodified
reference program printed for the text fixture (-o 1, -o 2), byte for byte; designed and random records through the lab entry
against the Python model (tests/text_model.py), whole buffer and offset table, for the four formats and every legal flag
combination; the drain / collect contract; the existing message and JSON paths untouched.  GPU box only."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
import label_model as LM
import text_model as TM

pytestmark = pytest.mark.gpu

VARIANTS = ("none", "A", "e", "b", "Aeb")
T0 = (1792301725, 269667)
CHUNK = 4096
COMBOS = [(fmt, fl) for fmt in (TM.ONELINE, TM.STD, TM.PP, TM.SV) for fl in TM.FLAGS_OF[fmt]]


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
        gj = json.load(f)
    with open(os.path.join(GOLDEN, "msgtext_golden.json")) as f:
        gt = json.load(f)
    x = pcm.astype(np.float32) / np.float32(32768.0)
    assert x.shape[0] == gj["nch"] == 3 and x.shape[1] % CHUNK == 0
    return x, gj, gt


def new_decoder(D, text=None, nch=3, **kw):
    """text: None or (fmt, flags) -> enable_text with T0"""
    dec = D.Decoder(nch, decim=8, ntaps=8, max_blocks=CHUNK // 1024, repair=True, bitlog=False, **kw)
    if text is not None:
        enable(dec, *text)
    return dec


def enable(dec, fmt, flags, station="STN1", freqs_hz=None):
    dec.enable_text(fmt, T0, date=bool(flags & TM.F_DATE), freq=bool(flags & TM.F_FREQ), station_id=station, freqs_hz=freqs_hz)


def play(dec, x, per_call=None):
    out = []
    for s in range(0, x.shape[1], CHUNK):
        dec.demod_msk(x[:, s:s + CHUNK])
        if per_call:
            out.append(per_call())
    return out


@pytest.fixture(scope="module")
def base_msgs(D, fix):
    """the fixture's records from a decoder that never enables a sink: (K.Msg, K.Oooi) in drain order, drained after every call"""
    x, gj, _ = fix
    dec = new_decoder(D)
    got = sum(play(dec, x, lambda: dec.drain_msgs(oooi=True)), [])
    dec.close()
    assert len(got) == len(gj["sent"])
    return got


def filter_kw(gj, variant):
    args = gj["variants"][variant]["args"]
    return dict(downlink_only="-A" in args, skip_empty="-e" in args, labels=gj["label_list"] if "-b" in args else None)


def test_drain_text_equals_the_reference_bytes(D, fix):
    """Every filter variant, -o 1 and -o 2: the fixture through demodulator, framing, repair, split, label pass and the text
    passes.  Per channel and in order, drain_text()'s records equal the records of the reference program's stdout."""
    x, gj, gt = fix
    for v in VARIANTS:
        for fmt, key, split in ((TM.ONELINE, "o1", TM.split_oneline), (TM.STD, "o2", TM.split_std)):
            dec = new_decoder(D, text=(fmt, 0))
            dec.set_msg_filter(**filter_kw(gj, v))
            recs = sum(play(dec, x, dec.drain_text), [])
            dec.close()
            ref = split(bytes.fromhex(gt["variants"][v][key]))
            assert len(recs) == len(ref) == gt["variants"][v]["records"], (v, key)
            for c in range(gj["nch"]):
                assert [r for r in recs if TM.chn_of(r) == c] == [r for r in ref if TM.chn_of(r) == c], (v, key, c)


def test_every_format_equals_the_model_on_the_fixtures_records(D, fix, base_msgs):
    """all four formats with every flag they take, station and frequencies set: what drain_text hands out equals the model's
    record of the (acg_msg, acg_oooi) a second decoder drains -- dates from soh_sample, levels from the host-computed lvl (the
    assertion reports the guard counter: records whose level could differ)"""
    x, gj, _ = fix
    fr = [131725000, 131525000, 129125000]
    for fmt, flags in ((TM.ONELINE, TM.F_DATE), (TM.STD, TM.F_DATE | TM.F_FREQ), (TM.PP, 0), (TM.SV, 0)):
        dec = new_decoder(D)
        enable(dec, fmt, flags, station="STATION-9", freqs_hz=fr)
        recs = sum(play(dec, x, dec.drain_text), [])
        guard = dec.text_level_guard()
        dec.close()
        oo = lambda o: (o.decoded not in (b"\x00", 0), {f: getattr(o, f) for f, _ in TM.OOOI_LINES})
        want = [TM.record(m, m.chn, fmt, flags, t0=T0, station=b"STATION-9", fr_hz=fr[m.chn], oooi=oo(o)) for m, o in base_msgs]
        assert len(recs) == len(want)
        # per C call the order is (chn, end_bit); base_msgs came from the same calls
        assert sorted(recs) == sorted(want), (fmt, flags, guard)
        assert recs == want, (fmt, flags, guard)


# ---- designed + random records through the lab entry ---------------------------------------------------------------------
PLAIN = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789", dtype=np.uint8)
ANY = np.concatenate([np.frombuffer(b"\x01\x1f\"\\\t\n\r ~\x7f\x80\xff", dtype=np.uint8), PLAIN])
TEXT_LENS = (0, 1, 58, 59, 60, 63, 64, 65, 241, 242)
LEVELS = (0.05, -0.05, 0.25, -0.25, 0.35, -0.35, -0.04, 0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, -7.9, 7.9, -9.95, -10.0, -12.34, -99.95,
          9.96, 3240.1, -3240.1, 123456.7)
CHNS = (0, 8, 98, 998, 9998, 99998, 999998, 1048575)            # chn + 1 has 1 .. 7 digits
NCH = 1 << 20
T0_SELF = (10 ** 9, 79)                                          # soh_sample = (S - 10^9) 12500 + 12499 -> S.999999


def string_field(rng, i, n):
    """a header string of capacity n at length 0, 1, full, and with an inner NUL"""
    v = PLAIN[rng.integers(0, len(PLAIN), n)].copy() if i % 5 else ANY[rng.integers(0, len(ANY), n)].copy()
    v[v == 0] = 0x41
    kind = i % 4
    if kind == 0:
        v[:] = 0
    elif kind == 1:
        v[1:] = 0
    elif kind == 3 and n > 1:
        v[1 + i % (n - 1)] = 0
    return v


def designed_records(rng, n, K):
    """n acg_msg records that walk through every branch of the four formats (the cycles have coprime periods, so the
    combinations mix): see the issue's list in test_designed_records_render_like_the_model"""
    recs = np.zeros((n, C.sizeof(K.Msg)), dtype=np.uint8)
    M = K.Msg
    put = lambda r, f, v, dt: r.__setitem__(slice(f.offset, f.offset + np.dtype(dt).itemsize), np.frombuffer(np.array(v, dtype=dt).tobytes(), dtype=np.uint8))
    labels = [l for l, s in LM.TABLE.items() if s != "26"]
    end_bits = rng.permutation(8 * n)[:n] if n > 3 else np.arange(n)
    nq1 = n17 = 0
    for i in range(n):
        r = recs[i]
        put(r, M.chn, CHNS[i % len(CHNS)], np.int32)
        put(r, M.err, (0, 10, 3, 240)[i % 4], np.int32)
        put(r, M.lvl, LEVELS[i % len(LEVELS)] if i % 3 else rng.uniform(-60, 10), np.float32)
        put(r, M.end_bit, int(end_bits[i]) if i % 11 else int(end_bits[i - 1 if i else 0]), np.int64)      # equal keys now and then
        if i % 2:
            soh = (TM.NAMED_SECONDS[(i // 2) % len(TM.NAMED_SECONDS)] - T0_SELF[0]) * 12500 + 12499              # S.999999: ms 999
        else:
            soh = int(rng.integers(0, 4 * 10 ** 13))
        put(r, M.soh_sample, soh, np.int64)
        put(r, M.end_sample, soh + int(rng.integers(0, 3000)), np.int64)
        r[M.reserved2.offset] = 1 if i % 13 == 12 else 0                                                   # dropped by the repair
        r[M.mode.offset] = (0x32, 0, 0x0A, 0x58)[(i // 3) % 4]
        r[M.ack.offset] = (0x21, 0, 0x4B, 0x0D)[(i // 5) % 4]
        r[M.bid.offset] = (0, 0x30 + i % 10, 0x41 + i % 26, 0x39, 0x0A)[(i // 7) % 5]
        r[M.addr.offset:M.addr.offset + 7] = string_field(rng, i, 7)
        r[M.addr.offset + 7] = 0x5A if i % 6 == 0 else 0                                                   # (not read: "%7s" of 7 bytes)
        r[M.fid.offset:M.fid.offset + 6] = string_field(rng, i // 4, 6)
        r[M.label.offset:M.label.offset + 2] = string_field(rng, i // 16, 2)
        r[M.label.offset + 2] = rng.integers(0, 256)                                                       # (not read)
        r[M.no.offset:M.no.offset + 4] = string_field(rng, i // 64, 4)
        r[M.be.offset] = (3, 0x17)[(i // 2) % 2]
        r[M.down.offset] = 1 if 0x30 <= r[M.bid.offset] <= 0x39 else 0
        tl = TEXT_LENS[i % len(TEXT_LENS)]
        txt = PLAIN[rng.integers(0, len(PLAIN), 242)].copy()
        where = (None, 0, 58, 59, "end", "nul", "any")[(i // len(TEXT_LENS)) % 7]
        if where == "any":
            txt = ANY[rng.integers(0, len(ANY), 242)].copy()
        elif where == "nul":
            txt[tl // 2] = 0
        elif where is not None:
            at = tl - 1 if where == "end" else where
            if 0 <= at < 242:
                txt[at] = 0x0A if i % 2 else 0x0D
        if i % 7 == 4:                                                                                     # a label that decodes
            d = i // 7
            live = i % 13 != 12                                                                            # (not dropped by the repair)
            if d % 3 != 2 and live:
                lbl, mask = "Q1", nq1 % 64                                                                 # every subset of its six fields
                nq1 += 1
            elif d % 2 and live:
                lbl, mask = "17", n17 % 8                                                                  # every subset of eta, sa, da
                n17 += 1
            else:
                lbl, mask = labels[d % len(labels)], 0
            guards, copies, opt = LM.TABLE[lbl]
            txt = PLAIN[rng.integers(0, len(PLAIN), 242)].copy()
            if txt[0] == ord("0"):
                txt[0] = ord("K")
            for off, alts in guards:
                txt[off:off + len(alts[0])] = np.frombuffer(alts[0], dtype=np.uint8)
            for k, (f, off) in enumerate(copies):
                if (mask >> k) & 1:
                    txt[off] = 0                                                                           # the field is empty: no line
            r[M.label.offset:M.label.offset + 2] = np.frombuffer(lbl.encode(), dtype=np.uint8)
            tl = max(tl, 64)
        r[M.txt.offset:M.txt.offset + 242] = txt                                                           # (garbage behind txt_len stays)
        if i % 61 == 60:
            tl = (-3, 300)[(i // 61) % 2]                                                                  # clamped to 0 .. 242
        put(r, M.txt_len, tl, np.int32)
    return recs


def run_selftest(K, L, D, recs, cfg, fr_arr, flt=None):
    n = recs.shape[0]
    buf = (K.Msg * n).from_buffer_copy(recs.tobytes())
    cap = n * K.TEXT_REC_MAX
    out = np.full(cap + 64, 0xA5, dtype=np.uint8)
    offs = np.full(n + 2, 0xA5A5A5A5, dtype=np.uint32)
    nb, nr = C.c_size_t(0), C.c_int(0)
    rc = L.acg_selftest_msg_text(buf, n, C.byref(flt) if flt is not None else None, C.byref(cfg), fr_arr.ctypes.data, NCH, out.ctypes.data, cap,
                                 C.byref(nb), offs.ctypes.data, C.byref(nr))
    return rc, out, offs, nb.value, nr.value


@pytest.fixture(scope="module")
def fr_arr():
    rng = np.random.default_rng(5)
    fr = rng.integers(118000000, 137000000, NCH).astype(np.int32)
    fr[0], fr[8], fr[98], fr[998] = 0, 131725000, 2147483647, -2147483648
    return fr


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_designed_records_render_like_the_model(D, fr_arr, n):
    """acg_selftest_msg_text against the model, whole buffer plus offset table, all four formats with each legal flag combination.
    The records are designed so that (at n = 1000, asserted there) every branch appears: every string field at length 0, 1, full and
    with an inner NUL; text lengths 0, 1, 58, 59, 60, 63, 64, 65, 241, 242; '\\n' / '\\r' at byte 0, 58, 59 and at the end; NUL mode,
    ack and bid; uplinks and downlinks; ETB; levels at tenths ties, negative, below -10, +-0, inf and nan; chn + 1 of 1 to 7
    digits; err 0 and 10; times on the dates of the CPU test at usec 999 999; every OOOI subset DecodeLabel() can produce from a text
    (the records enter in front of the label pass: all 64 subsets of label Q1's six fields, all 8 of label 17's eta, sa, da, so
    every line with and without each other); both ends of a record at every offset mod 16."""
    from acarsdec_amd import _capi as K
    L = K.load()
    rng = np.random.default_rng(2000 + n)
    recs = designed_records(rng, n, K)
    msgs = [K.Msg.from_buffer_copy(r.tobytes()) for r in recs]
    kept = sorted((m for m in msgs if m.reserved2 in (b"\x00", 0)), key=lambda m: (m.chn, m.end_bit))
    station = {1: b"", 63: b"S", 64: b"EIGHT--8", 65: b"NINE----9"}.get(n, b"X" * 32)
    for fmt, flags in COMBOS:
        cfg = D.text_config(fmt, T0_SELF, date=bool(flags & TM.F_DATE), freq=bool(flags & TM.F_FREQ), station_id=station)
        want = [TM.record(m, m.chn, fmt, flags, t0=T0_SELF, station=station, fr_hz=int(fr_arr[m.chn])) for m in kept]
        blob = b"".join(want)
        woffs = np.cumsum([0] + [len(w) for w in want])
        assert all(0 < len(w) <= K.TEXT_REC_MAX for w in want)
        rc, out, offs, nb, nr = run_selftest(K, L, D, recs, cfg, fr_arr)
        assert rc == K.OK, (n, fmt, flags, rc)
        assert nr == len(want) and nb == len(blob), (n, fmt, flags, nr, len(want), nb, len(blob))
        assert offs[:nr + 1].tolist() == woffs.tolist(), (n, fmt, flags)
        got = out[:nb].tobytes()
        if got != blob:                                          # name the first record that differs
            k = next(i for i in range(nr) if got[woffs[i]:woffs[i + 1]] != want[i])
            assert False, (n, fmt, flags, k, got[woffs[k]:woffs[k + 1]], want[k])
        assert (out[nb:] == 0xA5).all() and offs[nr + 1] == 0xA5A5A5A5, "bytes behind the result were written"
        if n == 1000:
            assert set((woffs % 16).tolist()) == set(range(16)), (fmt, flags)            # both ends of a record at every offset mod 16
        if len(blob) > 1:                                        # too small a buffer: ACG_EAGAIN, the size, nothing written
            buf = (K.Msg * n).from_buffer_copy(recs.tobytes())
            small, so = np.full(len(blob), 0xA5, dtype=np.uint8), np.full(n + 1, 0xA5A5A5A5, dtype=np.uint32)
            cnb, cnr = C.c_size_t(0), C.c_int(0)
            rc = L.acg_selftest_msg_text(buf, n, None, C.byref(cfg), fr_arr.ctypes.data, NCH, small.ctypes.data, len(blob) - 1, C.byref(cnb),
                                         so.ctypes.data, C.byref(cnr))
            assert rc == K.EAGAIN and cnb.value == len(blob) and (small == 0xA5).all() and (so == 0xA5A5A5A5).all()
    if n == 1000:                                                # the design reaches every branch
        s = lambda m, f, k: TM.cstr(getattr(m, f), k)
        for f, k in (("addr", 7), ("fid", 6), ("no", 4)):
            assert {0, 1, k} <= {len(s(m, f, k)) for m in kept} and any(1 < len(s(m, f, k)) < k for m in kept), f
        assert {0, 1, 2} == {len(TM.cstr((bytes(m.label) + b"\0\0")[:2])) for m in kept}
        tls = {max(0, min(m.txt_len, 242)) for m in kept}
        assert set(TEXT_LENS) <= tls
        for at in (0, 58, 59):
            assert any(m.txt_len > at and bytes(m.txt)[at] in (10, 13) and 0 not in bytes(m.txt)[:at] for m in kept), at
        assert any(m.txt_len > 1 and bytes(m.txt)[m.txt_len - 1] in (10, 13) and 0 not in bytes(m.txt)[:m.txt_len] for m in kept)
        assert any(0 in bytes(m.txt)[1:max(1, min(m.txt_len, 242))] for m in kept)
        for f in ("mode", "ack", "bid"):
            assert any(getattr(m, f) == b"\x00" for m in kept) and any(getattr(m, f) != b"\x00" for m in kept), f
        assert any(b"0" <= m.bid <= b"9" for m in kept) and any(m.bid >= b"A" for m in kept) and any(m.be == b"\x17" for m in kept)
        assert {0, 10} <= {m.err for m in kept} and {len(str(m.chn + 1)) for m in kept} == set(range(1, 8))
        lv = [m.lvl for m in kept]
        assert any(np.isnan(v) for v in lv) and any(np.isinf(v) for v in lv) and any(v < -10 for v in lv) and any(v == 0 and np.signbit(v) for v in lv)
        stds = [TM.record(m, m.chn, TM.STD, TM.F_DATE, t0=T0_SELF) for m in kept]
        dates = b"".join(stds)
        for piece in (b"09/09/2001 01:46:40.999", b"19/01/2038 03:14:07.999", b"19/01/2038 03:14:08.999", b"28/02/2100 23:59:59.999", b"01/03/2100 00:00:00.999",
                      b"29/02/2104 00:00:00.999", b"01/03/2104 00:00:00.999", b"Nak\n", b"ETB\n"):
            assert piece in dates, piece
        heads = dict(TM.OOOI_LINES)
        for lbl, fields in ((b"Q1", ("sa", "gout", "woff", "won", "gin", "da")), (b"17", ("eta", "sa", "da"))):
            mine = [r for m, r in zip(kept, stds) if bytes(m.label)[:2] == lbl and b"#" * 26 in r]
            subsets = {tuple(heads[f] in r for f in fields) for r in mine}
            assert len(subsets) == 2 ** len(fields), (lbl, len(subsets))
        assert all(any(head in r for r in stds) for head in heads.values())


def test_filters_apply_to_the_lab_entry(D, fr_arr):
    """-A, -e and -b on 257 designed records: the records of exactly the messages the model's filter keeps"""
    from acarsdec_amd import _capi as K
    L = K.load()
    recs = designed_records(np.random.default_rng(257), 257, K)
    msgs = [K.Msg.from_buffer_copy(r.tobytes()) for r in recs]
    cfg = D.text_config("std", T0_SELF, date=True, freq=True)
    for kw in (dict(downlink_only=True), dict(skip_empty=True), dict(labels="Q1:44:QA:10:17:AB"), dict(downlink_only=True, skip_empty=True)):
        mkw = dict(downlink_only=kw.get("downlink_only", False), skip_empty=kw.get("skip_empty", False), labels=LM.parse_label_filter(kw.get("labels")))
        kept = sorted((m for m in msgs if m.reserved2 in (b"\x00", 0) and TM.keep(m, **mkw)), key=lambda m: (m.chn, m.end_bit))
        want = [TM.record(m, m.chn, TM.STD, TM.F_DATE | TM.F_FREQ, t0=T0_SELF, fr_hz=int(fr_arr[m.chn])) for m in kept]
        flt = D.make_msg_filter(**kw)
        rc, out, offs, nb, nr = run_selftest(K, L, D, recs, cfg, fr_arr, flt)
        assert rc == K.OK and 0 < nr == len(want) < 257 and out[:nb].tobytes() == b"".join(want), kw


# ---- the contract ----------------------------------------------------------------------------------------------------------
def raw_drain(dec, K, cap, max_recs, lag=None):
    buf = C.create_string_buffer(max(cap, 1))
    offs = (C.c_uint * (max(max_recs, 0) + 2))()
    nb, nr = C.c_size_t(0), C.c_int(0)
    if lag is None:
        rc = dec.L.acg_drain_text(dec.ctx, buf, cap, C.byref(nb), offs, max_recs, C.byref(nr))
    else:
        rc = dec.L.acg_collect_text(dec.ctx, lag, buf, cap, C.byref(nb), offs, max_recs, C.byref(nr))
    blob = buf.raw[:nb.value]
    assert offs[0] == 0 and offs[nr.value] == nb.value
    return rc, [blob[offs[i]:offs[i + 1]] for i in range(nr.value)]


def test_state_and_argument_errors(D, fix):
    from acarsdec_amd import _capi as K
    x, _, _ = fix
    R = K.TEXT_REC_MAX
    plain = D.Decoder(3, decim=8, ntaps=8, max_blocks=4, repair=False, bitlog=False)
    cfg = D.text_config("oneline", T0, date=True)
    assert plain.L.acg_text_enable(plain.ctx, C.byref(cfg), None) == K.ESTATE                # no ACG_F_REPAIR
    assert raw_drain(plain, K, 4 * R, 4)[0] == K.ESTATE
    assert raw_drain(plain, K, 4 * R, 4, lag=0)[0] == K.ESTATE
    plain.close()
    dec = new_decoder(D)
    dec.demod_msk(x[:, :CHUNK])
    assert raw_drain(dec, K, 4 * R, 4)[0] == K.ESTATE                                        # before acg_text_enable
    for bad in (K.TextConfig(0, 0, T0[0], 0, b""), K.TextConfig(5, 0, T0[0], 0, b""), K.TextConfig(K.TEXT_ONELINE, K.TEXT_F_FREQ, T0[0], 0, b""),
                K.TextConfig(K.TEXT_PP, K.TEXT_F_DATE, T0[0], 0, b""), K.TextConfig(K.TEXT_SV, K.TEXT_F_FREQ, T0[0], 0, b""),
                K.TextConfig(K.TEXT_STD, 8, T0[0], 0, b""), K.TextConfig(K.TEXT_STD, 0, 999999999, 0, b""), K.TextConfig(K.TEXT_STD, 0, 4000000000, 0, b""),
                K.TextConfig(K.TEXT_STD, 0, T0[0], 1000000, b"")):
        assert dec.L.acg_text_enable(dec.ctx, C.byref(bad), None) == K.EINVAL
    assert raw_drain(dec, K, 4 * R, 4)[0] == K.ESTATE                                        # a refused configuration enables nothing
    enable(dec, TM.ONELINE, TM.F_DATE)
    assert raw_drain(dec, K, R - 1, 4)[0] == K.EINVAL
    assert raw_drain(dec, K, 4 * R, 0)[0] == K.EINVAL
    assert raw_drain(dec, K, R - 1, 4, lag=0)[0] == K.EINVAL
    assert raw_drain(dec, K, 4 * R, 4, lag=-1)[0] == K.EINVAL
    first = dec.drain_text()                                                                 # nothing was consumed by the refused calls
    dec.disable_text()
    dec.demod_msk(x[:, CHUNK:2 * CHUNK])
    assert raw_drain(dec, K, 4 * R, 4)[0] == K.ESTATE                                        # disabled: off again, nothing consumed
    enable(dec, TM.ONELINE, TM.F_DATE)                                                       # ... and on again
    second = dec.drain_text()
    dec.reset()                                                                              # acg_reset keeps the configuration
    dec.demod_msk(x[:, :CHUNK])
    again = dec.drain_text()
    dec.close()
    twin = new_decoder(D, text=(TM.ONELINE, TM.F_DATE))
    twin.demod_msk(x[:, :CHUNK])
    a = twin.drain_text()
    twin.demod_msk(x[:, CHUNK:2 * CHUNK])
    b = twin.drain_text()
    twin.close()
    assert first == a and second == b and again == a and len(a + b) > 0


@pytest.mark.parametrize("cap_recs,max_recs", [(5, 4096), (4096, 3)])
def test_small_buffer_says_again_and_loses_nothing(D, fix, cap_recs, max_recs):
    """the fixture's first calls queued, then drained through a buffer of five records / an offset table of three: ACG_EAGAIN
    until the queue is empty; the records concatenated over the calls are what one big drain hands out"""
    from acarsdec_amd import _capi as K
    x, _, _ = fix
    small, big = new_decoder(D, text=(TM.STD, TM.F_DATE)), new_decoder(D, text=(TM.STD, TM.F_DATE))
    ncall = 6                                                    # (the block queue holds the calls of acg_max_lag() + 1)
    assert small.max_lag + 1 >= ncall
    for dec in (small, big):
        play(dec, x[:, :ncall * CHUNK])
    whole = big.drain_text()
    limit = min(cap_recs, max_recs)
    parts, codes = [], []
    for _ in range(len(whole) + 2):
        rc, recs = raw_drain(small, K, cap_recs * K.TEXT_REC_MAX, max_recs)
        codes.append(rc)
        assert rc in (K.OK, K.EAGAIN) and len(recs) <= limit
        assert [TM.chn_of(r) for r in recs] == sorted(TM.chn_of(r) for r in recs)
        parts += recs
        if rc == K.OK:
            break
    assert codes[-1] == K.OK and codes.count(K.EAGAIN) == len(codes) - 1 >= 2
    assert len(whole) > 10 and sorted(parts) == sorted(whole)
    for c in range(3):                                           # per channel the order is completion order in both
        assert [r for r in parts if TM.chn_of(r) == c] == [r for r in whole if TM.chn_of(r) == c]
    assert raw_drain(small, K, cap_recs * K.TEXT_REC_MAX, max_recs) == (K.OK, [])
    small.close()
    big.close()


def test_collect_with_lag_equals_drain(D, fix):
    x, gj, _ = fix
    lagging, draining = new_decoder(D, text=(TM.ONELINE, TM.F_DATE), max_lag=1), new_decoder(D, text=(TM.ONELINE, TM.F_DATE))
    got = sum(play(lagging, x, lambda: lagging.collect_text(lag=1)), []) + lagging.collect_text(lag=0)
    want = sum(play(draining, x, draining.drain_text), [])
    lagging.close()
    draining.close()
    assert len(want) == len(gj["sent"])
    for c in range(3):
        assert [r for r in got if TM.chn_of(r) == c] == [r for r in want if TM.chn_of(r) == c]


def test_flight_table_is_updated_by_the_text_entry_points(D, fix):
    """with the flight table on, the snapshot and the routes after text drains equal those after drain_msgs drains"""
    x, _, _ = fix
    by_text, by_msgs = new_decoder(D, text=(TM.PP, 0)), new_decoder(D)
    for dec in (by_text, by_msgs):
        dec.enable_flights(t0=T0, mdly=600, max_flights=64)
    play(by_text, x, by_text.drain_text)
    play(by_msgs, x, by_msgs.drain_msgs)
    a, b = by_text.flights(), by_msgs.flights()
    ra, rb = by_text.drain_routes(), by_msgs.drain_routes()
    by_text.close()
    by_msgs.close()
    assert len(a) > 0 and [bytes(f) for f in a] == [bytes(f) for f in b]
    assert [bytes(r) for r in ra] == [bytes(r) for r in rb]


def test_existing_message_and_json_paths_are_untouched_by_an_enabled_text_sink(D, fix, base_msgs):
    """a context with the text sink enabled hands out, through drain_msgs(oooi=True) and drain_json, bytes identical to one that
    never enabled it; both sinks may be on, each entry point consuming what it hands out"""
    x, gj, _ = fix
    dec = new_decoder(D, text=(TM.STD, TM.F_DATE | TM.F_FREQ))
    got = sum(play(dec, x, lambda: dec.drain_msgs(oooi=True)), [])
    dec.close()
    assert [bytes(m) + bytes(o) for m, o in got] == [bytes(m) + bytes(o) for m, o in base_msgs]
    plain, both = new_decoder(D), new_decoder(D, text=(TM.SV, 0))
    for d in (plain, both):
        d.enable_json(T0, "STN1", "acarsdec", "3.7")
    want = b"".join(play(plain, x, plain.drain_json))
    half = x.shape[1] // (2 * CHUNK) * CHUNK
    lines = b"".join(play(both, x[:, :half], both.drain_json))
    recs = sum(play(both, x[:, half:], both.drain_text), [])
    plain.close()
    both.close()
    assert want.startswith(lines) and 0 < lines.count(b"\n") < want.count(b"\n")
    assert lines.count(b"\n") + len(recs) == want.count(b"\n") == len(gj["sent"])
