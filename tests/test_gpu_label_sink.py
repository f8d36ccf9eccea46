"""The batch sink's filters and label decoding on the device (label.hip) against the reference program's JSON for the label
fixture, against the Python model on random records, and the drain / collect contract with a filter set.  GPU box only."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
import label_model as M

pytestmark = pytest.mark.gpu

VARIANTS = ("none", "A", "e", "b", "Aeb")


@pytest.fixture(scope="module")
def D():
    from acarsdec_amd import decoder
    from acarsdec_amd import _capi as K
    assert K.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return decoder


@pytest.fixture(scope="module")
def fix():
    pcm = np.load(os.path.join(GOLDEN, "labels_pcm16.npz"))["pcm"]
    with open(os.path.join(GOLDEN, "labels_golden.json")) as f:
        return pcm, json.load(f)


def filter_kw(fixture, variant):
    args = fixture["variants"][variant]["args"]
    return dict(downlink_only="-A" in args, skip_empty="-e" in args, labels=fixture["label_list"] if "-b" in args else None)


def cstr(b):
    return bytes(b).split(b"\0")[0].decode("latin1")


def json_view(m, o, D):
    """(acg_msg, acg_oooi) as buildjson prints it (output.c:227-324 without timestamp, station, frequency, app)"""
    down = m.down not in (b"\x00", 0)
    j = dict(channel=int(m.chn), level="%2.1f" % m.lvl, error=int(m.err), mode=m.mode.decode("latin1"), label=m.label.decode("latin1"))
    if m.bid not in (b"\x00", 0):
        j["block_id"] = m.bid.decode("latin1")
        j["ack"] = False if m.ack == b"!" else m.ack.decode("latin1")
        j["tail"] = m.addr.decode("latin1")
        if down:
            j["flight"] = m.fid.decode("latin1")
            j["msgno"] = m.no.decode("latin1")
    if m.txt[0]:
        j["text"] = cstr(m.txt[: m.txt_len])
    if m.be == b"\x17":
        j["end"] = True
    j.update(D.oooi_json(m, o))
    return j


def lbl2(m):
    """the two label bytes of a record (ctypes reads char arrays only up to their NUL)"""
    return (m.label + b"\0\0")[:2]


def golden_view(j, chn):
    j = dict(j, channel=chn)
    j["level"] = "%2.1f" % j["level"]
    return j


def play(dec, x, chunk, nch, per_drain):
    out = []
    for s in range(0, x.size, chunk):
        dec.demod_msk(np.tile(x[s:s + chunk], (nch, 1)))
        out.append(per_drain(s // chunk))
    return out


def test_filtered_oooi_drain_matches_reference_json(D, fix):
    """Every filter variant: the fixture on three channels through demodulator, framing, repair, split and label pass; what
    drain_msgs(oooi=True) hands out equals the reference's JSON field for field, OOOI keys included."""
    pcm, g = fix
    x = pcm.astype(np.float32) / 32768.0
    chunk, nch = 4096, 3
    x = np.concatenate([x, np.zeros((-x.size) % chunk, dtype=np.float32)])
    for v in VARIANTS:
        dec = D.Decoder(nch, decim=8, ntaps=8, max_blocks=chunk // 1024, repair=True, bitlog=False)
        dec.set_msg_filter(**filter_kw(g, v))
        got = sum(play(dec, x, chunk, nch, lambda k: dec.drain_msgs(oooi=True)), [])
        want = g["variants"][v]["json"]
        assert len(got) == nch * len(want), v
        for c in range(nch):
            mine = [json_view(m, o, D) for m, o in got if m.chn == c]
            assert mine == [golden_view(j, c) for j in want], (v, c)
        for m, o in got:
            assert bytes(o)[36:] == b"\0" * 4 and (o.decoded != b"\x00" or bytes(o) == bytes(40))
        dec.close()


def test_filter_changed_between_drains(D, fix):
    """The filter set before a drain is the one that drain applies: drains with the variants in turn hand out, drain by drain,
    what the unfiltered drains hand out filtered by the model with that drain's variant; the plain drain obeys the filter too."""
    pcm, g = fix
    x = pcm.astype(np.float32) / 32768.0
    chunk, nch = 8192, 3
    x = np.concatenate([x, np.zeros((-x.size) % chunk, dtype=np.float32)])
    ref = D.Decoder(nch, decim=8, ntaps=8, max_blocks=chunk // 1024, repair=True, bitlog=False)
    base = play(ref, x, chunk, nch, lambda k: ref.drain_msgs(oooi=True))
    assert sum(map(len, base)) == nch * len(g["sent"])
    for plain in (False, True):
        dec = D.Decoder(nch, decim=8, ntaps=8, max_blocks=chunk // 1024, repair=True, bitlog=False)

        def drain(k):
            kw = filter_kw(g, VARIANTS[k % len(VARIANTS)])
            dec.set_msg_filter(**kw) if k % 6 != 5 else dec.set_msg_filter()          # (and "no filter" now and then)
            return [(m, None) for m in dec.drain_msgs()] if plain else dec.drain_msgs(oooi=True)
        got = play(dec, x, chunk, nch, drain)
        for k, (mine, theirs) in enumerate(zip(got, base)):
            kw = filter_kw(g, VARIANTS[k % len(VARIANTS)]) if k % 6 != 5 else {}
            labels = M.parse_label_filter(kw.get("labels"))
            want = [(m, o) for m, o in theirs
                    if M.keep(m.down not in (b"\x00", 0), lbl2(m), bytes(m.txt), m.txt_len,
                              downlink_only=kw.get("downlink_only", False), skip_empty=kw.get("skip_empty", False), labels=labels)]
            assert [bytes(m) for m, _ in mine] == [bytes(m) for m, _ in want], k
            if not plain:
                assert [bytes(o) for _, o in mine] == [bytes(o) for _, o in want], k
        dec.close()
    ref.close()


def random_records(rng, n, K):
    """n acg_msg records for the lab self-test: labels of the table (texts built to pass their checks, then mutated and cut
    short), random labels with NUL / DEL bytes, short texts, embedded NULs, garbage behind txt_len"""
    recs = np.zeros((n, C.sizeof(K.Msg)), dtype=np.uint8)
    o_len, o_lbl, o_down, o_txt = K.Msg.txt_len.offset, K.Msg.label.offset, K.Msg.down.offset, K.Msg.txt.offset
    labels = list(M.TABLE)
    alphabet = np.frombuffer(b"ABCDEFKLQRSTUVWXYZ0123456789,/ \n\0", dtype=np.uint8)
    t26 = b"VER/077XX\nSCH/AB12/KJFK.EGLL\nETA/1234ZZ"
    for i in range(n):
        r = recs[i]
        kind = rng.integers(0, 10)
        if kind < 7:
            lbl = labels[rng.integers(0, len(labels))].encode()
        else:
            lbl = bytes([rng.choice([0, 0x7F, 0x31, 0x51, 0x52, 0x32]), rng.choice([0, 0x7F, 0x64, 0x31, 0x42, 0x36])])
        r[o_lbl:o_lbl + 2] = np.frombuffer(lbl, dtype=np.uint8)
        r[o_lbl + 2] = rng.integers(0, 256)                     # (not read)
        r[o_down] = rng.integers(0, 2) * rng.integers(1, 256)
        txt = alphabet[rng.integers(0, len(alphabet), 242)].copy()
        spec = M.TABLE.get(lbl.decode("latin1"))
        if spec == "26":
            txt[:len(t26)] = np.frombuffer(t26, dtype=np.uint8)
        elif spec is not None:
            sh = 2 if (spec[2] and rng.integers(0, 2)) else 0
            if sh:
                txt[:2] = np.frombuffer(spec[2], dtype=np.uint8)
            elif txt[0] == ord("0"):
                txt[0] = ord("K")
            for off, alts in spec[0]:
                a = alts[rng.integers(0, len(alts))]
                txt[sh + off: sh + off + len(a)] = np.frombuffer(a, dtype=np.uint8)
        for _ in range(rng.integers(0, 3)):                     # mutations: some checks fail, some fields hold NULs
            txt[rng.integers(0, 60)] = alphabet[rng.integers(0, len(alphabet))]
        r[o_txt:o_txt + 242] = txt
        tl = int(rng.choice([rng.integers(0, 8), rng.integers(0, 64), rng.integers(0, 243)]))
        if rng.integers(0, 50) == 0:
            tl = int(rng.choice([-5, 300]))                     # clamped to 0 .. 242
        r[o_len:o_len + 4] = np.frombuffer(np.int32(tl).tobytes(), dtype=np.uint8)
    return recs


def test_device_decoder_and_filters_match_the_model_on_random_records(D):
    from acarsdec_amd import _capi as K
    L = K.load()
    rng = np.random.default_rng(11)
    n = 100000
    recs = random_records(rng, n, K)
    o_len, o_lbl, o_down, o_txt = K.Msg.txt_len.offset, K.Msg.label.offset, K.Msg.down.offset, K.Msg.txt.offset
    model = []
    for r in recs:
        tl = int(np.frombuffer(r[o_len:o_len + 4].tobytes(), dtype=np.int32)[0])
        txt = r[o_txt:o_txt + 242].tobytes()
        dec, fields = M.decode(r[o_lbl:o_lbl + 2].tobytes(), txt, tl)
        model.append((r[o_down] != 0, r[o_lbl:o_lbl + 2].tobytes(), txt, tl, M.oooi_bytes(dec, fields)))
    assert sum(1 for m in model if m[4][35]) > n // 10                       # the success paths are well exercised
    filters = [dict(), dict(downlink_only=True), dict(skip_empty=True), dict(labels="Q1:44:26:RB:1:Qd:2:TOOLONG::"),
               dict(downlink_only=True, skip_empty=True, labels=["QT", "8E", "d", "10"])]
    buf = (K.Msg * n).from_buffer_copy(recs.tobytes())
    for kw in filters:
        f = D.make_msg_filter(**kw) if kw else None
        keep = np.zeros(n, dtype=np.uint8)
        oo = (K.Oooi * n)()
        rc = L.acg_selftest_msg_labels(buf, n, C.byref(f) if f is not None else None, keep.ctypes.data, oo)
        assert rc == K.OK, (kw, rc)
        labels = M.parse_label_filter(kw["labels"]) if isinstance(kw.get("labels"), str) else \
            [l.encode() for l in kw.get("labels", [])]
        want_keep = np.array([M.keep(d, l, t, tl, downlink_only=kw.get("downlink_only", False), skip_empty=kw.get("skip_empty", False),
                                     labels=labels) for d, l, t, tl, _ in model], dtype=np.uint8)
        assert np.array_equal(keep, want_keep), kw
        got = np.frombuffer(bytes(oo), dtype=np.uint8).reshape(n, 40)
        want = np.frombuffer(b"".join(m[4] if k else bytes(40) for m, k in zip(model, want_keep)), dtype=np.uint8).reshape(n, 40)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (kw, bad[:5], [recs[i].tobytes() for i in bad[:2]])


def synth_label_traffic(rng, frames_audio, nch, nsamp):
    x = np.zeros((nch, nsamp), dtype=np.float32)
    for c in range(nch):
        t = int(rng.integers(200, 1500))
        while True:
            a = frames_audio[rng.integers(0, len(frames_audio))]
            if t + a.size >= nsamp:
                break
            x[c, t:t + a.size] = a
            t += a.size + int(rng.integers(400, 1200))
    return x


def test_collect_contract_with_filter_and_oooi_at_1024_channels(D, fix):
    """1024 channels of label traffic, collected with lag 1 after every call: the filtered collect_msgs(oooi=True) equals the
    unfiltered acg_collect_msgs filtered on the host by the model; without a filter the _oooi variant hands out byte-identical
    records; a small buffer gives ACG_EAGAIN and loses nothing."""
    from acarsdec_amd import _capi as K, synth as S
    pcm, g = fix
    rng = np.random.default_rng(5)
    frames = []
    for s in g["sent"]:
        txt = bytes.fromhex(s["text"])
        full = (b"M01AXY0123" + txt) if (s["down"] and txt) else txt
        fr = S.acars_frame(text=full, mode=b"2", addr=b".N12345", ack=b"\x15", label=bytes.fromhex(s["label"]), bid=s["bid"].encode())
        frames.append((0.25 * S.msk_audio(S.frame_bits(fr), phase0=float(rng.uniform(0, 6.28)))).astype(np.float32))
    nch, chunk, ncall = 1024, 4096, 4
    x = synth_label_traffic(rng, frames, nch, chunk * ncall)
    kw = filter_kw(g, "b")
    kw["skip_empty"] = True
    decs = [D.Decoder(nch, decim=8, ntaps=8, max_blocks=chunk // 1024, repair=True, bitlog=False, max_lag=1) for _ in range(4)]
    plain, oooi_nf, filt, small = decs
    filt.set_msg_filter(**kw)
    small.set_msg_filter(**kw)
    got = {k: [] for k in range(4)}
    codes = set()
    for k in range(ncall + 1):
        if k < ncall:
            for d in decs:
                d.demod_msk(x[:, k * chunk:(k + 1) * chunk])
        lag = 1 if k < ncall else 0
        got[0] += plain.collect_msgs(lag=lag)
        got[1] += oooi_nf.collect_msgs(lag=lag, oooi=True)
        got[2] += filt.collect_msgs(lag=lag, oooi=True)
        while True:                                             # the raw C call through a 5-record buffer
            mb, ob, n = (K.Msg * 5)(), (K.Oooi * 5)(), C.c_int(0)
            rc = small.L.acg_collect_msgs_oooi(small.ctx, lag, mb, ob, 5, C.byref(n))
            codes.add(rc)
            assert rc in (K.OK, K.EAGAIN) and 0 <= n.value <= 5
            got[3] += [(K.Msg.from_buffer_copy(mb[i]), K.Oooi.from_buffer_copy(ob[i])) for i in range(n.value)]
            if rc == K.OK:
                break
    assert len(got[0]) > nch
    assert [bytes(m) for m in got[0]] == [bytes(m) for m, _ in got[1]]
    labels = M.parse_label_filter(kw["labels"])
    want = [(m, o) for m, o in got[1] if M.keep(m.down not in (b"\x00", 0), lbl2(m), bytes(m.txt), m.txt_len,
                                                 skip_empty=True, labels=labels)]
    assert 0 < len(want) < len(got[1])
    assert [bytes(m) + bytes(o) for m, o in got[2]] == [bytes(m) + bytes(o) for m, o in want]
    for m, o in got[1]:
        dec, fields = M.decode(lbl2(m), bytes(m.txt), m.txt_len)
        assert bytes(o) == M.oooi_bytes(dec, fields)
    key = lambda p: (bytes(p[0]), bytes(p[1]))
    assert K.EAGAIN in codes and sorted(map(key, got[3])) == sorted(map(key, want))
    for d in decs:
        d.close()
