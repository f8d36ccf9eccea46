"""The one host runtime behind the JSON and the text sink (csrc/sinks.cpp: AcgOutputs, outputs_fetch, outputs_reserve) where the two
sinks meet: both enabled in one context and drained in turn beside the message entry point, one of them re-enabled mid-run; and
a work space that grows inside a live context, from outputs_reserve's floor of 4096 records to a larger drain.  GPU box only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN
import text_model as TM

pytestmark = pytest.mark.gpu

T0 = (1792301725, 269667)
CHUNK = 4096
FLOOR = 4096                                                     # outputs_reserve's smallest work space, in records


@pytest.fixture(scope="module")
def D():
    from acarsdec_amd import decoder
    from acarsdec_amd import _capi as K
    assert K.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return decoder


def new_decoder(D, nch=3, json_station=None, text=False):
    dec = D.Decoder(nch, decim=8, ntaps=8, max_blocks=CHUNK // 1024, repair=True, bitlog=False)
    if json_station is not None:
        dec.enable_json(T0, json_station, "acarsdec", "3.7")
    if text:
        dec.enable_text(TM.STD, T0, date=True)
    return dec


def json_call(dec, K, cap):
    """one acg_drain_json through a buffer of cap bytes: (rc, lines)"""
    buf = C.create_string_buffer(cap)
    nb, nl = C.c_size_t(0), C.c_int(0)
    rc = dec.L.acg_drain_json(dec.ctx, buf, cap, C.byref(nb), C.byref(nl))
    blob = buf.raw[:nb.value]
    lines = [ln + b"\n" for ln in blob.split(b"\n")[:-1]]
    assert (blob == b"" or blob.endswith(b"\n")) and len(lines) == nl.value
    return rc, lines


def text_call(dec, K, cap, max_recs):
    """one acg_drain_text through a buffer of cap bytes and an offset table of max_recs records: (rc, records)"""
    buf = C.create_string_buffer(cap)
    offs = (C.c_uint * (max_recs + 1))()
    nb, nr = C.c_size_t(0), C.c_int(0)
    rc = dec.L.acg_drain_text(dec.ctx, buf, cap, C.byref(nb), offs, max_recs, C.byref(nr))
    blob = buf.raw[:nb.value]
    assert offs[0] == 0 and offs[nr.value] == nb.value
    return rc, [blob[offs[i]:offs[i + 1]] for i in range(nr.value)]


def drain_one_by_one(call, K):
    """the whole queue through `call`, whose buffer holds one record: ACG_EAGAIN until the last"""
    out = []
    while True:
        rc, recs = call()
        assert rc in (K.OK, K.EAGAIN) and len(recs) <= 1
        out += recs
        if rc == K.OK:
            return out


def json_chn(ln):
    return int(re.search(rb',"channel":(-?\d+),"freq":', ln).group(1))


def per_channel(recs, chn_of, nch):
    out = [[] for _ in range(nch)]
    for r in recs:
        out[chn_of(r)].append(r)
    return out


def test_both_sinks_in_one_context_take_turns(D):
    """One decoder with the JSON and the text sink (ACG_TEXT_STD) on, played call by call; after successive calls the consumer is
    drain_json, drain_text, drain_msgs(oooi=True) in rotation, the two sinks through a buffer of exactly one record bound.  What
    each entry point hands out equals, per channel and in order, what the same calls hand out in a twin context that has only
    that sink (and consumes the other calls' blocks as messages).  Half way the JSON sink is disabled and enabled again with
    another station_id: the later lines carry it, the text records never notice."""
    from acarsdec_amd import _capi as K
    x = np.load(os.path.join(GOLDEN, "msgjson_pcm16.npz"))["pcm"].astype(np.float32) / np.float32(32768.0)
    assert x.shape[0] == 3 and x.shape[1] % CHUNK == 0
    ncall = x.shape[1] // CHUNK
    swap = ncall // 2 // 3 * 3                                   # the call in front of which JSON is re-enabled (a JSON turn follows)
    both, only_json, only_text = new_decoder(D, json_station="STN1", text=True), new_decoder(D, json_station="STN1"), new_decoder(D, text=True)
    got = {(d, k): [] for d in ("both", "twin") for k in ("json", "text", "msgs")}
    early_lines = 0
    for i in range(ncall):
        if i == swap:
            early_lines = len(got["both", "json"])
            for dec in (both, only_json):
                dec.disable_json()
                dec.enable_json(T0, "STATION-2", "acarsdec", "3.7")
        for dec in (both, only_json, only_text):
            dec.demod_msk(x[:, i * CHUNK:(i + 1) * CHUNK])
        turn = ("json", "text", "msgs")[i % 3]
        if turn == "json":
            got["both", "json"] += drain_one_by_one(lambda: json_call(both, K, K.JSON_LINE_MAX), K)
            got["twin", "json"] += drain_one_by_one(lambda: json_call(only_json, K, K.JSON_LINE_MAX), K)
            only_text.drain_msgs()
        elif turn == "text":
            got["both", "text"] += drain_one_by_one(lambda: text_call(both, K, K.TEXT_REC_MAX, 1), K)
            got["twin", "text"] += drain_one_by_one(lambda: text_call(only_text, K, K.TEXT_REC_MAX, 1), K)
            only_json.drain_msgs()
        else:
            got["both", "msgs"] += [bytes(m) + bytes(o) for m, o in both.drain_msgs(oooi=True)]
            got["twin", "msgs"] += [bytes(m) + bytes(o) for m, o in only_json.drain_msgs(oooi=True)]
            only_text.drain_msgs()
    for dec in (both, only_json, only_text):
        assert dec.drain_msgs() == []                            # every block was consumed by exactly one entry point
        dec.close()
    assert all(len(got["both", k]) >= 1 for k in ("json", "text", "msgs")), {k: len(v) for k, v in got.items()}
    assert per_channel(got["both", "json"], json_chn, 3) == per_channel(got["twin", "json"], json_chn, 3)
    assert per_channel(got["both", "text"], TM.chn_of, 3) == per_channel(got["twin", "text"], TM.chn_of, 3)
    assert got["both", "msgs"] == got["twin", "msgs"]
    lines = got["both", "json"]
    assert 0 < early_lines < len(lines)
    assert all(b',"station_id":"STN1",' in ln for ln in lines[:early_lines]) and all(b',"station_id":"STATION-2",' in ln for ln in lines[early_lines:])


# ---- the work space grows inside a live context ------------------------------------------------------------------------------
WIDE_NCH = 2048


@pytest.fixture(scope="module")
def wide(D):
    """test_gpu_json_sink.py's synthetic wide traffic (test_level_text_equals_the_host_computed_record): the transmissions of one
    track at varied amplitude on every channel, two calls long; and how many blocks a context reports for it"""
    from acarsdec_amd import synth as S
    rng = np.random.default_rng(3)
    nsamp = 2 * CHUNK
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
    y = np.zeros((WIDE_NCH, nsamp), dtype=np.float32)
    for c in range(WIDE_NCH):
        t = int(rng.integers(200, 1200))
        while True:
            a = pieces[rng.integers(0, len(pieces))]
            if t + a.size >= nsamp - 200:
                break
            y[c, t:t + a.size] = a * np.float32(rng.uniform(0.01, 0.9))
            t += a.size + int(rng.integers(500, 1200))
    dec = new_decoder(D, nch=WIDE_NCH)
    play(dec, y)
    nblocks, _ = dec.drain_frames_raw(max_frames=1 << 15)
    dec.close()
    return y, nblocks


def play(dec, y):
    for s in range(0, y.shape[1], CHUNK):
        dec.demod_msk(y[:, s:s + CHUNK])


@pytest.mark.parametrize("sink", ["json", "text"])
def test_work_space_regrows_inside_a_live_context(D, wide, sink):
    """More than 4096 + 5 blocks queued.  A first drain through a buffer of five record bounds creates the work space at its floor
    of 4096 records and says ACG_EAGAIN; one full-size drain then takes the rest, more than the floor, so the work space is
    freed and allocated again between two passes of one sink.  The two calls' records are, per channel and in order, those of
    a fresh context's single full drain (whose work space is created at the full size)."""
    from acarsdec_amd import _capi as K
    y, nblocks = wide
    print("blocks queued:", nblocks)
    assert nblocks > FLOOR + 5
    kw = dict(json_station="STN1") if sink == "json" else dict(text=True)
    if sink == "json":
        call, chn_of, bound = (lambda dec, nrec: json_call(dec, K, nrec * K.JSON_LINE_MAX)), json_chn, K.JSON_LINE_MAX
    else:
        call, chn_of, bound = (lambda dec, nrec: text_call(dec, K, nrec * K.TEXT_REC_MAX, nblocks)), TM.chn_of, K.TEXT_REC_MAX
    grown, fresh = new_decoder(D, nch=WIDE_NCH, **kw), new_decoder(D, nch=WIDE_NCH, **kw)
    for dec in (grown, fresh):
        play(dec, y)
    rc1, first = call(grown, 5)
    rc2, rest = call(grown, nblocks)
    rc3, whole = call(fresh, nblocks)
    assert call(grown, 1) == (K.OK, []) and call(fresh, 1) == (K.OK, [])
    grown.close()
    fresh.close()
    assert (rc1, rc2, rc3) == (K.EAGAIN, K.OK, K.OK)
    assert len(first) <= 5 and len(first) + len(rest) == len(whole) > FLOOR       # (a block the repair dropped yields no record)
    assert all(0 < len(r) <= bound for r in whole)
    assert per_channel(first + rest, chn_of, WIDE_NCH) == per_channel(whole, chn_of, WIDE_NCH)
