"""The per-channel statistics table on the device (acg_stats_enable / acg_stats_read; csrc/stats.hip, the outcome byte of
csrc/blk.hip) against the reference's own -v counts (tests/golden/stats_golden.json) and
the model that tests/test_stats_model.py pins to them (tests/stats_model.py).  All comparisons are exact.

  1. the golden's channels through process_dm and drain_msgs: every field is the reference's count and the model's;
  2. the whole repair corpus (1024 channels, five calls of 8192 samples) through collect_msgs(lag=1), through buffers of 7 messages
     (most calls say ACG_EAGAIN) and through collect_frames: the model on every channel, the same block-level fields in all
     three, both identities, and message records that do not change when statistics are switched on;
  3. the JSON fixture under every filter variant: the filter fields, unchanged JSON / text output, a sink call cut short by `cap`;
  4. a ring lapped on purpose: lost_blocks is the figure of acg_last_error, the channels' blocks are what was consumed;
  5. the lifecycle; 6. two runs give the same bytes."""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN
import repair_corpus as RC
import stats_model as SM
from test_stats_model import msgjson_rows

pytestmark = pytest.mark.gpu

REF_FIELDS = tuple(k for k in SM.BLOCK_FIELDS if k != "kept")        # the block-level lines of the reference ("kept" is no line)
T0 = (1792301725, 269667)
CHUNK = 4096


@pytest.fixture(scope="module")
def D():
    from acarsdec_amd import decoder
    from acarsdec_amd import _capi as K
    assert K.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return decoder


@functools.lru_cache(maxsize=1)
def golden():
    with open(os.path.join(GOLDEN, "stats_golden.json")) as f:
        g = json.load(f)
    pcm, sha = SM.golden_pcm(g)
    assert sha == g["pcm_sha256"]
    return g, pcm.astype(np.float32) / np.float32(32768.0)


@functools.lru_cache(maxsize=1)
def msgjson():
    pcm = np.load(os.path.join(GOLDEN, "msgjson_pcm16.npz"))["pcm"]
    with open(os.path.join(GOLDEN, "msgjson_golden.json")) as f:
        g = json.load(f)
    return g, pcm.astype(np.float32) / np.float32(32768.0)


@functools.lru_cache(maxsize=1)
def corpus_model():
    items, _ = RC.corpus()
    rows = SM.corpus_rows(items)
    return RC.audio(items), [rows.get(c, SM.new_row()) for c in range(RC.NCH)]


def rows_of(st):
    return [{k: int(st[k][c]) for k in SM.COUNTERS + ("last_end_sample",)} for c in range(len(st))]


def play(dec, x, call, after_call=None):
    out = []
    for k in range(0, x.shape[1], call):
        dec.demod_msk(x[:, k:k + call])
        if after_call:
            out += after_call()
    return out


def check_levels_and_stamps(D, st, recs):
    """lvl_min / lvl_max / last_end_sample against the kept records the device handed out itself: the level of a record is
    acars.c:351's float of the ratio, a monotonic function of it"""
    lo, hi = D.stats_level_db(st)
    per = {}
    for r in recs:
        per.setdefault(int(r.chn), []).append(r)
    for c in range(len(st)):
        rs = per.get(c, [])
        assert int(st["last_end_sample"][c]) == max([int(r.end_sample) for r in rs], default=-1), c
        if rs:
            assert (lo[c], hi[c]) == (min(np.float32(r.lvl) for r in rs), max(np.float32(r.lvl) for r in rs)), c
            assert 0 < st["lvl_min"][c] <= st["lvl_max"][c]
        else:
            assert st["lvl_min"][c] == 0 and st["lvl_max"][c] == 0


# ---- 1 ----------------------------------------------------------------------------------------------------------------------
def test_golden_channels_count_what_the_reference_prints(D):
    g, x = golden()
    dec = D.Decoder(x.shape[0], decim=8, ntaps=8, max_blocks=8, repair=True, bitlog=False)
    dec.enable_stats()
    msgs = play(dec, x, RC.CALL, dec.drain_msgs)
    st, lost = dec.stats()
    dec.close()
    model = SM.golden_model_rows(g)
    assert lost == 0 and len(st) == len(g["rows"])
    for c, (have, ref, m) in enumerate(zip(rows_of(st), g["rows"], model)):
        assert {k: have[k] for k in REF_FIELDS} == {k: ref["counts"][k] for k in REF_FIELDS}, (c, ref["what"])
        assert {k: have[k] for k in SM.COUNTERS} == {k: m[k] for k in SM.COUNTERS}, (c, ref["what"])
        SM.check_identities(have)
    assert sum(int(v) for v in st["delivered"]) == len(msgs)
    check_levels_and_stamps(D, st, msgs)


# ---- 2, 6 -------------------------------------------------------------------------------------------------------------------
def corpus_decoder(D, stats=True, **kw):
    dec = D.Decoder(RC.NCH, decim=8, ntaps=8, max_blocks=8, repair=True, bitlog=False, max_lag=1, **kw)
    if stats:
        dec.enable_stats()
    return dec


@functools.lru_cache(maxsize=4)
def corpus_run(how, stats=True, again=0):
    """(records handed out, table | None, how many C calls said ACG_EAGAIN)"""
    from acarsdec_amd import decoder as D
    from acarsdec_amd import _capi as K
    x, _ = corpus_model()
    dec = corpus_decoder(D, stats)
    eagain = [0]

    def small(fn, *lead):
        out = []
        while True:
            n = C.c_int(0)
            buf = dec._msg_buf(7)
            rc = dec._chk(fn(dec.ctx, *lead, buf, 7, C.byref(n)), allow=(K.EAGAIN,))
            out += [K.Msg.from_buffer_copy(buf[i]) for i in range(n.value)]
            eagain[0] += rc == K.EAGAIN
            if rc == K.OK:
                return out

    def frames():
        n, buf, more = dec._frames_call(dec.L.acg_collect_frames, 4096, 1)
        assert not more
        return [K.Frame.from_buffer_copy(buf[i]) for i in range(n)]
    if how == "msgs":
        got = play(dec, x, RC.CALL, lambda: dec.collect_msgs(lag=1)) + dec.drain_msgs()
    elif how == "small":
        got = play(dec, x, RC.CALL, lambda: small(dec.L.acg_collect_msgs, 1)) + small(dec.L.acg_drain_msgs)
    else:
        got = play(dec, x, RC.CALL, frames) + dec.drain_frames()
    st = dec.stats() if stats else None
    dec.close()
    return got, st, eagain[0]


@pytest.mark.parametrize("how", ["msgs", "small", "frames"])
def test_corpus_equals_the_model_on_every_channel(D, how):
    got, (st, lost), eagain = corpus_run(how)
    _, model = corpus_model()
    have = rows_of(st)
    assert lost == 0 and len(got) >= 1500
    bad = [c for c in range(RC.NCH) if any(have[c][k] != model[c][k] for k in SM.COUNTERS)]
    assert not bad, (how, len(bad), bad[:5], have[bad[0]], model[bad[0]])
    for r in have:
        SM.check_identities(r, msgs_only=how != "frames")
    assert sum(r["delivered"] for r in have) == len(got)               # (frames: delivered moves with kept, the filter fields do not)
    assert all(r["uplink_dropped"] == r["label_dropped"] == r["empty_dropped"] == 0 for r in have)
    if how == "small":
        assert eagain >= 200                                           # most calls handed out 7 records and said "again"
    check_levels_and_stamps(D, st, got)


def test_corpus_tables_are_the_same_through_every_entry_point():
    a, b, c = (corpus_run(h)[1][0] for h in ("msgs", "small", "frames"))
    assert a.tobytes() == b.tobytes() == c.tobytes()


def test_message_records_do_not_change_when_statistics_are_on():
    on, off = corpus_run("msgs")[0], corpus_run("msgs", stats=False)[0]
    assert len(on) == len(off) >= 1500 and all(bytes(x) == bytes(y) for x, y in zip(on, off))


def test_two_runs_give_the_same_bytes():
    a, b = corpus_run("msgs")[1][0], corpus_run("msgs", again=1)[1][0]
    assert a.tobytes() == b.tobytes() and int(a["kept"].sum()) >= 1500 and float(a["lvl_max"].max()) > 0


# ---- 3 ----------------------------------------------------------------------------------------------------------------------
def filter_kw(g, variant):
    args = g["variants"][variant]["args"]
    return dict(downlink_only="-A" in args, skip_empty="-e" in args, labels=g["label_list"] if "-b" in args else None)


def sink_decoder(D, g, variant, stats, text=False):
    dec = D.Decoder(g["nch"], decim=8, ntaps=8, max_blocks=CHUNK // 1024, repair=True, bitlog=False)
    if text:
        dec.enable_text("std", T0)
    else:
        dec.enable_json(T0, g["station"], "acarsdec", "3.7")
    dec.set_msg_filter(**filter_kw(g, variant))
    if stats:
        dec.enable_stats()
    return dec


@pytest.mark.parametrize("variant", ["none", "A", "e", "b", "Aeb"])
def test_filter_fields_under_every_variant_and_unchanged_sink_output(D, variant):
    g, x = msgjson()
    out = {}
    for stats in (True, False):
        dec = sink_decoder(D, g, variant, stats)
        out[stats] = b"".join(play(dec, x, CHUNK, lambda: [dec.drain_json()]))
        if stats:
            st, lost = dec.stats()
        dec.close()
    assert out[True] == out[False] and out[True].count(b"\n") == len(g["variants"][variant]["lines"])
    model = msgjson_rows(g, variant)
    have = rows_of(st)
    for c in range(g["nch"]):
        assert {k: have[c][k] for k in SM.BLOCK_FIELDS + SM.FILTER_FIELDS} == {k: model[c][k] for k in SM.BLOCK_FIELDS + SM.FILTER_FIELDS}, (variant, c)
        SM.check_identities(have[c])
    assert lost == 0 and sum(r["delivered"] for r in have) == out[True].count(b"\n")


def test_text_sink_output_is_unchanged_and_counts_the_same(D):
    g, x = msgjson()
    out, tab = {}, None
    for stats in (True, False):
        dec = sink_decoder(D, g, "Aeb", stats, text=True)
        out[stats] = play(dec, x, CHUNK, dec.drain_text)
        if stats:
            tab = dec.stats()[0]
        dec.close()
    assert out[True] == out[False] and len(out[True]) == len(g["variants"]["Aeb"]["lines"]) == int(tab["delivered"].sum())
    model = msgjson_rows(g, "Aeb")
    assert [int(v) for v in tab["uplink_dropped"]] == [r["uplink_dropped"] for r in model]
    assert [int(v) for v in tab["empty_dropped"]] == [r["empty_dropped"] for r in model]


def test_a_sink_call_cut_short_by_cap_counts_only_what_it_consumed(D):
    from acarsdec_amd import _capi as K
    g, x = msgjson()
    dec = sink_decoder(D, g, "A", True)
    ncall = min(6, dec.max_lag + 1)
    play(dec, x[:, :ncall * CHUNK], CHUNK)
    buf = C.create_string_buffer(5 * K.JSON_LINE_MAX)
    nb, nl = C.c_size_t(0), C.c_int(0)
    rc = dec.L.acg_drain_json(dec.ctx, buf, 5 * K.JSON_LINE_MAX, C.byref(nb), C.byref(nl))
    st, _ = dec.stats()
    assert rc == K.EAGAIN and int(st["blocks"].sum()) == 5             # five blocks fit, five were consumed
    assert int(st["delivered"].sum()) == nl.value == buf.raw[:nb.value].count(b"\n")
    assert int(st["kept"].sum()) == int(st["uplink_dropped"].sum()) + nl.value
    rest = dec.drain_json()
    st2, _ = dec.stats()
    assert dec.drain_json() == b"" and dec.stats()[0].tobytes() == st2.tobytes()      # a sink call that consumes nothing counts nothing
    twin = sink_decoder(D, g, "A", True)
    play(twin, x[:, :ncall * CHUNK], CHUNK)
    whole = twin.drain_json()
    st3, _ = twin.stats()
    dec.close()
    twin.close()
    assert sorted((buf.raw[:nb.value] + rest).split(b"\n")) == sorted(whole.split(b"\n"))
    assert st2.tobytes() == st3.tobytes() and int(st2["blocks"].sum()) > 5


# ---- 4 ----------------------------------------------------------------------------------------------------------------------
def test_lapped_ring_goes_to_lost_blocks(D):
    """an ordinary ACG_EOVERFLOW: a context whose block queue holds two calls of 1024 samples, the whole JSON fixture played
    without a collect"""
    from acarsdec_amd import _capi as K
    g, x = msgjson()
    dec = D.Decoder(g["nch"], decim=8, ntaps=8, max_blocks=1, repair=True, bitlog=False, max_lag=1)
    dec.enable_stats()
    ring = int(dec.L.acg_lab_block_ring_size(dec.ctx))
    assert ring < len(g["sent"])
    play(dec, x, 1024)
    fr = (K.Frame * 4096)()
    n = C.c_int(0)
    rc = dec.L.acg_drain_frames(dec.ctx, fr, 4096, C.byref(n))
    said = int(re.search(rb"the (\d+) oldest blocks are lost", dec.L.acg_last_error(dec.ctx)).group(1))
    st, lost = dec.stats()
    dec.close()
    assert rc == K.EOVERFLOW and lost == said == len(g["sent"]) - ring
    assert int(st["blocks"].sum()) == ring and int(st["delivered"].sum()) == n.value == int(st["kept"].sum())
    for r in rows_of(st):
        SM.check_identities(r, msgs_only=False)


# ---- 5 ----------------------------------------------------------------------------------------------------------------------
def test_lifecycle(D):
    from acarsdec_amd import _capi as K
    g, x = msgjson()
    plain = D.Decoder(3, decim=8, ntaps=8, max_blocks=4, repair=False, bitlog=False)
    assert plain.L.acg_stats_enable(plain.ctx, 1) == K.ESTATE          # no ACG_F_REPAIR
    plain.close()
    dec = D.Decoder(3, decim=8, ntaps=8, max_blocks=4, repair=True, bitlog=False)
    buf = np.zeros(3, dtype=K.CHAN_STATS_DTYPE)
    lost = C.c_ulonglong(7)
    read = lambda ch0, n: dec.L.acg_stats_read(dec.ctx, ch0, n, buf.ctypes.data, C.byref(lost))
    assert read(0, 3) == K.ESTATE                                      # off
    dec.enable_stats()
    for ch0, n in ((-1, 1), (0, 4), (3, 1), (2, 2), (0, -1)):
        assert read(ch0, n) == K.EINVAL, (ch0, n)
    assert read(3, 0) == K.OK and read(1, 2) == K.OK
    zero = np.zeros(3, dtype=K.CHAN_STATS_DTYPE)
    zero["last_end_sample"] = -1
    assert dec.stats()[0].tobytes() == zero.tobytes()                  # enable zeroes
    play(dec, x[:, :4 * CHUNK], CHUNK, dec.drain_msgs)
    first, _ = dec.stats()
    assert int(first["kept"].sum()) > 5
    part, _ = dec.stats(1, 2)
    assert part.tobytes() == first[1:].tobytes()
    dec.enable_stats()                                                 # on again: zeroes
    assert dec.stats()[0].tobytes() == zero.tobytes()
    play(dec, x[:, 4 * CHUNK:6 * CHUNK], CHUNK, dec.drain_msgs)
    assert int(dec.stats()[0]["blocks"].sum()) > 0
    dec.reset()                                                        # zeroes the table and keeps the switch
    assert dec.stats()[0].tobytes() == zero.tobytes()
    play(dec, x[:, :4 * CHUNK], CHUNK, dec.drain_msgs)
    assert dec.stats()[0].tobytes() == first.tobytes()
    dec.disable_stats()
    assert read(0, 3) == K.ESTATE
    play(dec, x[:, 4 * CHUNK:5 * CHUNK], CHUNK, dec.drain_msgs)       # off: the entry points go on as before
    dec.close()
