"""The reassembly table inside a working context: a Decoder fed 12.5 kHz audio through demod_msk, with everything on that lies
between the table and the host -- channel numbers (ctx->d_chnum in the time key and the completed record), the label pass and its
index map in fetch_msgs (oooi, the flight table, -A / -b / -e, of which -e must NOT keep a block from the table), takes smaller than
the queue, the outputs' entry points, and stream counters that straddle 2^32 samples.

The audio has three channels; rows 0 and 2 are identical sample for sample, so every block on them ends at the same end_sample on
two channels and the order rule (end_sample, chn) alone -- on the number handed out -- decides which copy is the DUPLICATE.  The
reference of every case is reasm_model.Table over the CPU oracle's messages, renumbered by the channel map."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reasm_cases as RC  # noqa: E402
import reasm_model as RM  # noqa: E402
import reasm_table_model as T  # noqa: E402
from test_gpu_reasm import done_tuple, oracle_messages  # noqa: E402

pytestmark = pytest.mark.gpu

T0 = T.T0
NSAMP = 32768
FEEDS = ((4096, 1), (16384, 0))                       # (samples per demod_msk call, lag of the collect behind it)


@pytest.fixture(scope="module")
def D():
    from acarsdec_amd import decoder
    from acarsdec_amd import _capi as K
    assert K.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return decoder


def tied_audio():
    """[3, NSAMP] audio.  Rows 0 and 2 (the same samples): a 4-block downlink chain whose second block has an empty text (its body
    is the message number and the flight id only).  Row 1, at the same time: a 2-block chain under label 5Z, an uplink chain over
    the wrap of mode '2' (Y, Z, A) and a lone uplink."""
    from acarsdec_amd import synth as S
    rng = np.random.default_rng(33)
    shared = [(b"M01A", b"3", True, b"H1", b".N777AB", True), (b"M01B", b"3", True, b"H1", b".N777AB", False), (b"M01C", b"3", True, b"H1", b".N777AB", True),
              (b"M01D", b"3", False, b"H1", b".N777AB", True)]
    row1 = [(b"Z01A", b"4", True, b"5Z", b".N555ZZ", True), (None, b"Y", True, b"H1", b".UPLINK", True), (b"Z01B", b"4", False, b"5Z", b".N555ZZ", True),
            (None, b"Z", True, b"H1", b".UPLINK", True), (None, b"C", False, b"H1", b".LONELY", True), (None, b"A", False, b"H1", b".UPLINK", True)]
    x = np.zeros((3, NSAMP), dtype=np.float32)
    for rows, plan, pos in (((0, 2), shared, 1500), ((1,), row1, 2600)):
        for no, bid, etb, label, addr, body in plan:
            text = (no + b"XY0042" if no else b"") + (S.random_text(rng, 20, 50) if body else b"")
            fr = S.acars_frame(text=text, addr=addr, label=label, bid=bid, etb=etb)
            a = S.msk_audio(S.frame_bits(fr), phase0=float(rng.uniform(0, 2 * np.pi)))
            assert pos + a.size + 500 < NSAMP
            for r in rows:
                x[r, pos:pos + a.size] = 0.06 * a
            pos += a.size + int(rng.integers(1200, 2400))
    return x, 2 * len(shared) + len(row1)


@pytest.fixture(scope="module")
def signal():
    """(audio, the oracle's messages): computed once, shared, never changed"""
    x, nframes = tied_audio()
    assert np.array_equal(x[0], x[2]) and not np.array_equal(x[0], x[1])
    orc = oracle_messages(x)
    assert len(orc) == nframes
    on = {c: [m for m in orc if m.chn == c] for c in range(3)}
    # the premise of the ties: every block of rows 0 and 2 has the same end_sample and end_bit on both channels
    assert [(m.end_sample, m.end_bit, m.no) for m in on[0]] == [(m.end_sample, m.end_bit, m.no) for m in on[2]] and len(on[0]) == 4
    assert [m.txt_len == 0 for m in on[0]] == [False, True, False, False] and on[0][1].no[:4] == b"M01B"
    assert sorted(RM.cstr(m.label) for m in on[1]) == [b"5Z", b"5Z", b"H1", b"H1", b"H1", b"H1"]
    assert len({m.end_sample for m in on[0]} | {m.end_sample for m in on[1]}) == 10      # ... and nothing else ties
    return x, orc


def model(orc, chmap=(0, 1, 2), keep=None, t0_us=T.T0_US):
    """reasm_model.Table over the oracle's messages numbered by chmap, in the rule's order: ({(chn, end_bit): status}, completed
    tuples).  A collect hands out whole demod_msk calls, blocks of a later call end later and tied blocks end in the same call:
    fed call by call in (end_sample, chn) order is fed in (end_sample, chn) order.  keep(m): what -A / -b let through."""
    ms = []
    for m in orc:
        c = types.SimpleNamespace(**vars(m))
        c.chn = chmap[m.chn]
        ms.append(c)
    ms.sort(key=lambda m: (m.end_sample, m.chn))
    t = RM.Table(t0_us)
    want = {(m.chn, m.end_bit): (t.add(m) if keep is None or keep(m) else RM.SKIPPED) for m in ms}
    return want, RC.completed_tuples(t.done)


def c_calls(dec, drain, max_msgs, oooi, lag=0):
    """acg_collect_msgs_reasm / acg_drain_msgs_reasm until the C side says there is no more: one list per C call of
    (K.Msg, status) or (K.Msg, K.Oooi, status)"""
    from acarsdec_amd import _capi as K
    buf, st = (K.Msg * max_msgs)(), (C.c_ubyte * max_msgs)()
    obuf = (K.Oooi * max_msgs)() if oooi else None
    out = []
    while True:
        n = C.c_int(0)
        if drain:
            rc = dec.L.acg_drain_msgs_reasm(dec.ctx, buf, obuf, st, max_msgs, C.byref(n))
        else:
            rc = dec.L.acg_collect_msgs_reasm(dec.ctx, lag, buf, obuf, st, max_msgs, C.byref(n))
        dec._chk(rc, allow=(K.EAGAIN,))
        assert 0 <= n.value <= max_msgs
        recs = [K.Msg.from_buffer_copy(buf[i]) for i in range(n.value)]
        out.append([(m, K.Oooi.from_buffer_copy(obuf[i]), int(st[i])) if oooi else (m, int(st[i])) for i, m in enumerate(recs)])
        if rc == K.OK:
            return out


def play(D, x, chunk, lag, reasm, chmap=None, oooi=False, flights=False, filt=None, max_msgs=4096, counters=None, t0=T0):
    """the audio through a Decoder set up as named: (decoder, [the records of every C call]); table off: one list per wrapper call"""
    dec = D.Decoder(3, decim=8, ntaps=8, max_blocks=chunk // 1024, repair=True, bitlog=False, max_lag=2)
    if counters:
        dec.set_stream_counters(*counters)
    if chmap:
        dec.set_channel_numbers(list(chmap))
    if filt:
        dec.set_msg_filter(**filt)
    if flights:
        dec.enable_flights(t0=t0)
    if reasm:
        dec.reasm_enable(t0=t0)
    calls = []
    for s in range(0, x.shape[1], chunk):
        dec.demod_msk(x[:, s:s + chunk])
        calls += c_calls(dec, False, max_msgs, oooi, lag) if reasm else [dec.collect_msgs(lag=lag, max_msgs=max_msgs, oooi=oooi)]
    calls += c_calls(dec, True, max_msgs, oooi) if reasm else [dec.drain_msgs(max_msgs=max_msgs, oooi=oooi)]
    return dec, calls


def flat(calls):
    return [r for c in calls for r in c]


def raw_records(recs):
    """every byte handed out for the records but their statuses, sorted"""
    return sorted(b"".join(bytes(p) for p in (r if isinstance(r, tuple) else (r,)) if not isinstance(p, int)) for r in recs)


def completed(dec):
    return [done_tuple(r, text) for r, text in dec.drain_reassembled()]


def statuses(recs):
    out = {(r[0].chn, r[0].end_bit): r[-1] for r in recs}
    assert len(out) == len(recs)
    return out


@pytest.mark.parametrize("chmap", [(0, 1, 2), (7, 3, 5)], ids=["identity", "7-3-5"])
def test_tied_blocks_follow_the_numbers_handed_out(D, signal, chmap):
    """rows 0 and 2 end every block at the same sample: the copy on the lower NUMBER is the chain's, the other the DUPLICATE, the
    final pair COMPLETE then OUT_OF_SEQUENCE, the completed record carries the lower number -- slot 0's under the identity, slot 2's
    under set_channel_numbers([7, 3, 5])"""
    x, orc = signal
    want, want_done = model(orc, chmap)
    lo, hi = sorted((chmap[0], chmap[2]))
    pairs = [m.end_bit for m in orc if m.chn == 0]
    assert [want[(lo, b)] for b in pairs] == [RM.IN_PROGRESS] * 3 + [RM.COMPLETE]
    assert [want[(hi, b)] for b in pairs] == [RM.DUPLICATE] * 3 + [RM.OUT_OF_SEQUENCE]
    assert [(d[0], d[1], d[7]) for d in want_done] == [(chmap[1], 2, b"N555ZZ"), (lo, 4, b"N777AB"), (chmap[1], 3, b"UPLINK")]
    for chunk, lag in FEEDS:
        dec, calls = play(D, x, chunk, lag, True, chmap=None if chmap == (0, 1, 2) else chmap)
        got = statuses(flat(calls))
        print("chmap %s feed %s: %s" % (chmap, (chunk, lag), {k: RM.NAMES[v] for k, v in sorted(got.items())}))
        assert got == want
        assert completed(dec) == want_done and dec.reasm_dropped == 0
        dec.close()


VARIANTS = {
    "oooi": dict(oooi=True),
    "flights": dict(flights=True),
    "downlink_only": dict(filt=dict(downlink_only=True)),
    "labels_H1": dict(filt=dict(labels=["H1"])),
    "skip_empty": dict(filt=dict(skip_empty=True)),
    "skip_empty_7-3-5": dict(filt=dict(skip_empty=True), chmap=(7, 3, 5), oooi=True),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_statuses_find_their_records_behind_the_label_pass(D, signal, name):
    """with the label pass on (oooi, the flight table, -A, -b, -e) the records that reach the host are a subset of the blocks
    consumed: every handed-out record carries the model's status of ITS block, the records are byte for byte those of the same
    set-up with the table off, and the completed messages are the model's.  -A and -b decide before the table (the uplink chain,
    the 5Z chain leave no trace); -e decides behind it (the empty block is not handed out, its chain completes with 4 fragments)."""
    x, orc = signal
    kw = dict(VARIANTS[name])
    filt = kw.get("filt") or {}
    chmap = kw.get("chmap", (0, 1, 2))
    keep = lambda m: not (filt.get("downlink_only") and RM._c(m.down) == 0) and not (filt.get("labels") and RM.cstr(m.label).decode() not in filt["labels"])
    want, want_done = model(orc, chmap, keep)
    handed = {(chmap[m.chn], m.end_bit) for m in orc if keep(m) and not (filt.get("skip_empty") and m.txt_len == 0)}
    keys = [d[7] for d in want_done]
    if filt.get("downlink_only"):
        assert keys == [b"N555ZZ", b"N777AB"] and len(handed) == 10
    elif filt.get("labels"):
        assert keys == [b"N777AB", b"UPLINK"] and len(handed) == 12
    elif filt.get("skip_empty"):
        assert keys == [b"N555ZZ", b"N777AB", b"UPLINK"] and want_done[1][1] == 4 and len(handed) == 12
    else:
        assert len(handed) == 14
    for chunk, lag in FEEDS:
        off_dec, off = play(D, x, chunk, lag, False, **kw)
        off_dec.close()
        dec, calls = play(D, x, chunk, lag, True, **kw)
        got = statuses(flat(calls))
        print("%s feed %s: %s" % (name, (chunk, lag), {k: RM.NAMES[v] for k, v in sorted(got.items())}))
        assert set(got) == handed
        assert got == {k: want[k] for k in handed}
        assert raw_records(flat(calls)) == raw_records(flat(off)) and len(flat(off)) == len(handed)
        assert completed(dec) == want_done and dec.reasm_dropped == 0
        dec.close()


@pytest.mark.parametrize("max_msgs", [1, 2, 3])
def test_takes_smaller_than_the_queue(D, signal, max_msgs):
    """collect / drain with room for 1 - 3 records: every C call is a pass of its own over the blocks it consumed.  The lists
    returned per call are the model's batches: statuses and completed messages equal the model fed exactly those, each in the
    rule's order"""
    x, orc = signal
    by = {(m.chn, m.end_bit): m for m in orc}
    for chunk, lag in FEEDS:
        dec, calls = play(D, x, chunk, lag, True, max_msgs=max_msgs)
        assert sum(len(c) for c in calls) == len(orc) and max(len(c) for c in calls) == max_msgs
        t = RM.Table(T.T0_US)
        want = {}
        for c in calls:
            part = [by[(m.chn, m.end_bit)] for m, _ in c]
            for i in RM.call_order(part):
                want[(part[i].chn, part[i].end_bit)] = t.add(part[i])
        got = statuses(flat(calls))
        print("max_msgs %d feed %s: calls of %s" % (max_msgs, (chunk, lag), [len(c) for c in calls if c]))
        assert got == want
        assert sorted(want.values()).count(RM.COMPLETE) == 3
        assert completed(dec) == RC.completed_tuples(t.done)
        dec.close()


def test_outputs_entry_points_feed_the_table(D, signal):
    """acg_collect_outputs / acg_drain_outputs go through the same split: with legs (msgs, json) the legs do not change with the
    table on, and the completed messages are the model's"""
    x, orc = signal
    _, want_done = model(orc)
    for chunk, lag in FEEDS:
        legs = {}
        for reasm in (False, True):
            dec = D.Decoder(3, decim=8, ntaps=8, max_blocks=chunk // 1024, repair=True, bitlog=False, max_lag=2)
            dec.enable_outputs(("msgs", "json"), T0, station_id="TEST")
            if reasm:
                dec.reasm_enable(t0=T0)
            out = [[], []]
            for s in range(0, x.shape[1], chunk):
                dec.demod_msk(x[:, s:s + chunk])
                for acc, leg in zip(out, dec.collect_outputs(lag=lag)):
                    acc += leg
            for acc, leg in zip(out, dec.drain_outputs()):
                acc += leg
            legs[reasm] = ([bytes(m) + bytes(o) for m, o in out[0]], out[1])
            if reasm:
                assert completed(dec) == want_done and dec.reasm_dropped == 0
            dec.close()
        assert legs[True] == legs[False] and len(legs[True][0]) == len(legs[True][1]) == len(orc)


def test_stream_counters_that_straddle_2_32_samples(D, signal):
    """the counters of a fresh context placed so that the 4-block chain begins below 2^32 samples and ends above, t0 moved back by
    as many samples: the statuses of the run from 0, its completed records with the stamps shifted"""
    x, orc = signal
    chain = [m for m in orc if m.chn == 0]
    base = (1 << 32) - (chain[1].end_sample + chain[2].soh_sample) // 2
    bits = (1 << 32) - chain[2].end_bit + 50                          # the bit counter passes 2^32 inside the chain too
    assert chain[1].end_sample + base < 1 << 32 < chain[2].soh_sample + base and chain[1].end_bit + bits < 1 << 32 < chain[2].end_bit + bits
    t0, _ = T.t0_before(base)
    want, want_done = model(orc)
    for chunk, lag in FEEDS:
        zero_dec, zero = play(D, x, chunk, lag, True)
        dec, calls = play(D, x, chunk, lag, True, counters=(base, bits), t0=t0)
        z, got = statuses(flat(zero)), statuses(flat(calls))
        assert z == want and got == {(c, b + bits): s for (c, b), s in z.items()}
        assert {(m.chn, m.end_bit + bits, m.end_sample + base, m.soh_sample + base) for m, _ in flat(zero)} == {(m.chn, m.end_bit, m.end_sample, m.soh_sample) for m, _ in flat(calls)}
        zd = completed(zero_dec)
        assert zd == want_done
        assert completed(dec) == [(d[0], d[1], d[2] + bits) + tuple(s + base for s in d[3:6]) + d[6:] for d in zd]
        zero_dec.close()
        dec.close()
