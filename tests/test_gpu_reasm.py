"""Reassembly of multi-block messages on the device (reasm.hip) against its specification, tests/reasm_model.py: through the lab
entry acg_selftest_reasm on hand-written and random records, and end to end on signal through a context.  This file checks the
status rule where the slot rules cannot be seen: its traffic can drop nobody and only idle slots are taken again.  The slots at full
load (the take-over of an expired live entry, the probe bound inside a larger table, racing claims, sample indices above 2^32) are
tests/test_gpu_reasm_pressure.py's; the context with channel numbers, the label pass, small takes, the outputs' entry points and
large counters is tests/test_gpu_reasm_context.py's (here: three channels, no filter, identity numbers, counters from 0)."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reasm_cases as RC  # noqa: E402
import reasm_model as RM  # noqa: E402

pytestmark = pytest.mark.gpu

T0 = (1700000000, 250000)
T0_US = T0[0] * 10**6 + T0[1]


@pytest.fixture(scope="module")
def K():
    from acarsdec_amd import _capi
    assert _capi.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return _capi


def done_tuple(r, text):
    """a handed-out acg_reasm_msg as reasm_model.Completed.astuple(); every byte of the record is defined"""
    raw = bytes(r)
    assert raw[53:61] == bytes(r.addr).ljust(8, b"\0") and raw[61:64] == bytes(r.label).ljust(3, b"\0") and raw[64:68] == bytes(r.msn).ljust(4, b"\0")
    assert raw[68:80] == b"\0" * 12 and r.text_len == len(text)
    return (r.chn, r.nfrag, r.end_bit, r.end_sample, r.soh_sample, r.first_soh_sample, r.down[0], bytes(r.addr), bytes(r.label), bytes(r.msn), text)


def device_run(K, msgs, batches, max_msgs=0, max_text=0, filt=None, pass_ms=False):
    """msgs through acg_selftest_reasm in calls of `batches` records: (statuses, completed tuples, dropped[, pass_ms])"""
    L = K.load(lab=True)
    n = len(msgs)
    assert sum(batches) == n
    arr = RC.pack(msgs)
    b = (C.c_int * len(batches))(*batches)
    cfg = K.ReasmConfig(T0[0], T0[1], max_msgs, max_text)
    status = (C.c_ubyte * max(n, 1))()
    done = (K.ReasmMsg * max(n, 1))()
    cap = max(n, 1) * 242 + 16
    text = C.create_string_buffer(cap)
    nd, dr = C.c_int(0), C.c_int(-1)
    ms = (C.c_float * len(batches))() if pass_ms else None
    rc = L.acg_selftest_reasm(arr, b, len(batches), C.byref(cfg), C.byref(filt) if filt is not None else None, status, done, n, text, cap, C.byref(nd), C.byref(dr), ms)
    assert rc == K.OK, rc
    out = []
    at = 0
    for i in range(nd.value):
        r = done[i]
        assert r.text_off == at                                       # packed back to back
        out.append(done_tuple(r, text.raw[at:at + r.text_len]))
        at += r.text_len
    res = (list(status[:n]), out, dr.value)
    return res + (list(ms),) if pass_ms else res


def check(K, msgs, batches, **kw):
    want_status, want_done, _ = RM.run(msgs, batches, t0_us=T0_US, max_text=kw.get("max_text", 0) or RM.DEFAULT_MAX_TEXT)
    status, done, dropped = device_run(K, msgs, batches, **kw)
    bad = [i for i in range(len(msgs)) if status[i] != want_status[i]]
    assert not bad, (len(bad), [(i, status[i], want_status[i]) for i in bad[:10]])
    assert done == RC.completed_tuples(want_done) and dropped == 0
    return want_status, want_done


def test_hand_written_chains_in_one_batch_and_cut_at_every_position(K):
    msgs, want = RC.hand_chains()
    got, _ = check(K, msgs, [len(msgs)])
    assert got == want
    for cut in range(1, len(msgs)):
        check(K, msgs, [cut, len(msgs) - cut])
    check(K, msgs, [1] * len(msgs))
    tm, tw = RC.timeout_chains()
    got, done = check(K, tm, [len(tm)])
    assert got == tw and len(done) == 2
    for cut in range(1, len(tm)):
        check(K, tm, [cut, len(tm) - cut])
    for max_text in (16, 256, 3584):
        om, ow = RC.overflow_chain(max_text)
        got, done = check(K, om, [len(om)], max_text=max_text)
        assert got == ow and len(done[0].text) == max_text
        check(K, om, [len(om) // 2, len(om) - len(om) // 2], max_text=max_text)


@pytest.fixture(scope="module")
def traffic():
    return RC.random_traffic()


@pytest.mark.parametrize("max_msgs", [256, 1024])
def test_random_traffic_equals_the_model(K, traffic, max_msgs):
    """20 000 records over ~300 keys, ETB chains of 2-16 blocks with duplicates, losses and time-outs, in calls of 1-2000 records
    whose records come in a random order (tests/test_reasm_model.py proves that no claim order can drop anybody)"""
    batches = RC.random_batches(len(traffic), seed=5 if max_msgs == 256 else 6)
    msgs = RC.shuffled_within(traffic, batches, seed=max_msgs)
    status, done = check(K, msgs, batches, max_msgs=max_msgs)
    assert len(done) > 1000 and status.count(RM.DUPLICATE) > 100 and status.count(RM.OUT_OF_SEQUENCE) > 100


def test_filters_decide_before_the_table(K):
    """-A / -b are applied before the table, -e is not: an uplink under -A and a label outside -b are SKIPPED and leave no trace;
    an empty fragment passes whatever -e says"""
    from acarsdec_amd import decoder
    msgs, _ = RC.hand_chains()
    L = K.load(lab=True)
    f = decoder.make_msg_filter(True, True, ["H1"], L)
    keep = lambda m: RM._c(m.down) != 0 and RM.cstr(RM.raw(m, "label", 2)) == b"H1"
    want_status, want_done, _ = RM.run(msgs, [len(msgs)], t0_us=T0_US, keep=keep)
    status, done, dropped = device_run(K, msgs, [len(msgs)], filt=f)
    assert status == want_status and done == RC.completed_tuples(want_done) and dropped == 0
    assert [d[7] for d in done] == [b"N123AB", b"N123AB"]            # the uplink chains are gone, the chain with the empty fragment is not


def test_keys_that_differ_in_one_character(K):
    msgs = RC.one_field_keys()
    status, done = check(K, msgs, [len(msgs)])
    assert len(done) == 11
    check(K, RC.shuffled_within(msgs, [len(msgs)], 3), [len(msgs)])


def test_pressure_where_the_answer_is_determinate(K):
    """a table of 128 slots is one probe window: 127 chains in progress plus one new key fit; one more new key finds no slot: its
    creating block is UNKNOWN, dropped == 1, its next block is what a block without an entry is; once the 127 are complete their
    slots are taken again"""
    t = [300000]

    def blk(i, k, final=False):
        t[0] += 700
        return RC.msg(addr=b"P%05d" % i, no=b"P%02d" % (i % 100) + bytes([65 + k]), be=RC.ETX if final else RC.ETB, txt=b"%d.%d/" % (i, k), end_sample=t[0], chn=i % 5)

    calls = [[blk(i, 0) for i in range(127)], [blk(127, 0)], [blk(128, 0), blk(128, 1)], [blk(i, 1, True) for i in range(127)],
             [blk(128, 0), blk(129, 0), blk(130, 0)], [blk(128, 1, True), blk(127, 1, True), blk(129, 1, True), blk(130, 1, True)]]
    msgs = [m for c in calls for m in c]
    batches = [len(c) for c in calls]
    status, done, dropped = device_run(K, msgs, batches, max_msgs=128)
    assert dropped == 1
    # the model has no bound: it is asked about the same calls without the two blocks of the key that found no slot
    at = 128
    want, want_done, _ = RM.run(msgs[:at] + msgs[at + 2:], batches[:2] + batches[3:], t0_us=T0_US)
    assert status[at] == RM.UNKNOWN and status[at + 1] == RM.OUT_OF_SEQUENCE
    assert status[:at] == want[:at] and status[at + 2:] == want[at:] and set(want) == {RM.IN_PROGRESS, RM.COMPLETE}
    assert done == RC.completed_tuples(want_done) and len(done) == 127 + 4


def test_one_key_with_4000_events_in_a_single_batch(K):
    msgs = []
    t = 400000
    i = 0
    while len(msgs) < 4000:
        for k in range(1 + i % 7):
            t += 600
            last = k == i % 7
            msgs.append(RC.msg(no=b"S01" + bytes([65 + k]), be=RC.ETX if last else RC.ETB, txt=RC.text_of(len(msgs), (i * 5 + k * 3) % 60), end_sample=t, chn=k % 4))
            if (i + k) % 11 == 0:                                     # a retransmission
                t += 600
                msgs.append(RC.msg(no=b"S01" + bytes([65 + k]), be=RC.ETX if last else RC.ETB, txt=b"again", end_sample=t, chn=4))
        i += 1
    msgs = msgs[:4000]
    status, done = check(K, RC.shuffled_within(msgs, [4000], 9), [4000])
    assert len(done) > 500 and status.count(RM.DUPLICATE) > 100


# ---- end to end on signal -------------------------------------------------------------------------------------------------------
def chain_audio():
    """[3, nsamp] audio: a 3-block downlink whose middle block is heard on another channel, a chain with a retransmitted block, a
    chain with a lost block, an uplink chain over the wrap of mode '2', and single-block messages between them"""
    from acarsdec_amd import synth as S
    rng = np.random.default_rng(21)
    plan = [(0, b"M01A", b"3", True), (1, b"M01B", b"3", True), (0, b"M01C", b"3", False),
            (2, b"S07A", b"5", False),
            (1, b"M02A", b"4", True), (1, b"M02B", b"4", True), (2, b"M02B", b"4", True), (1, b"M02C", b"4", False),
            (0, None, b"Y", True), (0, None, b"Z", True), (2, None, b"A", False),
            (2, b"M03A", b"6", True), (2, b"M03C", b"6", True), (2, b"M03D", b"6", False),
            (1, None, b"C", False)]
    x = np.zeros((3, 98304), dtype=np.float32)
    pos = 1500
    for chn, no, bid, etb in plan:
        body = S.random_text(rng, 20, 70)
        text = (no + b"XY0042" + body) if no else body
        fr = S.acars_frame(text=text, addr=b".N777AB" if no else b".UPLINK", label=b"H1", bid=bid, etb=etb)
        a = S.msk_audio(S.frame_bits(fr), phase0=float(rng.uniform(0, 2 * np.pi)))
        assert pos + a.size + 500 < x.shape[1]
        x[chn, pos:pos + a.size] = 0.06 * a
        pos += a.size + int(rng.integers(800, 2500))
    return x, len(plan)


def oracle_messages(x):
    """what the CPU oracle makes of the audio: its split messages with the block's place, in (end_sample, chn) order"""
    from oracle import oracle as O
    out = []
    for c in range(x.shape[0]):
        ch = O.Channel(c)
        ch.demod(x[c])
        for f in ch.frames:
            p = O.blk_process(f)
            if p is None:
                continue
            s = O.msg_split(p)
            out.append(types.SimpleNamespace(chn=c, end_bit=int(f.end_bit), end_sample=int(f.end_sample), soh_sample=int(f.soh_sample), mode=bytes(s.mode),
                                             addr=C.string_at(C.addressof(s) + O.OrcMsg.addr.offset, 8), label=C.string_at(C.addressof(s) + O.OrcMsg.label.offset, 3),
                                             bid=bytes(s.bid), no=C.string_at(C.addressof(s) + O.OrcMsg.no.offset, 5), bs=bytes(s.bs), be=bytes(s.be),
                                             down=bytes(s.down), txt=bytes(s.txt[:242]), txt_len=int(s.txt_len)))
    out.sort(key=lambda m: (m.end_sample, m.chn))
    return out


def play(D, x, chunk, lag, reasm, sink=None):
    dec = D.Decoder(x.shape[0], decim=8, ntaps=8, max_blocks=chunk // 1024, repair=True, bitlog=False, max_lag=2)
    if reasm:
        dec.reasm_enable(t0=T0)
    if sink == "json":
        dec.enable_json(T0, station_id="TEST")
    if sink == "text":
        dec.enable_text("std", T0, date=True)
    out = []
    for s in range(0, x.shape[1], chunk):
        dec.demod_msk(x[:, s:s + chunk])
        if sink == "json":
            out.append(dec.collect_json(lag=lag))
        elif sink == "text":
            out += dec.collect_text(lag=lag)
        else:
            out += dec.collect_msgs(lag=lag, reasm=reasm)
    if sink == "json":
        out.append(dec.drain_json())
    elif sink == "text":
        out += dec.drain_text()
    else:
        out += dec.drain_msgs(reasm=reasm)
    return dec, out


def test_end_to_end_on_signal(K):
    from acarsdec_amd import decoder as D
    x, nframes = chain_audio()
    orc = oracle_messages(x)
    assert len(orc) == nframes
    t = RM.Table(T0_US)
    want = {(m.chn, m.end_bit): t.add(m) for m in orc}
    assert sorted(want.values()).count(RM.COMPLETE) == 3 and RM.DUPLICATE in want.values() and RM.OUT_OF_SEQUENCE in want.values()
    assert [(c.addr, c.msn, c.nfrag) for c in t.done] == [(b"N777AB", b"M01", 3), (b"N777AB", b"M02", 3), (b"UPLINK", b"", 3)]
    plain_dec, plain = play(D, x, 4096, 1, False)
    plain_dec.close()
    assert len(plain) == nframes
    for chunk, lag in ((4096, 1), (8192, 0)):
        dec, got = play(D, x, chunk, lag, True)
        assert sorted(bytes(m) for m, _ in got) == sorted(bytes(m) for m in plain)       # the records: byte-identical with the table on
        assert {(m.chn, m.end_bit): s for m, s in got} == want
        done = [done_tuple(r, text) for r, text in dec.drain_reassembled()]
        assert done == RC.completed_tuples(t.done) and dec.reasm_dropped == 0
        assert dec.drain_reassembled() == []
        assert [dec.reasm_status_name(s) for s in range(8)] == list(RM.NAMES)
        dec.close()
    # the sinks feed the table too, and their bytes do not change
    for sink in ("json", "text"):
        a, off = play(D, x, 4096, 1, False, sink)
        b, on = play(D, x, 4096, 1, True, sink)
        assert on == off and sum(len(p) for p in off) > 1000
        assert [done_tuple(r, text) for r, text in b.drain_reassembled()] == RC.completed_tuples(t.done)
        a.close()
        b.close()


def test_states(K):
    from acarsdec_amd import decoder as D
    L = K.load()
    x, nframes = chain_audio()
    # without ACG_F_REPAIR: ACG_ESTATE
    dec = D.Decoder(3, decim=8, ntaps=8, max_blocks=4, repair=False, bitlog=False)
    cfg = K.ReasmConfig(T0[0], T0[1], 0, 0)
    assert L.acg_reasm_enable(dec.ctx, C.byref(cfg)) == K.ESTATE
    n, nb = C.c_int(0), C.c_size_t(0)
    assert L.acg_drain_reassembled(dec.ctx, None, 0, C.byref(n), None, 0, C.byref(nb), None) == K.ESTATE
    dec.close()
    dec = D.Decoder(3, decim=8, ntaps=8, max_blocks=8, repair=True, bitlog=False)
    buf, st = (K.Msg * 64)(), (C.c_ubyte * 64)()
    assert L.acg_drain_msgs_reasm(dec.ctx, buf, None, st, 64, C.byref(n)) == K.ESTATE              # the table is off
    for bad in (K.ReasmConfig(0, -1, 0, 0), K.ReasmConfig(0, 0, 0, 40), K.ReasmConfig(0, 0, -5, 0), K.ReasmConfig(0, 0, 0, 131072)):
        assert L.acg_reasm_enable(dec.ctx, C.byref(bad)) == K.EINVAL
    def run(x):
        out = []
        for s in range(0, x.shape[1], 8192):
            dec.demod_msk(x[:, s:s + 8192])
            out += dec.drain_msgs()                                   # the plain entry point beside an enabled table still feeds it
        return out

    orc = oracle_messages(x)
    m02a = [m for m in orc if m.no[:4] == b"M02A"][0]
    cut = (m02a.end_sample + 200 + 1023) // 1024 * 1024               # behind M02A, before the end of M02B
    assert cut < [m for m in orc if m.no[:4] == b"M02B"][0].end_sample
    dec.reasm_enable(t0=T0)
    assert len(run(x)) == nframes
    # ACG_EAGAIN by max, the remainder kept in order
    recs, text = (K.ReasmMsg * 8)(), C.create_string_buffer(8192)
    assert L.acg_drain_reassembled(dec.ctx, recs, 1, C.byref(n), text, 8192, C.byref(nb), None) == K.EAGAIN and n.value == 1
    first = (bytes(recs[0].msn), text.raw[:nb.value])
    # ... and by cap: the second text does not fit 10 bytes, nothing is handed out, nothing is lost
    assert L.acg_drain_reassembled(dec.ctx, recs, 8, C.byref(n), text, 10, C.byref(nb), None) == K.EAGAIN and n.value == 0 and nb.value == 0
    rest = dec.drain_reassembled()
    assert first[0] == b"M01" and [bytes(r.msn) for r, _ in rest] == [b"M02", b""] and len(first[1]) > 60
    # acg_reset empties the table and the completed messages not yet drained: a chain cut by the reset does not complete, the same
    # input from the start completes again afterwards
    run(x[:, :cut])
    dec.reset()
    run(x)
    assert [bytes(r.msn) for r, _ in dec.drain_reassembled()] == [b"M01", b"M02", b""]
    # disable / enable: an empty table and an empty queue again (M02 lost its first block with the old table); disabled: ACG_ESTATE
    run(x[:, :cut])
    dec.reasm_disable()
    assert L.acg_drain_reassembled(dec.ctx, recs, 8, C.byref(n), text, 8192, C.byref(nb), None) == K.ESTATE
    dec.reasm_enable(t0=T0)
    assert dec.drain_reassembled() == []
    run(x[:, cut:])
    assert [bytes(r.msn) for r, _ in dec.drain_reassembled()] == [b""]
    dec.close()
