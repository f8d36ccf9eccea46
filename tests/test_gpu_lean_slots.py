"""msk_lean.hip with the issue slots of round 10 taken out of a bit period (one counted wait in front of the five old taps, the fifth
step's hold without the clock, the mixer's Horner steps as three-address fmas): the same operations on the same operands per
channel, so everything the kernel leaves behind stays bit-identical to msk_demod_kernel (ACG_MSK_NOLEAN=1 in the same process)
after EVERY call -- the state record with its doubles and its ring, the text rows, the blocks, the bit counts and the bit records.
No tolerance, every channel, every call.

What the shapes are there for:
 * 1, 7, 8, 9 and 17 channels: slots that replicate the last channel, a last wave with one real group, a wave without any channel
   in a workgroup of four; 8 and 4 lanes per channel (one and two mixer evaluations per lane, so one and two ring writes in front
   of the counted wait, whose count follows them), both workgroup shapes;
 * calls of 32, 64, 96, 192 and 8192 samples in ONE context: the prologue's three block loads are clamped by the call's length
   (below one, two and three window blocks), a period straddles every call's end, and a long call refills the window 127 times;
 * the 8192-sample call either as one launch (bit_append off) or through the down-converter in eight chunks whose launches
   append to the call's log and count (ACG_PIPE_BLOCKS=1: bit_append on in seven of them), with and without the bit log;
 * a channel in every framing state at the start of some call: the schedule's boundaries are placed where channel 0 of
   tests/msk_exact_inputs.py's tracks is in SYN2, SOH1, CRC1, CRC2 and END (and WSYN and TXT anyway), which the test asserts on
   the states the device reports."""
import ctypes as C

import numpy as np
import pytest

import msk_exact_inputs as X

pytestmark = pytest.mark.gpu

NCH = 17
BIG = 1                                                # index of the 8192-sample call
SCHED = [32, 8192, 32, 32, 192, 192, 192, 32, 64, 96, 192, 64, 96]
M = 160


@pytest.fixture(scope="module")
def D():
    from acarsdec_amd import decoder
    from acarsdec_amd import _capi as K
    assert K.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return decoder


@pytest.fixture(scope="module")
def tracks():
    x = X.tracks()[:NCH]
    assert sum(SCHED) <= x.shape[1] and sorted(set(SCHED)) == [32, 64, 96, 192, 8192]
    return x


@pytest.fixture(scope="module")
def dongle(tracks):
    """(iq, taps): the 8192 samples of the long call on 17 carriers of ONE u8 stream, 50 kHz apart, and the channels' taps"""
    from acarsdec_amd import synth as S
    from oracle import oracle as O
    a0 = sum(SCHED[:BIG])
    offs = [50000.0 * (c - NCH // 2) for c in range(NCH)]
    iq = S.iq_u8_from_envelopes(tracks[:, a0:a0 + SCHED[BIG]].astype(np.float64), M, offs, phases=[0.37 * c for c in range(NCH)],
                                scale=0.08, noise=0.0, rng=np.random.default_rng(5))
    taps = np.stack([O.rtl_taps(131000000 + int(o), 131000000, M) for o in offs])
    return iq.reshape(1, -1), taps


def frame_key(f):
    return (f.chn, f.len, f.err, bytes(f.crc), bytes(f.txt[: f.len]), f.end_bit, f.end_sample, f.soh_sample, f.lvl)


def run(D, K, x, dongle, nch, bitlog, chunked):
    """[(state bytes, text rows, blocks, bit counts, bit records, framing states) after each call]"""
    if chunked:
        dec = D.Decoder(nch, decim=M, nstreams=1, max_blocks=8, bitlog=bitlog)
        dec.set_taps(dongle[1][:nch])
    else:
        dec = D.Decoder(nch, max_blocks=8, bitlog=bitlog)
    out, a0 = [], 0
    for i, n in enumerate(SCHED):
        if chunked and i == BIG:
            dec.in_callback(dongle[0])
        else:
            dec.demod_msk(x[:nch, a0:a0 + n])
        dec.sync()
        st = (K.ChanState * nch)()
        dec._chk(dec.L.acg_get_state_n(dec.ctx, 0, nch, st))
        txt = []
        for ch in range(nch):
            if st[ch].Acarsstate == X.TXT:
                buf = (C.c_ubyte * 256)()
                dec._chk(dec.L.acg_get_block_text(dec.ctx, ch, buf))
                txt.append(bytes(buf[: st[ch].blk_len]))
            else:
                txt.append(b"")
        blocks = sorted(frame_key(f) for f in dec.drain_frames())
        cnt, vo, lvl = dec.bits_all() if bitlog else (np.zeros(nch, np.int32), None, None)
        rec = b"".join(vo[c, : cnt[c]].tobytes() + lvl[c, : cnt[c]].tobytes() for c in range(nch)) if bitlog else b""
        out.append((bytes(st), txt, blocks, cnt.tobytes(), rec, [int(st[ch].Acarsstate) for ch in range(nch)]))
        a0 += n
    dec.close()
    return out


@pytest.mark.parametrize("lpc,cus", [(8, None), (4, None), (8, 0), (4, 0)])
def test_a_period_without_its_idle_slots_is_the_inline_kernel(D, tracks, dongle, tune, lpc, cus):
    from acarsdec_amd import _capi as K
    tune("ACG_MSK_LPC", str(lpc))
    tune("ACG_PIPE_BLOCKS", "1")                       # (read where a context is made: the chunked contexts take chunks of one block)
    if cus is not None:
        tune("ACG_MSK_CUS", str(cus))
    cases = [(nch, bitlog, chunked) for nch in (1, 7, 8, 9, 17) for bitlog in (True, False) for chunked in (False, True)]
    lean = {case: run(D, K, tracks, dongle, *case) for case in cases}
    tune("ACG_MSK_NOLEAN", "1")
    nblocks = nbits = 0
    for case in cases:
        nch, bitlog, chunked = case
        where = "%d channels, bit log %d, long call %s" % (nch, bitlog, "in eight appending chunks" if chunked else "as one launch")
        a, b = lean[case], run(D, K, tracks, dongle, *case)
        assert len(a) == len(b) == len(SCHED)
        for i, (p, q) in enumerate(zip(a, b)):
            if p[0] != q[0]:
                sz = C.sizeof(K.ChanState)
                bad = [ch for ch in range(nch) if p[0][ch * sz:(ch + 1) * sz] != q[0][ch * sz:(ch + 1) * sz]]
                raise AssertionError("%s, call %d (%d samples): state differs on channels %s" % (where, i, SCHED[i], bad))
            assert p[1] == q[1], "%s, call %d: text rows differ" % (where, i)
            assert p[2] == q[2], "%s, call %d: blocks differ" % (where, i)
            assert p[3] == q[3], "%s, call %d: bits per channel differ" % (where, i)
            assert p[4] == q[4], "%s, call %d: bit records {soft symbol, level} differ" % (where, i)
            nblocks += len(p[2])
        if bitlog:
            nbits += int(np.frombuffer(a[BIG][3], dtype=np.int32).sum())
            # the long call's log holds the whole call in both shapes: about one bit per 5.2 samples on every channel that fires
            assert int(np.frombuffer(a[BIG][3], dtype=np.int32)[0]) > SCHED[BIG] // 6, where
    assert nblocks > 20 and nbits > 20 * 1000, (nblocks, nbits)
    # every framing state stood at the start of some call, on channel 0 (so in every shape above)
    one = lean[1, True, False]
    seen = {snap[5][0] for snap in one[:-1]} | {X.WSYN}
    assert seen == {X.WSYN, X.SYN2, X.SOH1, X.TXT, X.CRC1, X.CRC2, X.END}, sorted(seen)
