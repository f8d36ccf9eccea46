"""msk_lean.hip runs the VCO phase steps and the clock steps of a bit period side by side, all six of each in one block, and a
lane that turns out not to take them (the loop out of lock, the clock firing early, the call ending) drops what it computed.  Same
operations on the same operands per channel, so everything the kernel leaves behind stays bit-identical to msk_demod_kernel
(ACG_MSK_NOLEAN=1 in the same process) after EVERY call: the state record with its doubles, the text under assembly, the blocks,
the bit counts and the bit records.  No tolerance, every channel, every call.

What the cases are there for:
 * a phase wrap at every one of the six steps, on the `>=` edge: a channel is given df = 0 (so that the step is K_VCO exactly),
   a phase whose j-th running sum IS 2 pi, and a clock with which the period has at least j samples; and the same one ulp lower,
   where that step does not wrap.  The phases are found by search and checked in float64 / float32 arithmetic on the host.
 * lanes whose speculative steps are dropped: df = -1 (the step is negative: one sample per period, for good), df = +3 (the clock
   fires on the first sample), noise, silence and a constant, in the same wave as channels in lock, so that lanes of one period
   differ in which steps they keep.
 * calls of 32, 64, 96 and 128 samples (a period straddles every call and the six-sample pass does not fit at its end), then
   1024 and 8192; 1, 7, 9 and 17 channels; 8 and 4 lanes per channel; both workgroup shapes; with and without the bit log.
The traffic is that of test_gpu_lean_order.py (both polarities, parity errors, the length limit, a lost terminator, repairable
corruption), so that five- and six-sample periods and the rare framing branches run behind the front part."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NCH = 17
# "ends": planted once, in front of the first call; "plants": planted in front of every call, every plant on every planted channel
SEQS = {"ends": [32, 64, 96, 128, 1024, 8192], "plants": [32, 64, 96, 128] * 4}
NSAMP = max(sum(v) for v in SEQS.values())


@pytest.fixture(scope="module")
def plants():
    """[(phi, df, clk)]: for j = 1..6 the wrap exactly at step j, then the same one ulp lower, then df = -1 and df = +3 (derived and
    checked in tests/msk_exact_inputs.py, which holds them to the oracle as well)"""
    import msk_exact_inputs as X
    return X.plants()


@pytest.fixture(scope="module")
def D():
    from acarsdec_amd import decoder
    from acarsdec_amd import _capi as K
    assert K.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return decoder


@pytest.fixture(scope="module")
def tracks():
    """12.5 kHz envelopes [NCH, NSAMP]; kinds by channel % 9 as in test_gpu_lean_order.py: plain frames; inverted; six parity errors;
    texts at the length limit; noise; silence; a constant; the terminator lost; repairable corruption in noise, inverted"""
    from acarsdec_amd import synth as S
    rng = np.random.default_rng(23)
    x = np.zeros((NCH, NSAMP), dtype=np.float32)

    def audio(frames, gap):
        parts = [np.zeros(int(rng.integers(0, 40)))]
        for i, fr in enumerate(frames):
            parts.append(S.msk_audio(S.frame_bits(fr, prekey=32 + (i + len(frames)) % 8), phase0=float(rng.uniform(0, 2 * np.pi))))
            parts.append(np.zeros(int(rng.integers(*gap))))
        a = np.concatenate(parts)
        return a[:NSAMP] if len(a) >= NSAMP else np.concatenate([a, np.zeros(NSAMP - len(a))])

    for c in range(NCH):
        k = c % 9
        if k in (0, 1, 2, 3, 7, 8):
            frames = []
            for i in range(3 if k == 3 else 12):
                fr = bytearray(S.acars_frame(text=S.random_text(rng, 230, 250) if k == 3 else S.random_text(rng, 1, 40)))
                if k == 2 and len(fr) > 32:
                    for j in rng.choice(np.arange(20, len(fr) - 6), size=6, replace=False):
                        fr[int(j)] ^= 1 << int(rng.integers(0, 7))
                if k == 7:
                    fr[len(fr) - 4] = S.odd_parity(0x41 + int(rng.integers(0, 26)))
                if k == 8:
                    fr = bytearray(S.corrupt_frame(bytes(fr), rng, ["p1", "p2", "p3", "p4", "db", "crc"][i % 6])) if len(fr) > 24 else fr
                frames.append(bytes(fr))
            a = audio(frames, (40, 400))
            x[c] = S.envelope(-a if k in (1, 8) else a, noise=0.02 if k == 8 else 0.0, rng=rng)
        elif k == 4:
            x[c] = rng.normal(0.5, 0.2, size=NSAMP).astype(np.float32)
        elif k == 5:
            x[c] = 0.0
        else:
            x[c] = 0.37
    return x


def frame_key(f):
    return (f.chn, f.len, f.err, bytes(f.crc), bytes(f.txt[: f.len]), f.end_bit, f.end_sample, f.soh_sample, f.lvl)


def plant_for(name, call, ch, plants):
    """the plant of channel `ch` in front of call number `call`, or None.  Even channels are planted, odd ones keep their lock, so
    that both kinds share every wave (8 or 16 channels each)."""
    if ch % 2:
        return None
    if name == "plants":
        return plants[(ch // 2 + call) % len(plants)]
    if call == 0 and ch > 0:
        return plants[-2] if ch % 4 == 2 else plants[-1]               # df = -1 on 2, 6, 10, 14; df = +3 on 4, 8, 12, 16
    return None


def run(D, K, x, name, bitlog, plants):
    """[(state bytes, texts under assembly, blocks, bit counts, bit records) after each call]"""
    nch = x.shape[0]
    dec = D.Decoder(nch, max_blocks=8, bitlog=bitlog)
    out = []
    a0 = 0
    for i, n in enumerate(SEQS[name]):
        todo = [(ch, plant_for(name, i, ch, plants)) for ch in range(nch)]
        if any(p is not None for _, p in todo):
            st = (K.ChanState * nch)()
            dec._chk(dec.L.acg_get_state_n(dec.ctx, 0, nch, st))
            for ch, p in todo:
                if p is not None:
                    st[ch].MskPhi, st[ch].MskDf, st[ch].MskClk = p
            dec._chk(dec.L.acg_set_state_n(dec.ctx, 0, nch, st))
        dec.demod_msk(x[:, a0:a0 + n])
        dec.sync()
        st = (K.ChanState * nch)()
        dec._chk(dec.L.acg_get_state_n(dec.ctx, 0, nch, st))
        txt = []
        for ch in range(nch):
            if st[ch].Acarsstate == 3:
                buf = (C.c_ubyte * 256)()
                dec._chk(dec.L.acg_get_block_text(dec.ctx, ch, buf))
                txt.append(bytes(buf[: st[ch].blk_len]))
            else:
                txt.append(b"")
        got = sorted(frame_key(f) for f in dec.drain_frames())
        snap = (bytes(st), txt, got)
        if bitlog:
            cnt, vo, lvl = dec.bits_all()
            snap += (cnt.tobytes(), b"".join(vo[c, : cnt[c]].tobytes() + lvl[c, : cnt[c]].tobytes() for c in range(nch)))
        out.append(snap)
        a0 += n
    dec.close()
    return out


@pytest.mark.parametrize("lpc,cus", [(8, None), (4, None), (8, 0), (4, 0)])
def test_side_by_side_vco_and_clock_steps_are_the_inline_kernel(D, tracks, plants, tune, lpc, cus):
    from acarsdec_amd import _capi as K
    tune("ACG_MSK_LPC", str(lpc))
    if cus is not None:
        tune("ACG_MSK_CUS", str(cus))
    cases = [(nch, name, bitlog) for nch in (1, 7, 9, 17) for name in SEQS for bitlog in (False, True)]
    lean = {case: run(D, K, tracks[:case[0]], case[1], case[2], plants) for case in cases}
    tune("ACG_MSK_NOLEAN", "1")
    nblocks = 0
    for nch, name, bitlog in cases:
        where = "%d channels, %s calls, bit log %d" % (nch, name, bitlog)
        a = lean[nch, name, bitlog]
        b = run(D, K, tracks[:nch], name, bitlog, plants)
        assert len(a) == len(b) == len(SEQS[name])
        for i, (p, q) in enumerate(zip(a, b)):
            if p[0] != q[0]:
                sz = C.sizeof(K.ChanState)
                bad = [ch for ch in range(nch) if p[0][ch * sz:(ch + 1) * sz] != q[0][ch * sz:(ch + 1) * sz]]
                raise AssertionError("%s, call %d: state differs on channels %s" % (where, i, bad))
            assert p[1] == q[1], "%s, call %d: block text under assembly differs" % (where, i)
            assert p[2] == q[2], "%s, call %d: blocks differ" % (where, i)
            if bitlog:
                assert p[3] == q[3], "%s, call %d: bits per channel differ" % (where, i)
                assert p[4] == q[4], "%s, call %d: bit records {soft symbol, level} differ" % (where, i)
            nblocks += len(p[2])
    # the traffic did what it is there for: the channels in lock delivered blocks behind the changed front part, of both
    # polarities and from the DEL ending, and the channel that was given df = -1 never fired a bit again
    full = lean[17, "ends", True]
    chans = {f[0] for snap in full for f in snap[2]}
    assert {1, 7, 9} <= chans, sorted(chans)
    assert nblocks > 10, nblocks
    cnt = np.frombuffer(full[-1][3], dtype=np.int32)
    assert cnt[2] == 0 and cnt[1] > 1000, cnt
