"""msk_lean.hip issues its LDS operations in a different order than it reads (the newest-tap reads right behind the ring write,
the table entry in front of the tap phase): same operations, same operands, so everything the
kernel leaves behind must stay bit-identical to msk_demod_kernel (framing inline; ACG_MSK_NOLEAN=1 in the same process) after
EVERY call, and to the oracle at the end.  The shapes are the smallest at which a reordered LDS access can go wrong: a partial
wave (1, 7 channels), a wave whose last slots replicate (7, 9), a second wave (9 channels at 8 lanes per channel, 17 at 4), both
lane layouts, both workgroup shapes, with and without the bit log; calls short enough that a period straddles them (32 samples =
six periods and a bit), that the one-sample pass runs (the end of every call, and wherever the loop is out of lock) and that the
ring index wraps (every second period).  Tolerance: none."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NCH = 17
SEQS = {"short": [32, 64, 96, 32, 1024, 8192],
        "ragged": [160, 2048, 32, 992, 4096, 96, 3008, 64, 8192, 480, 1056, 2336]}
NSAMP = max(sum(v) for v in SEQS.values())


@pytest.fixture(scope="module")
def D():
    from acarsdec_amd import decoder
    from acarsdec_amd import _capi as K
    assert K.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return decoder


@pytest.fixture(scope="module")
def tracks():
    """12.5 kHz envelopes [NCH, NSAMP], the signal starting within the first short calls.  Kinds (channel % 9): plain frames; the
    same inverted (~SYN: the other polarity); six parity errors in the text (the block is dropped at MAXPERR + 2, acars.c:312);
    texts of 230-250 bytes (the length limit, acars.c:336); noise; silence; a constant; the terminator lost (the block ends at DEL,
    acars.c:323); repairable corruption in noise, inverted.  The pre-key grows by a bit from frame to frame, so that the sync
    lands on -- and the segments of the states behind it close at -- every bit position of a segment."""
    from acarsdec_amd import synth as S
    rng = np.random.default_rng(20)
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


@pytest.fixture(scope="module")
def oracle_ref(tracks):
    """{sequence: ([blocks of channel c], [framing state of channel c])} -- demodMSK + decodeAcars on the host, once"""
    from oracle import oracle as O
    ref = {}
    for name, chunks in SEQS.items():
        blocks, states = [], []
        for ch in range(NCH):
            oc = O.Channel(ch, max_frames=256)
            a0 = 0
            for n in chunks:
                oc.demod(tracks[ch, a0:a0 + n])
                a0 += n
            blocks.append(sorted(frame_key(f) for f in oc.frames))
            st = oc.state()
            states.append(tuple(int(st[k]) for k in ("MskS", "idx", "outbits", "nbits", "Acarsstate", "MskBitCount")))
        ref[name] = (blocks, states)
    return ref


def run(D, K, x, chunks, bitlog):
    """[(state bytes, texts under assembly, blocks, bit counts, bit records) after each call], blocks of all calls, final states"""
    nch = x.shape[0]
    dec = D.Decoder(nch, max_blocks=8, bitlog=bitlog)
    out, blocks = [], []
    a0 = 0
    for n in chunks:
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
        blocks += got
        snap = (bytes(st), txt, got)
        if bitlog:
            cnt, vo, lvl = dec.bits_all()
            snap += (cnt.tobytes(), b"".join(vo[c, : cnt[c]].tobytes() + lvl[c, : cnt[c]].tobytes() for c in range(nch)))
        out.append(snap)
        a0 += n
    states = []
    for ch in range(nch):
        g = dec.state(ch)
        states.append(tuple(int(g[k]) for k in ("MskS", "idx", "outbits", "nbits", "Acarsstate", "MskBitCount")))
    dec.close()
    return out, sorted(blocks), states


@pytest.mark.parametrize("lpc,cus", [(8, None), (4, None), (8, 0), (4, 0)])
def test_reordered_lean_kernel_is_the_inline_kernel_and_the_oracle(D, tracks, oracle_ref, tune, lpc, cus):
    from acarsdec_amd import _capi as K
    tune("ACG_MSK_LPC", str(lpc))
    if cus is not None:
        tune("ACG_MSK_CUS", str(cus))
    cases = [(nch, name, bitlog) for nch in (1, 7, 9, 17) for name in SEQS for bitlog in (False, True)]
    lean = {}
    for nch, name, bitlog in cases:
        lean[nch, name, bitlog] = run(D, K, tracks[:nch], SEQS[name], bitlog)
    tune("ACG_MSK_NOLEAN", "1")
    nblocks = 0
    for nch, name, bitlog in cases:
        where = "%d channels, %s calls, bit log %d" % (nch, name, bitlog)
        a, a_blocks, a_states = lean[nch, name, bitlog]
        b, b_blocks, b_states = run(D, K, tracks[:nch], SEQS[name], bitlog)
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
        # once at the end: the oracle's blocks and framing state
        o_blocks, o_states = oracle_ref[name]
        assert a_blocks == sorted(f for ch in range(nch) for f in o_blocks[ch]), where
        assert a_states == o_states[:nch], where
        assert b_blocks == a_blocks and b_states == a_states, where
        nblocks += len(a_blocks)
    # the traffic did what it is there for: blocks came out on the long sequence, of both polarities and from the DEL ending
    full = lean[17, "ragged", False][1]
    chans = {f[0] for f in full}
    assert {0, 1, 7} <= chans and not ({4, 5, 6} & chans), sorted(chans)
    assert nblocks > 100
