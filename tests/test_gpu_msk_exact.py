"""The assembled demodulator loop against the oracle, bit for bit.  All three kernels (msk_lean_kernel, msk_demod_kernel, the lab's
msk_demod2_kernel) take the phase detector, loop filter, table sin/cos, quotients, square root, phase wrap and framing from one
header (msk_common.h), so a change there moves them together and the kernel-against-kernel tests cannot see it; against the oracle
the suite so far held the soft bits to 1e-4 and the doubles to 1e-9.  Here: through acg_process_dm_host, after EVERY call, on every
channel, with NO tolerance and no excluded case --

  * the bit count and the bit records {vo, lvl} as float32 bit patterns (+0 and -0 taken as equal).  The oracle writes its log
    where the device does: BEHIND the MskS & 2 sign (acars_oracle.c orc_demod_msk, `sv = (MskS & 2) ? -vo : vo` is what it logs
    and hands to putbit, msk.c:122-126), with lvl = cabsf(v) from before the normalisation;
  * MskPhi, MskDf, MskLvlSum as uint64 patterns, MskClk and the 22 floats of inb[] as uint32 patterns;
  * MskS, idx, outbits, nbits, Acarsstate, MskBitCount, blk_len, blk_err, soh_back;
  * the text under assembly (acg_get_block_text) while in TXT;
  * the drained blocks with end_bit, end_sample, soh_sample and the level's bit pattern.

The one legitimate source of a difference is the mixer's sin/cos (the device's table + series against glibc's cexp); the inputs
(tests/msk_exact_inputs.py) are chosen such that it cannot show, and tests/test_msk_exact_inputs.py asserts that on the CPU: at
every (phase, sample) pair of every run below, the float products of the device's sin/cos model are cexp's.

A failure names the kernel, the call, the channel, the field and both values in hex of the FIRST difference in time order (within a
call: the earliest bit record, then the state the call left behind)."""
import contextlib
import ctypes as C
import faulthandler
import struct

import numpy as np
import pytest

import msk_exact_inputs as X

pytestmark = pytest.mark.gpu

STEP_LIMIT_S = 120          # one GPU step (a decoder's creation, a call with its read-back): far above the milliseconds it takes


@contextlib.contextmanager
def limit(seconds=STEP_LIMIT_S):
    """a GPU step that hangs ends the process (with a traceback) instead of the suite waiting on it; nothing is tried again"""
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def D():
    from acarsdec_amd import decoder
    from acarsdec_amd import _capi as K
    assert K.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return decoder


# (name, ACG_MSK_LPC, ACG_MSK_NOLEAN, ACG_MSK_CUS or None, schedule, two-wave kernel of the lab build, bit-log settings)
# msk_lean_kernel alone has an instantiation without the log; it and only it runs in both workgroup shapes in test_gpu_lean_chains.py
KERNELS = [
    ("lean8", 8, 0, None, X.EVEN, False, (True, False)),
    ("lean8-cus0", 8, 0, 0, X.EVEN, False, (True, False)),
    ("lean4", 4, 0, None, X.EVEN, False, (True, False)),
    ("lean4-cus0", 4, 0, 0, X.EVEN, False, (True, False)),
    ("inline8", 8, 1, None, X.EVEN, False, (True,)),                # msk_demod_kernel
    ("inline2", 2, 0, None, X.EVEN, False, (True,)),
    ("inline1", 1, 0, None, X.EVEN, False, (True,)),
    ("inline8-ragged", 8, 0, None, X.RAGGED, False, (True,)),       # its scalar-refill shape: call lengths that are no multiples of 32
    ("two-wave", 8, 0, None, X.EVEN, True, (True,)),                # msk_demod2_kernel
]
PLANTED = [k for k in KERNELS if k[4] is X.EVEN]


def select(tune, kernel):
    name, lpc, nolean, cus, _, split, _ = kernel
    tune("ACG_MSK_LPC", str(lpc), lab=split)
    if nolean:
        tune("ACG_MSK_NOLEAN", "1")
    if cus is not None:
        tune("ACG_MSK_CUS", str(cus))
    if split:
        tune("ACG_MSK_SPLIT", "1", lab=True)             # (the two-wave kernel exists in the lab build only)


def f32_bits(a):
    """bit patterns of float32 values, -0 folded onto +0"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = a.view(np.uint32).copy()
    b[a == 0] = 0
    return b


def hex64(v):
    return "0x%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]


def hex32(v):
    return "0x%08x" % struct.unpack("<I", struct.pack("<f", v))[0]


def chan_state(K, s):
    """the oracle's channel as the public state record (acg_chan_state)"""
    t, c = K.ChanState(), s.c
    t.MskPhi, t.MskDf, t.MskLvlSum, t.MskClk = c.MskPhi, c.MskDf, c.MskLvlSum, c.MskClk
    t.MskBitCount, t.MskS, t.idx = c.MskBitCount, c.MskS, c.idx
    for j in range(22):
        t.inb[j] = c.inb[j]
    t.outbits, t.nbits, t.Acarsstate, t.blk_len, t.blk_err, t.soh_back = c.outbits, c.nbits, c.Acarsstate, c.blk_len, c.blk_err, s.soh_back
    return t


def differences(dec, K, want, bitlog, stamps):
    """[(time key, channel, field, got, want)] between the decoder after its last call and the oracle's row `want`"""
    nch = len(want)
    st = (K.ChanState * nch)()
    dec._chk(dec.L.acg_get_state_n(dec.ctx, 0, nch, st))
    out = []
    late = 1 << 30                                                       # the state a call leaves behind sorts after its bits
    if bitlog:
        cnt, vo, lvl = dec.bits_all()
        assert cnt.max() <= dec.bit_cap
    for ch, s in enumerate(want):
        g, c = st[ch], s.c
        if bitlog:
            if int(cnt[ch]) != len(s.vo):
                out.append((min(int(cnt[ch]), len(s.vo)), ch, "bit count", str(int(cnt[ch])), str(len(s.vo))))
            n = min(int(cnt[ch]), len(s.vo))
            for name, got, ref in (("vo", vo[ch, :n], s.vo[:n]), ("lvl", lvl[ch, :n], s.lvl[:n])):
                bad = np.flatnonzero(f32_bits(got) != f32_bits(ref))
                if len(bad):
                    i = int(bad[0])
                    out.append((i, ch, "bit record %d of the call, %s" % (i, name), hex32(got[i]), hex32(ref[i])))
        for name in ("MskPhi", "MskDf", "MskLvlSum"):
            if hex64(getattr(g, name)) != hex64(getattr(c, name)):
                out.append((late, ch, name, hex64(getattr(g, name)), hex64(getattr(c, name))))
        if hex32(g.MskClk) != hex32(c.MskClk):
            out.append((late, ch, "MskClk", hex32(g.MskClk), hex32(c.MskClk)))
        for j in range(22):
            if hex32(g.inb[j]) != hex32(c.inb[j]):
                out.append((late, ch, "inb[%d]" % j, hex32(g.inb[j]), hex32(c.inb[j])))
        for name in ("MskS", "idx", "outbits", "nbits", "Acarsstate", "MskBitCount", "blk_len", "blk_err"):
            if int(getattr(g, name)) != int(getattr(c, name)):
                out.append((late, ch, name, hex(int(getattr(g, name))), hex(int(getattr(c, name)))))
        if int(g.soh_back) != s.soh_back:
            out.append((late, ch, "soh_back", hex(int(g.soh_back)), hex(s.soh_back)))
        if int(g.Acarsstate) == X.TXT and int(c.Acarsstate) == X.TXT:
            buf = (C.c_ubyte * 256)()
            dec._chk(dec.L.acg_get_block_text(dec.ctx, ch, buf))
            if bytes(buf[: c.blk_len]) != s.text:
                out.append((late, ch, "text under assembly", bytes(buf[: c.blk_len]).hex(), s.text.hex()))
    got = {}
    for f in dec.drain_frames():
        got.setdefault(int(f.chn), []).append(X.frame_key(f, stamps))
    for ch, s in enumerate(want):
        ref = [X.frame_key(f, stamps) for f in s.blocks]
        if got.get(ch, []) != ref:
            out.append((late, ch, "blocks (chn, len, err, crc, txt, lvl%s)" % (", end_bit, end_sample, soh_sample" if stamps else ""),
                        repr(got.get(ch, [])), repr(ref)))
    assert set(got) <= set(range(nch))
    return sorted(out)


def check(dec, K, want, kernel, bitlog, where, call, stamps=True):
    with limit():
        diff = differences(dec, K, want, bitlog, stamps)
    if diff:
        _, ch, field, got, ref = diff[0]
        raise AssertionError("%s kernel, bit log %d, %s, call %d, channel %d (%s): %s is %s, the oracle has %s  [%d differences in this call]"
                             % (kernel[0], bitlog, where, call, ch, X.KIND_NAMES[ch % X.NKINDS], field, got, ref, len(diff)))


def plant(dec, K, states):
    """the oracle's state of every channel into the decoder (acg_set_state_n; the text under assembly where there is one)"""
    nch = len(states)
    st = (K.ChanState * nch)(*[chan_state(K, s) for s in states])
    with limit():
        dec._chk(dec.L.acg_set_state_n(dec.ctx, 0, nch, st))
        for ch, s in enumerate(states):
            assert s.c.Acarsstate != X.CRC2
            if s.c.Acarsstate in (X.TXT, X.CRC1):
                dec._chk(dec.L.acg_set_block_text(dec.ctx, ch, (C.c_ubyte * 256)(*bytes(s.c.blk_txt))))


# ---- the mixer's sin/cos ------------------------------------------------------------------------------------------------------------
def test_device_sincos_is_its_cpu_model_at_every_visited_phase(D):
    """What the loop keeps of the mixer's sin/cos are two float products, and those cannot show an error of 1e-13 in the sine (a
    series term dropped from sincos_tab_rotate moves none of the 460 000 products of this file: tried).  So the function itself
    (msk_common.h sincos_tab through acg_selftest_sincos) is held to its CPU model (tests/sincos_model.h, whose accuracy
    tests/test_host_logic.py bounds against long-double libm): the same doubles, bit for bit, at every phase the runs below visit
    -- the negative ones of df = -1 included -- and at the table's nodes and midpoints."""
    from acarsdec_amd import _capi as K
    x = np.concatenate([X.visited_phases(), np.arange(-128, 257) * (np.pi / 64), (np.arange(-128, 256) + 0.5) * (np.pi / 64), [X.TWO_PI, 0.0]])
    s, c = np.zeros_like(x), np.zeros_like(x)
    with limit():
        assert K.load().acg_selftest_sincos(x.ctypes.data, s.ctypes.data, c.ctypes.data, x.size) == 0
    ms, mc = X.model_sincos(x)
    for name, got, ref in (("sin", s, ms), ("cos", c, mc)):
        bad = np.flatnonzero(got.view(np.uint64) != ref.view(np.uint64))
        assert len(bad) == 0, "%s(%r): the device has %s, the model %s  [%d of %d differ]" % (
            name, x[bad[0]], hex64(got[bad[0]]), hex64(ref[bad[0]]), len(bad), x.size)
    assert x.size > 2 * X.NCH * sum(X.EVEN) // 2 and x.min() < -2 * np.pi


# ---- a. free running ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [X.NCH, 1])
@pytest.mark.parametrize("kernel", KERNELS, ids=[k[0] for k in KERNELS])
def test_free_running_demodulator_is_the_oracle_after_every_call(D, tune, kernel, nch):
    from acarsdec_amd import _capi as K
    select(tune, kernel)
    x = X.tracks()[:nch]
    sched = kernel[4]
    want = X.oracle_run(sched, nch=nch)
    for bitlog in kernel[6]:
        with limit():
            dec = D.Decoder(nch, max_blocks=8, bitlog=bitlog, lab=kernel[5])
        a0 = 0
        for i, n in enumerate(sched):
            with limit():
                dec.demod_msk(x[:, a0:a0 + n])
                dec.sync()
            check(dec, K, want[i], kernel, bitlog, "%d channels, free run" % nch, i)
            a0 += n
        dec.close()


# ---- b. planted -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", PLANTED, ids=[k[0] for k in PLANTED])
def test_decoder_brought_to_the_oracles_state_goes_on_as_the_oracle(D, tune, kernel):
    """At every cut point (the ends of the EVEN calls and the extra cuts that reach every framing state but CRC2, which the public
    state cannot express: tests/test_msk_exact_inputs.py) a fresh decoder is given the oracle's state through acg_set_state_n and
    acg_set_block_text, then runs one call of 32, 64, 96 and 128 samples from there (the state is brought back in front of each).
    The time stamps are left out: a fresh decoder counts its samples from 0."""
    from acarsdec_amd import _capi as K
    select(tune, kernel)
    x = X.tracks()
    for bitlog in kernel[6]:
        for t in X.cut_points():
            state, calls = X.oracle_cut(t)
            with limit():
                dec = D.Decoder(X.NCH, max_blocks=8, bitlog=bitlog, lab=kernel[5])
            for n in X.SHORT:
                plant(dec, K, state)
                with limit():
                    dec.demod_msk(x[:, t:t + n])
                    dec.sync()
                check(dec, K, calls[n], kernel, bitlog, "state of sample %d planted" % t, n, stamps=False)
            dec.close()


@pytest.mark.parametrize("kernel", PLANTED, ids=[k[0] for k in PLANTED])
def test_planted_wrap_edges_and_out_of_lock_steps_are_the_oracles(D, tune, kernel):
    """test_gpu_lean_chains.py's plants -- a phase wrap on the `>=` edge at each of the six steps of a period and one ulp below it,
    df = -1 (a negative step: the phase runs below -2 pi, outside the range the table reduction was written for) and df = +3 (the
    clock fires on the first sample) -- written into the decoder AND into the oracle in front of each of 16 short calls, every
    plant on every planted channel: held to the reference, not only kernel to kernel."""
    from acarsdec_amd import _capi as K
    select(tune, kernel)
    x = X.tracks()
    want = X.oracle_run(X.PLANT_CALLS, planted=True)
    for bitlog in kernel[6]:
        with limit():
            dec = D.Decoder(X.NCH, max_blocks=8, bitlog=bitlog, lab=kernel[5])
        a0 = 0
        st = (K.ChanState * X.NCH)()
        for i, n in enumerate(X.PLANT_CALLS):
            with limit():
                dec._chk(dec.L.acg_get_state_n(dec.ctx, 0, X.NCH, st))
                for ch in range(X.NCH):
                    p = X.plant_for(i, ch)
                    if p is not None:
                        st[ch].MskPhi, st[ch].MskDf, st[ch].MskClk = p
                dec._chk(dec.L.acg_set_state_n(dec.ctx, 0, X.NCH, st))
                dec.demod_msk(x[:, a0:a0 + n])
                dec.sync()
            check(dec, K, want[i], kernel, bitlog, "plants in front of every call", i)
            a0 += n
        dec.close()
