"""The down-converter at any input rate on the GPU (acg_set_input_rate, acg_process_rate_dev, acg_feed_rate_host; the kernel:
csrc/fir_rate.hip): every output against the float64-exact value of the definition (tests/rate_ref.py), pieces against the
whole bit for bit, the integer case against the existing path, three ACARS channels end to end, the refusals.  Runs on the GPU
box only (-m gpu).

Tolerances, the project's written ones (rate_ref.bar): CU8, CS8, CS16 1e-5 |x| + 1e-6; CF32 1e-5 |x| + 1e-6 max|x| over the
channel's windows.
"""
import ctypes as C

import numpy as np
import pytest

import format_ref as R
import iq_format_ref as Q
import rate_ref as RR

pytestmark = pytest.mark.gpu

NS = 6                              # streams, one channel each
FIRST, SECOND = 1061, 517           # windows of the two calls: not whole tiles, not a multiple of Q


@pytest.fixture(scope="module")
def D():
    from acarsdec_amd import decoder
    from acarsdec_amd import _capi as K
    assert K.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return decoder


@pytest.fixture(scope="module")
def K():
    from acarsdec_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def S():
    from acarsdec_amd import synth
    return synth


def to_device(x, pad=48, shift=0):
    """rows of interleaved values on the device, `pitch` bytes apart: the row rounded up to 16 bytes plus `pad`, the gaps filled
    with a byte that is no sample of the input.  Returns (tensor, pitch, samples per row)."""
    import torch
    x = np.ascontiguousarray(x)
    ns, rowb = x.shape[0], x.shape[1] * x.itemsize
    pitch = ((rowb + 15) & ~15) + pad
    buf = np.full(ns * pitch + shift, 0x5A, dtype=np.uint8)
    for s in range(ns):
        buf[shift + s * pitch: shift + s * pitch + rowb] = x[s].view(np.uint8)
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 16 == 0
    return t[shift:], pitch, x.shape[1] // 2


def all_dm(dec, nch, n):
    return np.stack([dec.dm(c, n) for c in range(nch)])


def check_exact(got, ex, fmt, what):
    r = np.abs(got.astype(np.float64) - ex) / RR.bar(ex, fmt)
    c, m = np.unravel_index(int(r.argmax()), r.shape)
    assert r.max() <= 1.0, "%s: %.3f of the bar at channel %d window %d: %r, exact %r" % (what, r.max(), c, m, got[c, m], ex[c, m])
    return float(r.max())


def scrambled(rng, n):
    m = rng.permutation(n).astype(np.int32)
    while np.array_equal(m, np.arange(n)):
        m = rng.permutation(n).astype(np.int32)
    return m


def timing_launches(dec):
    ms, n = C.c_double(0), C.c_int(0)
    dec._chk(dec.L.acg_get_timing(dec.ctx, C.byref(ms), C.byref(n), None, None))
    return n.value


# ------------------------------------------------------------------------------------ every output against the exact value
CASE_RATES = [2048000, 1024000, 31250, 1999999, 3999999]


@pytest.mark.parametrize("rate", CASE_RATES)
@pytest.mark.parametrize("fmt", RR.FORMATS)
def test_every_output_against_the_exact_value(D, fmt, rate):
    """Six streams, one channel each, through a scrambled stream map; make_taps' tables.  The first call presents 1061 windows and
    all but one sample of the next, the second continues the grid at k0 = 1061 on a different input that ends with its last
    window (so the sample behind a short last window is not the caller's).  2 048 000: L in {163, 164}; 1 024 000: {81, 82};
    31 250: L alternates 2 and 3; 1 999 999: Q = 12 500 and window 0 is the short one; 3 999 999: decim 320, several slices."""
    M = RR.decim(rate)
    rng = np.random.default_rng(rate % 100003 + len(fmt))
    taps = RR.make_taps(D, rate, NS, np.random.default_rng(rate % 1009))
    dec = D.Decoder(NS, decim=M, nstreams=NS, max_blocks=2, bitlog=False)
    dec.set_taps(taps)
    dec.set_input_rate(rate)
    worst = 0.0
    k0 = 0
    for call, nwin in enumerate((FIRST, SECOND)):
        extra = RR.span(rate, k0 + nwin, 1) - 1 if call == 0 else 0
        x = RR.make_input(fmt, rate, NS, k0, nwin, rng, k=call, extra=extra)
        smap = scrambled(rng, NS)
        dec.set_channel_streams(smap)
        t, pitch, ns = to_device(x)
        got_n, used = dec.process_rate(RR.capi_fmt(fmt), t, ns, pitch)
        assert (got_n, used) == (nwin, RR.span(rate, k0, nwin)), (fmt, rate, call, got_n, used)
        assert ns - used == extra
        got = all_dm(dec, NS, nwin)
        ex = np.stack([RR.exact(fmt, x[smap[c]], rate, taps[c], k0, nwin) for c in range(NS)])
        worst = max(worst, check_exact(got, ex, fmt, "%s at %d, call %d" % (fmt, rate, call)))
        k0 += nwin
    dec.close()
    print("LEDGER rate %s R=%d: worst err/bar %.3f" % (fmt, rate, worst))


# ------------------------------------------------------------------------------------ pieces equal the whole
@pytest.mark.parametrize("fmt", [RR.CU8, RR.CF32])
def test_feed_in_pieces_equals_one_device_call_bit_for_bit(D, S, fmt):
    """acg_feed_rate_host at 2 048 000 Hz, three streams: pieces of 1, L_0 - 1, 3 decim + 7, 5 samples and the rest -- dm of every
    launch and the drained blocks are those of one acg_process_rate_dev call over the same input.  The same kernel, the same
    order of additions."""
    rate, ns, nblk = 2048000, 3, 4
    nout, M = nblk * 1024, RR.decim(rate)
    rows, taps, frames = [], [], []
    for s in range(ns):
        row, t3, fr = RR.acars_stream(D, S, fmt, rate, nout, 70 + 3 * s + len(fmt), nch=1)
        rows.append(row)
        taps.append(t3[0])
        frames.append(fr[0])
    x, taps = np.stack(rows), np.stack(taps)
    total = RR.start(rate, nout)
    assert x.shape[1] == 2 * total and sum(len(f) for f in frames) >= ns

    ref = D.Decoder(ns, decim=M, nstreams=ns, max_blocks=nblk)
    ref.set_taps(taps)
    ref.set_input_rate(rate)
    t, pitch, n = to_device(x)
    assert ref.process_rate(RR.capi_fmt(fmt), t, n, pitch) == (nout, total)
    want_dm = all_dm(ref, ns, nout)
    want = [D.frame_tuple(f) for f in ref.drain_frames()]
    ref.close()
    assert len(want) >= ns
    ex = np.stack([RR.exact(fmt, x[c], rate, taps[c], 0, nout) for c in range(ns)])
    check_exact(want_dm, ex, fmt, "device call " + fmt)

    dec = D.Decoder(ns, decim=M, nstreams=ns, max_blocks=nblk)
    dec.set_taps(taps)
    dec.set_input_rate(rate)
    got, pos, launches = [], 0, 0
    for piece in (1, RR.span(rate, 0, 1) - 1, 3 * M + 7, 5, total):
        piece = min(piece, total - pos)
        w0, w1 = RR.windows_fit(rate, 0, pos), RR.windows_fit(rate, 0, pos + piece)
        dec.feed_rate(RR.capi_fmt(fmt), x[:, 2 * pos: 2 * (pos + piece)])
        pos += piece
        if w1 > w0:
            launches += 1
            dm = all_dm(dec, ns, w1 - w0)
            assert np.array_equal(dm.view(np.uint32), want_dm[:, w0: w1].view(np.uint32)), (fmt, w0, w1)
        got += [D.frame_tuple(f) for f in dec.drain_frames()]
    assert pos == total and launches == 3
    assert sorted(got) == sorted(want)
    dec.close()


# ------------------------------------------------------------------------------------ Q = 1 meets the existing path
@pytest.mark.parametrize("fmt", [RR.CS16, RR.CF32])
def test_integer_rate_meets_the_existing_path(D, S, fmt):
    """R = 2 500 000: the rate path with rate_taps, and acg_process_samples_dev at M = 200 with soapy_taps, are each within the
    bar of their exact value, and both deliver the same blocks."""
    rate, M, nblk = 2500000, 200, 4
    nout = nblk * 1024
    assert RR.pq(rate) == (200, 1)
    row, rtaps, frames = RR.acars_stream(D, S, fmt, rate, nout, 41 + len(fmt))
    fc = D.choose_fc(RR.FREQS3, M)[0]
    staps = np.stack([D.soapy_taps(float(f), fc, M) for f in RR.FREQS3])
    x = row[None, :]
    t, pitch, n = to_device(x)
    smap = np.zeros(3, dtype=np.int32)
    out = {}
    for path in ("rate", "samples"):
        dec = D.Decoder(3, decim=M, nstreams=1, max_blocks=nblk)
        dec.set_channel_streams(smap)
        if path == "rate":
            dec.set_taps(rtaps)
            dec.set_input_rate(rate)
            assert dec.process_rate(RR.capi_fmt(fmt), t, n, pitch) == (nout, nout * M)
            ex = np.stack([RR.exact(fmt, row, rate, rtaps[c], 0, nout) for c in range(3)])
        else:
            dec.set_taps(staps)
            dec.process_samples(RR.capi_fmt(fmt), t, nblk, pitch, 0)
            ex = np.stack([(R.exact_cs16 if fmt == RR.CS16 else lambda *a: Q.exact(Q.CF32, *a))(row, M, staps[c], nout) for c in range(3)])
        check_exact(all_dm(dec, 3, nout), ex, fmt, "%s path %s" % (path, fmt))
        out[path] = sorted(D.frame_tuple(f) for f in dec.drain_frames())
        dec.close()
    assert out["rate"] == out["samples"] and len(out["rate"]) >= 3 and sum(len(f) for f in frames) >= 3


# ------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("fmt", [RR.CU8, RR.CF32])
def test_end_to_end_three_channels_on_one_stream(D, O, S, K, fmt):
    """Three synthetic ACARS channels on one stream at 2 048 000 Hz (tests/test_rate_ref.py holds the fixtures decodable): every
    transmitted frame is delivered field for field by acg_drain_msgs, and the oracle's demodulator on the GPU's own dm queues
    the same blocks."""
    rate, nout, nch = RR.E2E_RATE, RR.E2E_NOUT, 3
    row, taps, frames = RR.acars_stream(D, S, fmt, rate, nout, RR.E2E_SEED[fmt])
    dec = D.Decoder(nch, decim=RR.decim(rate), nstreams=1, max_blocks=nout // 1024, repair=True)
    dec.set_taps(taps)
    dec.set_channel_streams(np.zeros(nch, dtype=np.int32))
    dec.set_input_rate(rate)
    t, pitch, n = to_device(row[None, :])
    assert dec.process_rate(RR.capi_fmt(fmt), t, n, pitch) == (nout, RR.start(rate, nout))
    msgs = dec.drain_msgs()
    dm = np.zeros((nch, nout), dtype=np.float32)
    assert dec.L.acg_read_dm_n(dec.ctx, 0, nch, dm.ctypes.data, nout, nout) == K.OK
    dec.close()
    ex = np.stack([RR.exact(fmt, row, rate, taps[c], 0, nout) for c in range(nch)])
    check_exact(dm, ex, fmt, "end to end " + fmt)
    for c in range(nch):
        mine = [m for m in msgs if m.chn == c]
        assert len(mine) == len(frames[c]) >= 1, (c, len(mine), len(frames[c]))
        for m, fr in zip(mine, frames[c]):
            f = RR.frame_fields(fr)
            assert m.err == 0 and m.mode == f["mode"] and m.addr == f["addr"] and m.ack == b"!" and m.label == f["label"]
            assert m.bid == f["bid"] and m.down not in (b"\x00", 0) and m.no == f["no"] and m.fid == f["fid"]
            assert bytes(m.txt[: m.txt_len]) == f["txt"] and m.be == b"\x03"
        ch = O.Channel(c)
        ch.demod(dm[c])
        orc = [O.msg_split(O.blk_process(f)) for f in ch.frames]
        assert [O.msg_tuple(m) for m in mine] == [O.msg_tuple(m) for m in orc], c


# ------------------------------------------------------------------------------------ refusals and state
def test_refusals_and_state(D, K):
    """After every refusal acg_last_error names the rule and no down-converter launch was made."""
    import torch
    rate, M, nblk = 2048000, 164, 1
    rng = np.random.default_rng(3)
    L = K.load()

    def refused(dec, rc, code, word):
        assert rc == code, (rc, code, word)
        assert word in L.acg_last_error(dec.ctx).decode(), (word, L.acg_last_error(dec.ctx))
        assert timing_launches(dec) == 0

    # a context whose decim is not the rate's
    dec = D.Decoder(3, decim=160, nstreams=3, max_blocks=nblk, timing=True)
    refused(dec, L.acg_set_input_rate(dec.ctx, rate), K.EINVAL, "acg_rate_decim")
    nw, used = C.c_int(-1), C.c_size_t(7)
    buf = torch.zeros(3 * 1024 * 160 * 4 + 64, dtype=torch.uint8, device="cuda")
    refused(dec, L.acg_process_rate_dev(dec.ctx, K.FMT_CS16, buf.data_ptr(), 1024 * 160 * 4, 1000, None, C.byref(nw), C.byref(used)),
            K.ESTATE, "no input rate")
    assert (nw.value, used.value) == (0, 0)
    # ... and set_input_rate(0) on a context that never had one changes nothing: the CS16 path's bits, here and below
    x16 = R.make_input(R.CS16, 160, 3, 1024, rng)
    t16 = torch.from_numpy(x16.copy()).cuda()
    taps160 = R.make_taps(D, R.CS16, 160, 3, np.random.default_rng(4))
    dec.set_taps(taps160)
    dec.process_samples(K.FMT_CS16, t16, 1, x16.shape[1] * 2, 0)
    fresh = all_dm(dec, 3, 1024)
    assert timing_launches(dec) == 1
    dec.close()

    dec = D.Decoder(3, decim=M, nstreams=3, max_blocks=nblk, timing=True)
    taps = RR.make_taps(D, rate, 3, np.random.default_rng(5))
    dec.set_taps(taps)
    dec.set_input_rate(rate)
    nwin = 300
    x = RR.make_input(RR.CS16, rate, 3, 0, nwin, rng)
    t, pitch, n = to_device(x)
    fmt = K.FMT_CS16
    call = lambda f, ptr, p, ns: L.acg_process_rate_dev(dec.ctx, f, ptr, p, ns, None, C.byref(nw), C.byref(used))
    refused(dec, call(K.FMT_S16_SPLIT, t.data_ptr(), pitch, n), K.EINVAL, "fix their own rates")
    refused(dec, call(K.FMT_F32_REAL, t.data_ptr(), pitch, n), K.EINVAL, "fix their own rates")
    refused(dec, L.acg_feed_rate_host(dec.ctx, K.FMT_S16_SPLIT, x.ctypes.data, n, n), K.EINVAL, "fix their own rates")
    refused(dec, call(99, t.data_ptr(), pitch, n), K.EINVAL, "unknown sample format")
    refused(dec, call(fmt, t.data_ptr() + 4, pitch, n - 8), K.EINVAL, "16-byte aligned")
    refused(dec, call(fmt, t.data_ptr(), pitch + 8, n), K.EINVAL, "16-byte aligned")
    refused(dec, call(fmt, t.data_ptr(), ((4 * n + 15) & ~15) - 16, n), K.EINVAL, "pitch smaller than a row")
    # every window-aligned entry point while a rate is set
    u8 = torch.zeros(3 * 1024 * M * 2, dtype=torch.uint8, device="cuda")
    h8 = np.zeros(3 * 1024 * M * 2, dtype=np.uint8)
    word = "an input rate is set"
    refused(dec, L.acg_process_iq_u8_dev(dec.ctx, u8.data_ptr(), 1024 * M * 2, 1, None), K.ESTATE, word)
    refused(dec, L.acg_process_iq_u8_host(dec.ctx, h8.ctypes.data, 1024 * M * 2, 1), K.ESTATE, word)
    refused(dec, L.acg_fir_only_dev(dec.ctx, u8.data_ptr(), 1024 * M * 2, 1, None), K.ESTATE, word)
    refused(dec, L.acg_process_samples_dev(dec.ctx, fmt, u8.data_ptr(), 1024 * M * 2, 0, 1, None), K.ESTATE, word)
    refused(dec, L.acg_feed_samples_host(dec.ctx, fmt, h8.ctypes.data, None, 100, 100), K.ESTATE, word)
    # process_rate while the feed carries samples; the rate cannot change either
    dec.feed_rate(fmt, x[:, : 2 * 100])
    assert timing_launches(dec) == 0                              # 100 samples: no whole window
    refused(dec, call(fmt, t.data_ptr(), pitch, n), K.ESTATE, "partial window")
    refused(dec, L.acg_set_input_rate(dec.ctx, 0), K.ESTATE, "carries samples")
    # acg_reset drops the carried samples and restarts the grid at window 0
    ex = np.stack([RR.exact(RR.CS16, x[c], rate, taps[c], 0, nwin) for c in range(3)])
    for again in range(2):
        dec.reset()
        assert dec.process_rate(fmt, t, n, pitch) == (nwin, RR.span(rate, 0, nwin))
        check_exact(all_dm(dec, 3, nwin), ex, RR.CS16, "after reset %d" % again)
    assert timing_launches(dec) == 2
    # without the reset the same input is taken as windows 300 ..: another grid position, another length pattern
    got_n, got_used = dec.process_rate(fmt, t, n, pitch)
    assert (got_n, got_used) == (RR.windows_fit(rate, nwin, n), RR.span(rate, nwin, RR.windows_fit(rate, nwin, n)))
    assert timing_launches(dec) == 1
    dec.close()

    # set_input_rate(0) brings back the existing CS16 path with the bits of a fresh context
    dec = D.Decoder(3, decim=160, nstreams=3, max_blocks=nblk, timing=True)
    dec.set_taps(taps160)
    dec.set_input_rate(2000000)
    assert L.acg_process_samples_dev(dec.ctx, fmt, t16.data_ptr(), x16.shape[1] * 2, 0, 1, None) == K.ESTATE
    dec.set_input_rate(0)
    dec.process_samples(fmt, t16, 1, x16.shape[1] * 2, 0)
    assert np.array_equal(all_dm(dec, 3, 1024).view(np.uint32), fresh.view(np.uint32))
    dec.close()
