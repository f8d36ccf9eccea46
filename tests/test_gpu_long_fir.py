"""Channel filters over several windows on the GPU (acg_set_channel_filter on the rate path; the kernel: csrc/fir_long.hip): every
output against the float64-exact value of the definition (tests/long_ref.py), pieces against the whole bit for bit, the history
rules, three ACARS channels beside a strong carrier end to end -- decoded with the filter, lost without it -- and the refusals.
Runs on the GPU box only (-m gpu).

The tolerance is long_ref.bar: derived from the kernel's fixed order of additions, not measured; tests/test_long_ref.py shows
that wrong kernels exceed it.
"""
import ctypes as C

import numpy as np
import pytest

import rate_ref as RR
import long_ref as LR

pytestmark = pytest.mark.gpu

NS = 6                              # streams, one channel each
FIRST, SECOND = 203, 131            # windows of the two calls: tiles that are not whole, a halo across the call


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


def to_device(x, pad=48):
    """rows of interleaved values on the device, `pitch` bytes apart: the row rounded up to 16 bytes plus `pad`, the gaps filled
    with a byte that is no sample of the input.  Returns (tensor, pitch, samples per row)."""
    import torch
    x = np.ascontiguousarray(x)
    ns, rowb = x.shape[0], x.shape[1] * x.itemsize
    pitch = ((rowb + 15) & ~15) + pad
    buf = np.full(ns * pitch, 0x5A, dtype=np.uint8)
    for s in range(ns):
        buf[s * pitch: s * pitch + rowb] = x[s].view(np.uint8)
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 16 == 0
    return t, pitch, x.shape[1] // 2


def all_dm(dec, nch, n):
    return np.stack([dec.dm(c, n) for c in range(nch)])


def against_model(got, fmt, rows_h, M, J, taps, nzero, what):
    """got [nch, nwin] against long_ref.exact of rows_h[c] (the channel's row behind its history); the worst err / bar"""
    nwin = got.shape[1]
    worst = 0.0
    for c in range(got.shape[0]):
        ex = LR.exact(fmt, rows_h[c], M, J, taps[c], nwin, nzero)
        r = np.abs(got[c].astype(np.float64) - ex) / LR.bar(fmt, rows_h[c], M, J, taps[c], nwin, ex, nzero)
        m = int(r.argmax())
        assert r.max() <= 1.0, "%s: %.3f of the bar at channel %d window %d: %r, exact %r" % (what, r.max(), c, m, got[c, m], ex[m])
        worst = max(worst, float(r.max()))
    return worst


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
SHAPES = [(RR.CU8, 160, 4), (RR.CS8, 160, 2), (RR.CS16, 200, 3), (RR.CF32, 320, 4), (RR.CF32, 8, 4)]


@pytest.mark.parametrize("kind", ["unit", "kaiser"])
@pytest.mark.parametrize("fmt,M,J", SHAPES)
def test_every_output_against_the_exact_value(D, fmt, M, J, kind):
    """Six streams, one channel each, through a scrambled stream map (another one per call).  Two calls of 203 and 131 windows
    on different device buffers, the first presented with all but one sample of a further window: tiles that are not whole, a
    halo across the call, history from a buffer the caller has since replaced.  M = 320 complex float32 goes through in four
    slices; at M = 8 a window is one chunk."""
    import torch
    rate = 12500 * M
    rng = np.random.default_rng(1000 * M + 10 * J + len(fmt))
    taps = LR.tap_tables(kind, rate, J, NS, np.random.default_rng(M + J), D)
    dec = D.Decoder(NS, decim=M, nstreams=NS, max_blocks=1, bitlog=False)
    dec.set_taps(RR.make_taps(D, rate, NS, np.random.default_rng(3)))        # the one-window table: unused while a filter is on
    dec.set_input_rate(rate)
    dec.set_channel_filter(taps)
    worst, seen, k0 = 0.0, [], 0
    for call, nwin in enumerate((FIRST, SECOND)):
        extra = M - 1 if call == 0 else 0
        x = RR.make_input(fmt, rate, NS, k0, nwin, rng, k=call, extra=extra)
        smap = scrambled(rng, NS)
        dec.set_channel_streams(smap)
        t, pitch, ns = to_device(x)
        assert dec.process_rate(RR.capi_fmt(fmt), t, ns, pitch) == (nwin, nwin * M), (fmt, M, J, call)
        got = all_dm(dec, NS, nwin)
        t.fill_(0x5A)                                                        # the caller's buffer is gone: the history is the context's
        torch.cuda.synchronize()
        rows_h = [LR.with_history([p[smap[c]] for p in seen], x[smap[c]][: 2 * nwin * M], M, J) for c in range(NS)]
        worst = max(worst, against_model(got, fmt, rows_h, M, J, taps, J - 1 if call == 0 else 0, "%s M=%d J=%d %s, call %d" % (fmt, M, J, kind, call)))
        seen.append(x[:, : 2 * nwin * M])
        k0 += nwin
    dec.close()
    print("LEDGER long %s M=%d J=%d %s: worst err/bar %.3f" % (fmt, M, J, kind, worst))


# ------------------------------------------------------------------------------------ pieces equal the whole
@pytest.mark.parametrize("fmt", [RR.CU8, RR.CF32])
def test_feed_in_pieces_equals_one_device_call_bit_for_bit(D, S, fmt):
    """acg_feed_rate_host at 2.0 Msps, three streams, J = 4: pieces of 1 sample, M - 1, M (one window: fewer than J - 1), 3 M + 7,
    5 and the rest -- dm of every launch and the drained blocks are those of one acg_process_rate_dev call over the same input."""
    rate, ns, nblk, J = 2000000, 3, 4, 4
    nout, M = nblk * 1024, 160
    rows, taps, frames = [], [], []
    for s in range(ns):
        row, _t, fr = RR.acars_stream(D, S, fmt, rate, nout, 170 + 3 * s + len(fmt), nch=1)
        fc = D.choose_fc(RR.FREQS3, M)[0]
        rows.append(row)
        taps.append(D.channel_filter_taps(rate, RR.FREQS3[0] - fc, J))
        frames.append(fr[0])
    x, taps = np.stack(rows), np.stack(taps)
    total = nout * M
    assert x.shape[1] == 2 * total and sum(len(f) for f in frames) >= ns

    ref = D.Decoder(ns, decim=M, nstreams=ns, max_blocks=nblk)
    ref.set_input_rate(rate)
    ref.set_channel_filter(taps)
    t, pitch, n = to_device(x)
    assert ref.process_rate(RR.capi_fmt(fmt), t, n, pitch) == (nout, total)
    want_dm = all_dm(ref, ns, nout)
    want = [D.frame_tuple(f) for f in ref.drain_frames()]
    ref.close()
    assert len(want) >= ns
    against_model(want_dm, fmt, [LR.with_history([], x[c], M, J) for c in range(ns)], M, J, taps, J - 1, "device call " + fmt)

    dec = D.Decoder(ns, decim=M, nstreams=ns, max_blocks=nblk)
    dec.set_input_rate(rate)
    dec.set_channel_filter(taps)
    got, pos, launches = [], 0, 0
    for piece in (1, M - 1, M, 3 * M + 7, 5, total):
        piece = min(piece, total - pos)
        w0, w1 = pos // M, (pos + piece) // M
        dec.feed_rate(RR.capi_fmt(fmt), x[:, 2 * pos: 2 * (pos + piece)])
        pos += piece
        if w1 > w0:
            launches += 1
            dm = all_dm(dec, ns, w1 - w0)
            assert np.array_equal(dm.view(np.uint32), want_dm[:, w0: w1].view(np.uint32)), (fmt, w0, w1)
        got += [D.frame_tuple(f) for f in dec.drain_frames()]
    assert pos == total and launches == 4
    assert sorted(got) == sorted(want)
    dec.close()


# ------------------------------------------------------------------------------------ history rules
def test_reset_empties_the_history(D):
    """After acg_reset the next call's first J - 1 outputs are the model's with zeros before them, and not the model's with the
    old history."""
    fmt, M, J, nwin = RR.CS16, 160, 4, 70
    rate = 12500 * M
    rng = np.random.default_rng(21)
    taps = LR.tap_tables("unit", rate, J, NS, np.random.default_rng(22))
    dec = D.Decoder(NS, decim=M, nstreams=NS, max_blocks=1, bitlog=False)
    dec.set_input_rate(rate)
    dec.set_channel_filter(taps)
    xa = RR.make_input(fmt, rate, NS, 0, nwin, rng, k=0)
    xb = RR.make_input(fmt, rate, NS, 0, nwin, rng, k=1)
    ta, pitch, ns = to_device(xa)
    assert dec.process_rate(RR.capi_fmt(fmt), ta, ns, pitch) == (nwin, nwin * M)
    dec.reset()
    tb, pitch, ns = to_device(xb)
    assert dec.process_rate(RR.capi_fmt(fmt), tb, ns, pitch) == (nwin, nwin * M)
    got = all_dm(dec, NS, nwin)
    dec.close()
    against_model(got, fmt, [LR.with_history([], xb[c], M, J) for c in range(NS)], M, J, taps, J - 1, "after reset")
    for c in range(NS):
        row_old = LR.with_history([xa[c]], xb[c], M, J)
        old = LR.exact(fmt, row_old, M, J, taps[c], nwin)
        far = np.abs(got[c].astype(np.float64) - old) > LR.bar(fmt, row_old, M, J, taps[c], nwin, old)
        assert far[: J - 1].all() and not far[J - 1:].any(), (c, far[:8])


def test_filter_off_is_the_plain_rate_path_bit_for_bit(D):
    """acg_set_channel_filter(NULL) makes the next call bit-identical to a fresh context on the plain rate path."""
    fmt, M, J, nwin = RR.CU8, 160, 3, 300
    rate = 12500 * M
    rng = np.random.default_rng(31)
    box = RR.make_taps(D, rate, NS, np.random.default_rng(32))
    x = RR.make_input(fmt, rate, NS, 0, nwin, rng)
    t, pitch, ns = to_device(x)
    fresh = D.Decoder(NS, decim=M, nstreams=NS, max_blocks=1, bitlog=False)
    fresh.set_taps(box)
    fresh.set_input_rate(rate)
    assert fresh.process_rate(RR.capi_fmt(fmt), t, ns, pitch) == (nwin, nwin * M)
    want = all_dm(fresh, NS, nwin)
    fresh.close()
    dec = D.Decoder(NS, decim=M, nstreams=NS, max_blocks=1, bitlog=False)
    dec.set_taps(box)
    dec.set_input_rate(rate)
    dec.set_channel_filter(LR.tap_tables("kaiser", rate, J, NS, np.random.default_rng(33), D))
    assert dec.process_rate(RR.capi_fmt(fmt), t, ns, pitch) == (nwin, nwin * M)
    assert not np.array_equal(all_dm(dec, NS, nwin).view(np.uint32), want.view(np.uint32))
    dec.set_channel_filter(None)
    assert dec.process_rate(RR.capi_fmt(fmt), t, ns, pitch) == (nwin, nwin * M)
    assert np.array_equal(all_dm(dec, NS, nwin).view(np.uint32), want.view(np.uint32))
    dec.close()


def test_three_channels_on_one_stream(D):
    """acg_set_channel_streams: channels 0, 1, 2 read stream 1, channels 3, 4 stream 0 -- two calls against the model"""
    fmt, M, J = RR.CS16, 160, 4
    rate, nch, ns_ = 12500 * M, 5, 3
    smap = np.array([1, 1, 1, 0, 0], dtype=np.int32)
    rng = np.random.default_rng(41)
    taps = LR.tap_tables("kaiser", rate, J, nch, np.random.default_rng(42), D)
    dec = D.Decoder(nch, decim=M, nstreams=ns_, max_blocks=1, bitlog=False)
    dec.set_channel_streams(smap)
    dec.set_input_rate(rate)
    dec.set_channel_filter(taps)
    seen = []
    for call, nwin in enumerate((97, 2, 64)):               # the second call is shorter than the history
        x = RR.make_input(fmt, rate, ns_, 0, max(nwin, RR.NPLANT), rng)[:, : 2 * nwin * M]
        t, pitch, ns = to_device(x)
        assert dec.process_rate(RR.capi_fmt(fmt), t, ns, pitch) == (nwin, nwin * M)
        rows_h = [LR.with_history([p[smap[c]] for p in seen], x[smap[c]], M, J) for c in range(nch)]
        against_model(all_dm(dec, nch, nwin), fmt, rows_h, M, J, taps, J - 1 if call == 0 else 0, "shared stream, call %d" % call)
        seen.append(x)
    dec.close()


# ------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("fmt", [RR.CF32, RR.CS16])
def test_end_to_end_beside_a_strong_carrier(D, O, S, K, fmt):
    """long_ref.interferer_stream (tests/test_long_ref.py holds it decodable on the model): with the filter on, acg_drain_msgs
    delivers every transmitted frame of all three channels field for field, dm is inside the bar and the oracle's demodulator on
    the GPU's own dm queues the same blocks; with the filter off the same context and input deliver fewer than half of channel
    0's frames."""
    row, box, filt, frames = LR.interferer_stream(D, S, fmt)
    rate, nout, nch, J = LR.E2E_RATE, LR.E2E_NOUT, 3, LR.E2E_J
    M = rate // 12500
    dec = D.Decoder(nch, decim=M, nstreams=1, max_blocks=nout // 1024, repair=True)
    dec.set_taps(box)
    dec.set_channel_streams(np.zeros(nch, dtype=np.int32))
    dec.set_input_rate(rate)
    dec.set_channel_filter(filt)
    t, pitch, n = to_device(row[None, :])
    assert dec.process_rate(RR.capi_fmt(fmt), t, n, pitch) == (nout, nout * M)
    msgs = dec.drain_msgs()
    dm = np.zeros((nch, nout), dtype=np.float32)
    assert dec.L.acg_read_dm_n(dec.ctx, 0, nch, dm.ctypes.data, nout, nout) == K.OK
    rowh = LR.with_history([], row, M, J)
    worst = against_model(dm, fmt, [rowh] * nch, M, J, filt, J - 1, "end to end " + fmt)
    print("LEDGER long end to end %s: worst err/bar %.3f" % (fmt, worst))
    for c in range(nch):
        mine = [m for m in msgs if m.chn == c]
        assert len(mine) == len(frames[c]) >= 2, (c, len(mine), len(frames[c]))
        for m, fr in zip(mine, frames[c]):
            f = RR.frame_fields(fr)
            assert m.err == 0 and m.mode == f["mode"] and m.addr == f["addr"] and m.ack == b"!" and m.label == f["label"]
            assert m.bid == f["bid"] and m.down not in (b"\x00", 0) and m.no == f["no"] and m.fid == f["fid"]
            assert bytes(m.txt[: m.txt_len]) == f["txt"] and m.be == b"\x03"
        ch = O.Channel(c)
        ch.demod(dm[c])
        orc = [O.msg_split(O.blk_process(f)) for f in ch.frames]
        assert [O.msg_tuple(m) for m in mine] == [O.msg_tuple(m) for m in orc], c
    # the same context and input without the filter: today's boxcar
    dec.set_channel_filter(None)
    dec.reset()
    assert dec.process_rate(RR.capi_fmt(fmt), t, n, pitch) == (nout, nout * M)
    texts = [RR.frame_fields(fr)["txt"] for fr in frames[0]]
    kept = [m for m in dec.drain_msgs() if m.chn == 0 and bytes(m.txt[: m.txt_len]) in texts]
    dec.close()
    assert 2 * len(kept) < len(frames[0]), (len(kept), len(frames[0]))


# ------------------------------------------------------------------------------------ refusals
def test_refusals(D, K):
    """After every refusal acg_last_error names the rule and no down-converter launch was made; acg_set_input_rate switches the
    filter off."""
    rate, M, J = 2000000, 160, 4
    L = K.load()
    rng = np.random.default_rng(51)
    taps = LR.tap_tables("kaiser", rate, J, 3, np.random.default_rng(52), D)
    five = np.zeros((3, 5 * M, 2), dtype=np.float32)

    def refused(dec, rc, code, word):
        assert rc == code, (rc, code, word)
        assert word in L.acg_last_error(dec.ctx).decode(), (word, L.acg_last_error(dec.ctx))
        assert timing_launches(dec) == 0

    dec = D.Decoder(3, decim=M, nstreams=3, max_blocks=1, timing=True)
    refused(dec, L.acg_set_channel_filter(dec.ctx, J, taps.ctypes.data), K.ESTATE, "no input rate")
    dec.set_input_rate(rate)
    refused(dec, L.acg_set_channel_filter(dec.ctx, 1, taps.ctypes.data), K.EINVAL, "nseg outside 2")
    refused(dec, L.acg_set_channel_filter(dec.ctx, 5, five.ctypes.data), K.EINVAL, "nseg outside 2")
    refused(dec, L.acg_set_channel_filter(dec.ctx, -2, taps.ctypes.data), K.EINVAL, "nseg outside 2")
    x = RR.make_input(RR.CS16, rate, 3, 0, 100, rng)
    dec.feed_rate(K.FMT_CS16, x[:, : 2 * 100])
    assert timing_launches(dec) == 0                              # 100 samples: no whole window
    refused(dec, L.acg_set_channel_filter(dec.ctx, J, taps.ctypes.data), K.ESTATE, "carries samples")
    refused(dec, L.acg_set_channel_filter(dec.ctx, 0, None), K.ESTATE, "carries samples")
    dec.reset()
    # on, then acg_set_input_rate (the same value): off again, the plain rate path's bits
    box = RR.make_taps(D, rate, 3, np.random.default_rng(53))
    dec.set_taps(box)
    t, pitch, ns = to_device(x)
    assert dec.process_rate(K.FMT_CS16, t, ns, pitch) == (100, 100 * M)
    plain = all_dm(dec, 3, 100)
    dec.set_channel_filter(taps)
    assert dec.process_rate(K.FMT_CS16, t, ns, pitch) == (100, 100 * M)
    assert not np.array_equal(all_dm(dec, 3, 100).view(np.uint32), plain.view(np.uint32))
    dec.set_input_rate(rate)
    assert dec.process_rate(K.FMT_CS16, t, ns, pitch) == (100, 100 * M)
    assert np.array_equal(all_dm(dec, 3, 100).view(np.uint32), plain.view(np.uint32))
    assert timing_launches(dec) == 3
    dec.close()

    # a rate that is no multiple of 12 500 Hz
    dec = D.Decoder(3, decim=164, nstreams=3, max_blocks=1, timing=True)
    dec.set_input_rate(2048000)
    t164 = np.zeros((3, J * 164, 2), dtype=np.float32)
    refused(dec, L.acg_set_channel_filter(dec.ctx, J, t164.ctypes.data), K.EINVAL, "multiple of 12 500")
    dec.close()
