"""The recordings' sample formats on the GPU: complex int8 (ACG_FMT_CS8, SigMF ci8) and complex float32 (ACG_FMT_CF32, SigMF
cf32_le) through every kernel they can take -- the wave-private streaming kernels, the workgroup-granular fallbacks, the matrix
pipe and the shared-stream vector kernel for int8 with several channels per stream -- the limits, the host feed with carry and
the whole pipeline down to acg_drain_msgs.  Every output against the float64-exact value of the reference's expression
(tests/iq_format_ref.py; the oracle knows neither format), the matrix pipe bit for bit against its model.  Every test first asks
the launcher (acg_lab_samples_launch_shape) that the launch takes the kernel it names.  Runs on the GPU box only (-m gpu).

Tolerances, the project's written ones: CS8 1e-5 |x| + 1e-6; CF32 1e-5 |x| + 1e-6 max|x| over the channel's windows; the matrix
pipe equal to its model (and the model within 2e-7 relative of the exact value: tests/test_iq_format_ref.py).
"""
import numpy as np
import pytest

import iq_format_ref as Q
from test_gpu_formats import SHAPES_FEWER, set_shape, to_device

pytestmark = pytest.mark.gpu

NS = 6                              # streams, one channel each


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


def all_dm(dec, nch, n):
    return np.stack([dec.dm(c, n) for c in range(nch)])


def check_exact(got, ex, fmt, what):
    """every output within the bar of the exact value; returns the worst err / bar"""
    r = np.abs(got.astype(np.float64) - ex) / Q.bar(ex, fmt)
    c, m = np.unravel_index(int(r.argmax()), r.shape)
    assert r.max() <= 1.0, "%s: %.3f of the bar at channel %d window %d: %r, exact %r" % (what, r.max(), c, m, got[c, m], ex[c, m])
    return float(r.max())


class Inputs:
    """`n` inputs of one (format, M) on NS streams with a scrambled stream map each, on the device, and the exact values of six
    channels (one per stream): made once per case.  Calls cycle through them, so what one launch left behind is never what the
    next must produce."""

    def __init__(self, D, fmt, M, ntaps, nwin, seed, n=3):
        rng = np.random.default_rng(seed)
        self.fmt, self.M, self.nwin = fmt, M, nwin
        self.taps = Q.make_taps(D, M, NS, np.random.default_rng(seed + 1), ntaps)
        self.maps, self.dev, self.exact = [], [], []
        for k in range(n):
            x = Q.make_input(fmt, M, NS, nwin, rng, k)
            smap = rng.permutation(NS).astype(np.int32)
            while np.array_equal(smap, np.arange(NS)):
                smap = rng.permutation(NS).astype(np.int32)
            self.maps.append(smap)
            self.dev.append(to_device(fmt, x))
            self.exact.append(np.stack([Q.exact(fmt, x[smap[c]], M, self.taps[c], nwin) for c in range(NS)]))
        for j in range(n):              # a stale channel cannot pass: most windows differ between two inputs by more than both bars
            for k in range(j):
                near = np.abs(self.exact[j] - self.exact[k]) <= Q.bar(self.exact[j], fmt) + Q.bar(self.exact[k], fmt)
                assert near.mean(axis=1).max() < 0.1

    def run(self, dec, k, nblk):
        t, pitch, _ = self.dev[k]
        dec.set_channel_streams(self.maps[k])
        dec.process_samples(Q.capi_fmt(self.fmt), t, nblk, pitch, 0)
        return all_dm(dec, NS, self.nwin)


def streaming_case(D, K, tune, fmt, M, ntaps):
    nblk = 2
    nwin = nblk * 1024
    W = Q.DIRECT_W[(fmt, M)]
    P = Inputs(D, fmt, M, ntaps, nwin, 4000 * M + ntaps + len(fmt))
    dec = D.Decoder(NS, decim=M, ntaps=ntaps, nstreams=NS, max_blocks=nblk, bitlog=False)
    dec.set_taps(P.taps)
    out, worst = {}, 0.0
    for k, shape in enumerate(SHAPES_FEWER):
        set_shape(tune, shape)
        s = dec.samples_launch(Q.capi_fmt(fmt), nblk)
        if shape[0] == "fallback":
            assert s.family == K.FIR_WORKGROUP, (shape[0], s.family)
        else:
            assert s.family == K.FIR_STREAMING and s.tile_windows == W, (shape[0], s.family, s.tile_windows)
            assert s.runs == NS * nwin // (2 * W * s.bodies_per_run) and s.runs >= 4 * NS          # several runs per channel
            if shape[0] == "1wave-pairs1":
                assert s.waves_per_workgroup == 1 and s.bodies_per_run == 1 and s.waves <= 256
                assert s.runs > s.waves or s.waves == s.runs < 256, (s.runs, s.waves)             # runs by ticket, or fewer runs than waves
        assert s.chunk_blocks >= nblk                                                               # one launch per call
        for j in (k, (k + 1) % 3):
            out[shape[0], j] = got = P.run(dec, j, nblk)
            worst = max(worst, check_exact(got, P.exact[j], fmt, "%s %d/%d %s input %d" % (fmt, M, ntaps, shape[0], j)))
    set_shape(tune, SHAPES_FEWER[0])
    dec.close()
    # run length and workgroup shape change no sum; the fallback adds in another order: not the same bits, so the others did
    # not run it
    assert np.array_equal(out["default", 1], out["1wave-pairs1", 1])
    assert not np.array_equal(out["fallback", 0], out["default", 0])
    print("LEDGER %s M=%d ntaps=%d W=%d: worst err/bar %.3f" % (fmt, M, ntaps, W, worst))


# ------------------------------------------------------------------------------------ streaming kernels
@pytest.mark.parametrize("fmt,M", Q.DIRECT, ids=["%s-%d" % c for c in Q.DIRECT])
def test_streaming_kernels_six_streams_two_callbacks(D, K, fmt, M, tune):
    """fir_s8_direct_kernel<20 / 24 / 25> and fir_fmt_direct_kernel<CF32, 80 / 96 / 100, 16>: six streams, one channel each,
    through a scrambled stream map, 2048 windows (two callbacks, several runs per channel), a different frequency per channel,
    one table scaled by 1/512, one with exact zeros at the odd indices.  Default launch shape, one-wave workgroups one per CU
    (fewer runs than waves / runs by ticket) and the fallback kernel; every output against the exact value."""
    streaming_case(D, K, tune, fmt, M, M)


@pytest.mark.parametrize("fmt,M", Q.DIRECT, ids=["%s-%d" % c for c in Q.DIRECT])
def test_streaming_kernels_fewer_taps_than_the_window(D, K, fmt, M, tune):
    """the same with ntaps = M - 8: the kernels' zero tap columns"""
    streaming_case(D, K, tune, fmt, M, M - 8)


# ------------------------------------------------------------------------------------ fallback kernels
FALLBACK_CASES = [(f, M, None) for f, M in Q.FALLBACK] + [(Q.CS8, 200, 3), (Q.CF32, 200, 3)]


@pytest.mark.parametrize("fmt,M,variant", FALLBACK_CASES, ids=["%s-%d%s" % (f, M, "-variant3" if v else "") for f, M, v in FALLBACK_CASES])
def test_fallback_kernels(D, K, fmt, M, variant, tune):
    """The workgroup-granular kernels: CS8 (fir_u8_persist_kernel, signed) at M = 8, 168 (21 chunks per window) and 320; CF32
    (fir_fmt_kernel) at M = 2 (one chunk), 164, 400 (several LDS slices) and 1024; both at M = 200 with ACG_FIR_VARIANT=3.  One
    callback on six streams, two inputs in turn, twice: the second round gives the bits of the first."""
    nblk, nwin = 1, 1024
    if variant:
        tune("ACG_FIR_VARIANT", str(variant))
    P = Inputs(D, fmt, M, M, nwin, 700 * M + len(fmt), n=2)
    dec = D.Decoder(NS, decim=M, nstreams=NS, max_blocks=nblk, bitlog=False)
    dec.set_taps(P.taps)
    s = dec.samples_launch(Q.capi_fmt(fmt), nblk)
    assert s.family == K.FIR_WORKGROUP and s.tile_windows == 0, (s.family, s.tile_windows)
    first, worst = {}, 0.0
    for rnd in range(2):
        for k in range(2):
            got = P.run(dec, k, nblk)
            worst = max(worst, check_exact(got, P.exact[k], fmt, "%s M=%d round %d input %d" % (fmt, M, rnd, k)))
            assert np.array_equal(first.setdefault(k, got), got), (rnd, k)
    dec.close()
    print("LEDGER fallback %s M=%d: worst err/bar %.3f" % (fmt, M, worst))


# ------------------------------------------------------------------------------------ refused
@pytest.mark.parametrize("fmt,M,rule", Q.REFUSED, ids=["%s-%d" % (f, M) for f, M, _ in Q.REFUSED])
def test_window_lengths_outside_the_limits_are_refused(D, K, fmt, M, rule):
    """CS8 at M = 164 (no whole number of 8-sample chunks) and 328 (above ACG_MAXDECIM), CF32 at M = 161: ACG_EINVAL,
    acg_last_error names the rule, nothing is launched, and the context still works afterwards.  CF32 at M = 1026 is above
    ACG_MAXDECIM_SAMPLES, which no context can have: acg_create says ACG_EINVAL."""
    import torch
    if rule is None:
        with pytest.raises(K.AcgError) as e:
            D.Decoder(2, decim=M, nstreams=2, max_blocks=1, bitlog=False)
        assert e.value.code == K.EINVAL
        return
    dec = D.Decoder(2, decim=M, nstreams=2, max_blocks=1, bitlog=False)
    dec.set_timing(2)
    row = 1024 * M * Q.sample_bytes(fmt)
    pitch = (row + 15) // 16 * 16
    t = torch.zeros(2 * pitch + 64, dtype=torch.uint8, device="cuda")
    for call in (lambda: dec.process_samples(Q.capi_fmt(fmt), t, 1, pitch, 0), lambda: dec.samples_launch(Q.capi_fmt(fmt), 1),
                 lambda: dec.feed(Q.capi_fmt(fmt), np.zeros((2, 64), dtype=np.int8 if fmt == Q.CS8 else np.float32))):
        with pytest.raises(K.AcgError) as e:
            call()
        assert e.value.code == K.EINVAL and rule in str(e.value), str(e.value)
    assert dec.timing()["fir_launches"] == 0
    # the context still works: the u8 path takes any window length up to ACG_MAXDECIM, CS16 any multiple of 4
    if M <= 320:
        u8 = torch.full((2 * 1024 * M * 2,), 130, dtype=torch.uint8, device="cuda")
        dec.in_callback(u8.view(2, -1), nblocks=1, pitch=1024 * M * 2)
    else:
        s16 = torch.zeros(2 * 1024 * M * 4, dtype=torch.uint8, device="cuda")
        dec.process_samples(K.FMT_CS16, s16, 1, 1024 * M * 4, 0)
    dec.sync()
    assert dec.timing()["fir_launches"] == 1 and np.all(np.isfinite(dec.dm(1, 1024)))
    dec.close()


@pytest.mark.parametrize("fmt", [Q.CS8, Q.CF32])
def test_misaligned_pitch_and_base_are_refused(D, K, fmt):
    """base and pitch must be 16-byte aligned, as for every sample format: ACG_EINVAL with the rule, nothing launched, and the
    aligned call right behind it works"""
    import torch
    M = 200
    dec = D.Decoder(2, decim=M, nstreams=2, max_blocks=1, bitlog=False)
    dec.set_timing(2)
    row = 1024 * M * Q.sample_bytes(fmt)
    t = torch.zeros(2 * row + 64, dtype=torch.uint8, device="cuda")
    for kw in (dict(t=t, pitch=row + 8), dict(t=t[8:], pitch=row)):
        with pytest.raises(K.AcgError) as e:
            dec.process_samples(Q.capi_fmt(fmt), kw["t"], 1, kw["pitch"], 0)
        assert e.value.code == K.EINVAL and "16-byte aligned" in str(e.value)
    assert dec.timing()["fir_launches"] == 0
    dec.process_samples(Q.capi_fmt(fmt), t, 1, row + 16, 0)
    dec.sync()
    assert dec.timing()["fir_launches"] == 1
    dec.close()


# ------------------------------------------------------------------------------------ ACARS on the new formats
FREQS3 = [131525000, 131725000, 131825000]


def acars_streams(D, S, fmt, M, nstreams, nout, seed, per_stream=3):
    """`nstreams` clean streams with `per_stream` synthetic ACARS channels each (the same three frequencies on every stream,
    different traffic), as the format's samples [nstreams, nout M 2 values]; returns (x, taps [nch, M, 2], stream map, frames per
    channel)"""
    rng = np.random.default_rng(seed)
    fc = D.choose_fc(FREQS3, M)[0]
    nch = nstreams * per_stream
    taps = np.stack([D.soapy_taps(float(FREQS3[c % per_stream]), fc, M) for c in range(nch)])
    smap = np.repeat(np.arange(nstreams), per_stream).astype(np.int32)
    rows, frames = [], []
    for s in range(nstreams):
        env = []
        for c in range(per_stream):
            a, fr = S.channel_audio(rng, nout, gap=(400, 900), text_len=(12, 40))
            env.append(0.5 * (1 + 0.5 * a))
            frames.append(fr)
        offs = [FREQS3[c] - fc for c in range(per_stream)]
        ph = np.linspace(0, 3, per_stream)
        if fmt == Q.CS8:
            rows.append(S.iq_s8_from_envelopes(np.array(env), M, offs, phases=ph, scale=0.3, noise=0.004, rng=rng))
        else:
            rows.append(S.iq_cf32_from_envelopes(np.array(env), M, offs, phases=ph, scale=0.3, noise=0.004, rng=rng).view(np.float32))
    return np.stack(rows), taps, smap, frames


@pytest.mark.parametrize("fmt", [Q.CS8, Q.CF32])
def test_host_feed_with_carry_equals_one_device_call(D, S, K, fmt, tune):
    """acg_feed_samples_host with three streams at M = 200: the same samples fed in pieces of 1, M - 1, 3 M + 7, 5 samples and the
    rest (lengths are in samples: no piece boundary falls inside a sample's bytes) -- dm of every launch and the blocks are bit for
    bit those of one acg_process_samples_dev call over the whole input.
    The feed's launches are 1, 3 and nout - 4 windows: none is whole runs, so they take the workgroup-granular kernel.  Bit
    identity needs the same order of additions, so the device call is held to that kernel too (ACG_FIR_VARIANT=3, asked of the
    launcher); against the exact value it is checked like every other launch."""
    M, ns, nblk = 200, 3, 4
    nout = nblk * 1024
    x, taps, smap, frames = acars_streams(D, S, fmt, M, ns, nout, 11 + len(fmt), per_stream=1)
    nch, total = ns, nout * M
    assert sum(len(f) for f in frames) >= nch

    tune("ACG_FIR_VARIANT", "3")
    ref = D.Decoder(nch, decim=M, nstreams=ns, max_blocks=nblk)
    ref.set_taps(taps)
    ref.set_channel_streams(smap)
    assert ref.samples_launch(Q.capi_fmt(fmt), nblk).family == K.FIR_WORKGROUP
    t, pitch, _ = to_device(fmt, x)
    ref.process_samples(Q.capi_fmt(fmt), t, nblk, pitch, 0)
    want_dm = all_dm(ref, nch, nout)
    want = [D.frame_tuple(f) for f in ref.drain_frames()]
    ref.close()
    assert len(want) >= nch
    ex = np.stack([Q.exact(fmt, x[smap[c]], M, taps[c], nout) for c in range(nch)])
    check_exact(want_dm, ex, fmt, "device call " + fmt)
    tune("ACG_FIR_VARIANT", None)

    dec = D.Decoder(nch, decim=M, nstreams=ns, max_blocks=nblk)
    dec.set_taps(taps)
    dec.set_channel_streams(smap)
    got, pos, launches = [], 0, 0
    for n in (1, M - 1, 3 * M + 7, 5, total):
        n = min(n, total - pos)
        w0, w1 = pos // M, (pos + n) // M
        if w1 > w0:                                      # the windows this feed completes: one launch, and never whole runs
            assert (w1 - w0) % 32 != 0
        dec.feed(Q.capi_fmt(fmt), x[:, 2 * pos: 2 * (pos + n)])
        pos += n
        if w1 > w0:
            launches += 1
            dm = all_dm(dec, nch, w1 - w0)
            assert np.array_equal(dm.view(np.uint32), want_dm[:, w0: w1].view(np.uint32)), (fmt, w0, w1)
        got += [D.frame_tuple(f) for f in dec.drain_frames()]
    assert pos == total and launches == 3
    assert sorted(got) == sorted(want)
    dec.close()


def test_u8_host_calls_and_carrying_feeds_alternate_on_one_context(D, K, tune):
    """acg_process_iq_u8_host and acg_feed_samples_host(ACG_FMT_CS8) share the two staging buffers of a context and may alternate
    on it: feed of exactly one window, u8 call, u8 call, feed of 3 M + 7 samples, u8 call, feed of M - 7 samples, every call with
    data of its own.  After each call dm (acg_read_dm_n) is bit for bit what a twin context makes of the same samples in one
    device call: acg_process_iq_u8_dev per u8 block, one acg_process_samples_dev call over the feeds' 5 M samples (held to the
    workgroup-granular kernel, which the feeds' launches of 1, 3 and 1 windows take: see the test above).
    The third u8 call comes while 7 samples are carried: it is refused (ACG_ESTATE, include/acarsdec_amd.h) and must leave dm,
    the carried samples and the buffers as they were -- the last feed completes the window the 7 samples began."""
    import torch
    M, ns, nwin = 160, 3, 1024
    rng = np.random.default_rng(31)
    fc = D.choose_fc(FREQS3, M)[0]
    taps = np.stack([D.soapy_taps(float(f), fc, M) for f in FREQS3])
    u8 = [rng.integers(0, 256, size=(ns, nwin * M * 2), dtype=np.uint8) for _ in range(3)]
    s8 = rng.integers(-128, 128, size=(ns, nwin * M * 2), dtype=np.int8)          # the feeds' samples are its first 5 M

    def context():
        d = D.Decoder(ns, decim=M, nstreams=ns, max_blocks=1, bitlog=False)
        d.set_taps(taps)
        return d

    def dm_of(d, n):
        dm = np.zeros((ns, n), dtype=np.float32)
        assert d.L.acg_read_dm_n(d.ctx, 0, ns, dm.ctypes.data, n, n) == K.OK
        return dm.view(np.uint32)

    twin = context()
    want_u8 = []
    for x in u8[:2]:
        twin.in_callback(torch.from_numpy(x).cuda(), 1)
        want_u8.append(dm_of(twin, nwin))
    tune("ACG_FIR_VARIANT", "3")
    assert twin.samples_launch(K.FMT_CS8, 1).family == K.FIR_WORKGROUP
    t, pitch, _ = to_device(Q.CS8, s8)
    twin.process_samples(K.FMT_CS8, t, 1, pitch, 0)
    want_s8 = dm_of(twin, 5)
    tune("ACG_FIR_VARIANT", None)
    twin.close()
    assert not np.array_equal(want_u8[0], want_u8[1])

    dec = context()
    pos = [0]

    def feed(n, w0, w1):
        dec.feed(K.FMT_CS8, s8[:, 2 * pos[0]: 2 * (pos[0] + n)])
        pos[0] += n
        assert np.array_equal(dm_of(dec, w1 - w0), want_s8[:, w0: w1]), (w0, w1)

    def u8_host(k):
        dec.in_callback(u8[k], 1)
        assert np.array_equal(dm_of(dec, nwin), want_u8[k]), k

    feed(M, 0, 1)
    u8_host(0)
    u8_host(1)
    feed(3 * M + 7, 1, 4)
    assert dec.L.acg_process_iq_u8_host(dec.ctx, u8[2].ctypes.data, u8[2].shape[1], 1) == K.ESTATE
    assert b"partial window" in dec.L.acg_last_error(dec.ctx)
    assert np.array_equal(dm_of(dec, 3), want_s8[:, 1: 4])
    feed(M - 7, 4, 5)
    assert pos[0] == 5 * M
    dec.close()


@pytest.mark.parametrize("fmt", [Q.CF32, Q.CS8])
def test_end_to_end_three_channels_on_one_stream(D, O, S, K, fmt):
    """Three synthetic ACARS channels on one clean stream, M = 200: every transmitted frame is delivered field for field by
    acg_drain_msgs, and the oracle's demodulator fed the GPU's own dm (acg_read_dm_n) queues the same blocks."""
    M, nblk = 200, 4
    nout = nblk * 1024
    x, taps, smap, frames = acars_streams(D, S, fmt, M, 1, nout, 23 + len(fmt))
    nch = 3
    assert all(len(f) >= 1 for f in frames)
    dec = D.Decoder(nch, decim=M, nstreams=1, max_blocks=nblk, repair=True)
    dec.set_taps(taps)
    dec.set_channel_streams(smap)
    s = dec.samples_launch(Q.capi_fmt(fmt), nblk)
    # CS8: three channels of one stream at M = 200 go to the matrix pipe; CF32: every channel reads the stream itself
    assert s.family == (K.FIR_MATRIX if fmt == Q.CS8 else K.FIR_STREAMING), s.family
    t, pitch, _ = to_device(fmt, x)
    dec.process_samples(Q.capi_fmt(fmt), t, nblk, pitch, 0)
    msgs = dec.drain_msgs()
    dm = np.zeros((nch, nout), dtype=np.float32)
    assert dec.L.acg_read_dm_n(dec.ctx, 0, nch, dm.ctypes.data, nout, nout) == K.OK
    dec.close()
    ex = np.stack([Q.exact(fmt, x[0], M, taps[c], nout) for c in range(nch)])
    err = np.abs(dm - ex)
    assert np.all(err <= (2e-7 * ex + 1e-9 if fmt == Q.CS8 else Q.bar(ex, fmt)))
    for c in range(nch):
        mine = [m for m in msgs if m.chn == c]
        assert len(mine) == len(frames[c]), (c, len(mine), len(frames[c]))
        for m, fr in zip(mine, frames[c]):
            # synth.acars_frame: + * SYN SYN SOH | mode addr[7] ack label[2] bid STX text ETX | crc[2] DEL, parity on every byte;
            # output.c's split of a downlink (bid is a digit): msgno = text[0:4], flight = text[4:10], the rest is the text
            body = bytes(b & 0x7F for b in fr[5:-3])
            text = body[13:-1]
            assert body[12] == 0x02 and body[-1] == 0x03 and len(text) >= 12
            assert m.err == 0 and m.mode == body[0:1] and m.addr == body[2:8] and m.ack == b"!" and m.label == body[9:11]
            assert m.bid == body[11:12] and m.down not in (b"\x00", 0) and m.no == text[0:4] and m.fid == text[4:10]
            assert bytes(m.txt[: m.txt_len]) == text[10:] and m.be == b"\x03"
        # the oracle's demodulator on the GPU's own dm queues the same blocks, and its split gives the same fields
        ch = O.Channel(c)
        ch.demod(dm[c])
        orc = [O.msg_split(O.blk_process(f)) for f in ch.frames]
        assert [O.msg_tuple(m) for m in mine] == [O.msg_tuple(m) for m in orc], c


# ------------------------------------------------------------------------------------ CS8 with several channels per stream
@pytest.mark.parametrize("M", [160, 192, 200])
def test_cs8_matrix_pipe_bit_for_bit(D, K, M, tune):
    """fir_s8_mm_kernel: two streams, 11 channels on one (groups of 8 and 3) and 1 on the other, one and two tiles in flight
    (ACG_FIR_MM_STAGES): every dm bit for bit equal to the model, the all-(-128) windows included.  The same context with
    ACG_FIR_MM=0 (the shared-stream vector kernel) within the bar of the exact value."""
    nblk, nch = 2, 12
    nout = nblk * 1024
    rng = np.random.default_rng(600 + M)
    x = rng.integers(-128, 128, size=(2, nout * M * 2), dtype=np.int8)
    x[0, : 3 * 2 * M] = -128                                       # three windows of all -128 on each stream, at different places
    x[1, 40 * 2 * M: 43 * 2 * M] = -128
    x[0, 70 * 2 * M: 72 * 2 * M] = 127
    smap = np.zeros(nch, dtype=np.int32)
    smap[7] = 1                                                    # the lone channel sits in the middle of the channel numbers
    taps = Q.make_taps(D, M, nch, rng)
    taps[9] = 0                                                    # an all-zero table: +0.0
    model, ex = np.zeros((nch, nout), dtype=np.float32), np.zeros((nch, nout))
    for s in range(2):
        chs = np.flatnonzero(smap == s)
        model[chs] = Q.mm_model_dm(x[s], M, [taps[c] for c in chs], nout)
        ex[chs] = Q.exact(Q.CS8, x[s], M, taps[chs], nout)
    tune("ACG_PIPE_BLOCKS", "0")
    t, pitch, _ = to_device(Q.CS8, x)
    for stages in (1, 2):
        tune("ACG_FIR_MM_STAGES", str(stages))
        dec = D.Decoder(nch, decim=M, nstreams=2, max_blocks=nblk, bitlog=False)
        dec.set_taps(taps)
        dec.set_channel_streams(smap)
        s = dec.samples_launch(K.FMT_CS8, nblk)
        assert s.family == K.FIR_MATRIX and s.stages == stages and s.tile_windows == 32, (s.family, s.stages)
        for rnd in range(2):
            dec.process_samples(K.FMT_CS8, t, nblk, pitch, 0)
            got = all_dm(dec, nch, nout)
            bad = np.flatnonzero(got.view(np.uint32) != model.view(np.uint32))
            assert bad.size == 0, (stages, rnd, int(bad.size), int(bad[0]), float(got.flat[bad[0]]), float(model.flat[bad[0]]))
        assert np.all(got[9] == 0) and not np.signbit(got[9]).any()
        # the same context on the shared-stream vector kernel
        tune("ACG_FIR_MM", "0")
        assert dec.samples_launch(K.FMT_CS8, nblk).family == K.FIR_SHARED_VECTOR
        dec.process_samples(K.FMT_CS8, t, nblk, pitch, 0)
        vec = all_dm(dec, nch, nout)
        check_exact(vec, ex, Q.CS8, "CS8 shared vector M=%d" % M)
        assert not np.array_equal(vec, model)                      # another kernel, another order of roundings
        tune("ACG_FIR_MM", None)
        dec.close()
    err = np.abs(model.astype(np.float64) - ex)
    assert np.all(err <= 2e-7 * ex + 1e-9)


def test_cs8_shared_streams_at_a_length_without_a_matrix_kernel(D, K, tune):
    """M = 168: several channels per stream take the shared-stream vector kernel with the signed switch; within the bar"""
    M, nblk, nch = 168, 1, 12
    nout = 1024
    rng = np.random.default_rng(168)
    x = Q.make_input(Q.CS8, M, 3, nout, rng)[:2]
    smap = np.zeros(nch, dtype=np.int32)
    smap[4] = 1
    taps = Q.make_taps(D, M, nch, rng)
    dec = D.Decoder(nch, decim=M, nstreams=2, max_blocks=nblk, bitlog=False)
    dec.set_taps(taps)
    dec.set_channel_streams(smap)
    assert dec.samples_launch(K.FMT_CS8, nblk).family == K.FIR_SHARED_VECTOR
    t, pitch, _ = to_device(Q.CS8, x)
    dec.process_samples(K.FMT_CS8, t, nblk, pitch, 0)
    got = all_dm(dec, nch, nout)
    dec.close()
    ex = np.stack([Q.exact(Q.CS8, x[smap[c]], M, taps[c], nout) for c in range(nch)])
    print("LEDGER CS8 shared vector M=168: worst err/bar %.3f" % check_exact(got, ex, Q.CS8, "CS8 shared vector M=168"))


def test_cf32_shared_streams_read_their_stream(D, K):
    """CF32 with several channels per stream: no matrix path -- every channel reads its stream through the stream map, on the
    streaming kernel"""
    M, nblk, nch = 200, 1, 7
    nout = 1024
    rng = np.random.default_rng(7)
    x = Q.make_input(Q.CF32, M, NS, nout, rng)
    smap = np.array([5, 3, 3, 0, 4, 3, 0], dtype=np.int32)
    taps = Q.make_taps(D, M, nch, rng)
    dec = D.Decoder(nch, decim=M, nstreams=NS, max_blocks=nblk, bitlog=False)
    dec.set_taps(taps)
    dec.set_channel_streams(smap)
    assert dec.samples_launch(K.FMT_CF32, nblk).family == K.FIR_STREAMING
    t, pitch, _ = to_device(Q.CF32, x)
    dec.process_samples(K.FMT_CF32, t, nblk, pitch, 0)
    got = all_dm(dec, nch, nout)
    dec.close()
    ex = np.stack([Q.exact(Q.CF32, x[smap[c]], M, taps[c], nout) for c in range(nch)])
    check_exact(got, ex, Q.CF32, "CF32 shared streams")
