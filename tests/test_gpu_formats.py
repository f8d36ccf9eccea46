"""The sample-format down-converters (CS16 / split int16 / real f32, csrc/fir.hip) where their machinery matters: launches of
thousands of runs on several streams, every launch shape, the workgroup-granular fallback at its other window lengths, and
several streams through the host feed.  Every window of every channel against the float64-exact value of the reference's
expression (tests/format_ref.py) and against the oracle, on full-range input.  Runs on the GPU box only (-m gpu).

Tolerance: the project's written one for dm, format_ref.bar -- 1e-5 |x| + 1e-6 (split int16: + 1e-6 max|x|).
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import format_ref as R

pytestmark = pytest.mark.gpu

SIZES6 = [1, 3, 8, 11, 16, 1]       # channels per stream, 40 channels on 6 streams
SIZES3 = [3, 2, 2]                  # 7 channels on 3 streams
RESIDENT_WAVES = 2048               # 256 CUs x 8 waves: the most a launch of these kernels keeps resident
SWITCHES = ("ACG_FIR_WAVES_PER_WG", "ACG_FIR_WG_PER_CU", "ACG_FIR_RUN_PAIRS", "ACG_FIR_VARIANT")
# launch shapes of one context, in the order they run: (name, WAVES_PER_WG, WG_PER_CU, RUN_PAIRS, VARIANT)
SHAPES = [("default", None, None, None, None),
          ("1wave-pairs1", 1, 1, 1, None),          # <= 256 waves
          ("1wave-pairs2", 1, 1, 2, None),
          ("1wave-pairs8", 1, 1, 8, None),
          ("2waves", 2, 1, None, None),
          ("fallback", None, None, None, 3)]
SHAPES_FEWER = [SHAPES[0], SHAPES[1], SHAPES[5]]


@pytest.fixture(scope="module")
def D():
    from acarsdec_amd import decoder
    from acarsdec_amd import _capi as K
    assert K.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return decoder


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def S():
    from acarsdec_amd import synth
    return synth


def by_channel(tuples):
    out = {}
    for t in tuples:
        out.setdefault(t[0], []).append(t)
    return out


def capi_fmt(fmt):
    from acarsdec_amd import _capi as K
    return {R.CS16: K.FMT_CS16, R.SPLIT: K.FMT_S16_SPLIT, R.F32R: K.FMT_F32_REAL}[fmt]


def to_device(fmt, x, pad=48):
    """One input of format_ref.make_input on the device, rows `pitch` bytes apart with pitch > the row (16-byte aligned; the
    gaps hold a filler that is no sample of the input); split int16: all I rows, then all Q rows `plane` bytes further.
    Returns (tensor, pitch, plane)."""
    import torch
    planes = x if fmt == R.SPLIT else (x,)
    ns, rowb = planes[0].shape[0], planes[0].shape[1] * planes[0].itemsize
    assert rowb % 16 == 0 and pad % 16 == 0 and pad > 0
    pitch = rowb + pad
    plane = ns * pitch + 32 if fmt == R.SPLIT else 0
    buf = np.full(plane * (len(planes) - 1) + ns * pitch, 0x5A, dtype=np.uint8)
    for p, a in enumerate(planes):
        for s in range(ns):
            o = p * plane + s * pitch
            buf[o: o + rowb] = np.ascontiguousarray(a[s]).view(np.uint8)
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 16 == 0
    return t, pitch, plane


def scrambled_map(sizes, rng):
    m = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(m)
    return m.astype(np.int32)


class Pairs:
    """Three (input, stream map) pairs with their references, computed once: exact [nch, nwin] float64 and oracle
    [nch, nwin] float32 per pair.  Calls cycle through the three, so a repeat lands neither one nor two calls behind (dm is
    double-buffered per call), and what an earlier launch left behind is never what the next one must produce."""

    def __init__(self, O, fmt, M, taps, sizes, nwin, rng):
        self.fmt, self.M, self.nwin, self.nch = fmt, M, nwin, int(sum(sizes))
        self.maps, self.dev, self.exact, self.oracle = [], [], [], []
        for k in range(3):
            x = R.make_input(fmt, M, len(sizes), nwin, rng, k)
            smap = scrambled_map(sizes, rng)
            ex = np.zeros((self.nch, nwin))
            orc = np.zeros((self.nch, nwin), dtype=np.float32)

            def exact_of_stream(s):
                chans = np.flatnonzero(smap == s)
                ex[chans] = R.exact(fmt, R.row_of(fmt, x, s), M, taps[chans], nwin)

            def oracle_of_channel(c):
                orc[c] = R.oracle(O, fmt, R.row_of(fmt, x, smap[c]), M, taps[c], nwin)

            with ThreadPoolExecutor(8) as pool:             # (numpy and the oracle's C run without the interpreter lock)
                list(pool.map(oracle_of_channel, range(self.nch)))
                list(pool.map(exact_of_stream, range(len(sizes))))
            self.maps.append(smap)
            self.dev.append(to_device(fmt, x))
            self.exact.append(ex)
            self.oracle.append(orc)
        self.bar = [R.bar(e, fmt) for e in self.exact]
        self.bar_o = [R.bar(o, fmt) for o in self.oracle]
        # a stale value cannot pass: in every channel, nine windows in ten differ between any two pairs by more than both bars
        # (a launch that leaves a channel stale leaves all its windows; the 1/512 table's values are few bars apart)
        for j in range(3):
            for k in range(j):
                near = np.abs(self.exact[j] - self.exact[k]) <= self.bar[j] + self.bar[k]
                assert near.mean(axis=1).max() < 0.1, (j, k, near.mean(axis=1).max())
        self.worst = 0.0

    def run(self, dec, k, nblk):
        t, pitch, plane = self.dev[k]
        dec.set_channel_streams(self.maps[k])
        dec.process_samples(capi_fmt(self.fmt), t, nblk, pitch, plane)
        return np.stack([dec.dm(c, self.nwin) for c in range(self.nch)])

    def check(self, got, k, what):
        e = np.abs(got - self.exact[k]) / self.bar[k]
        o = np.abs(got - self.oracle[k]) / self.bar_o[k]
        self.worst = max(self.worst, float(e.max()))
        c, m = np.unravel_index(int(e.argmax()), e.shape)
        assert e.max() <= 1.0, "%s pair %d: %.3f of the bar from the exact value at channel %d (stream %d) window %d: %r, exact %r" % (
            what, k, e.max(), c, self.maps[k][c], m, got[c, m], self.exact[k][c, m])
        c, m = np.unravel_index(int(o.argmax()), o.shape)
        assert o.max() <= 1.0, "%s pair %d: %.3f of the bar from the oracle at channel %d (stream %d) window %d: %r, oracle %r" % (
            what, k, o.max(), c, self.maps[k][c], m, got[c, m], self.oracle[k][c, m])


def set_shape(tune, shape):
    for name, v in zip(SWITCHES, shape[1:]):
        tune(name, None if v is None else str(v))


def make_tables(D, O, fmt, M, nch, ntaps, seed):
    """the library's tables; the oracle's restatement of the same front end gives the same bits"""
    taps = R.make_taps(D, fmt, M, nch, np.random.default_rng(seed), ntaps)
    assert np.array_equal(taps, R.make_taps(O, fmt, M, nch, np.random.default_rng(seed), ntaps))
    return taps


def direct_case(D, O, tune, fmt, M, ntaps, shapes, with_shared_cus):
    W = R.DIRECT_W[(fmt, M)]
    nch = sum(SIZES6)
    nblk = 1
    while nch * nblk * 1024 // (2 * W) < 8192:
        nblk += 1
    nwin = nblk * 1024
    nrun = nch * nwin // (2 * W)                      # runs of one launch at one two-tile body per run
    bodies_per_ch = nwin // W // 2
    # default shape: several tickets per resident wave; shrunk shape (<= 256 waves): >= 5 runs each; RUN_PAIRS = 8 is taken
    # as asked (the launcher falls back to 1 where it does not divide a channel's bodies) and still leaves > 256 runs
    assert nwin % (2 * W) == 0 and nrun >= 8192 and nrun >= 4 * RESIDENT_WAVES and nrun >= 5 * 256
    assert bodies_per_ch % 8 == 0 and nrun // 8 > 2 * 256
    rng = np.random.default_rng(1000 * M + ntaps + len(fmt))
    taps = make_tables(D, O, fmt, M, nch, ntaps, 7 * M + ntaps)
    P = Pairs(O, fmt, M, taps, SIZES6, nwin, rng)
    out = {}
    dec = D.Decoder(nch, decim=M, ntaps=ntaps, nstreams=len(SIZES6), max_blocks=nblk, bitlog=False)
    dec.set_taps(taps)
    for shape in shapes:                               # the switches are read at every launch
        set_shape(tune, shape)
        for k in range(3):
            out[shape[0], k] = got = P.run(dec, k, nblk)
            P.check(got, k, shape[0])
    dec.close()
    set_shape(tune, SHAPES[0])
    names = [s[0] for s in shapes if s[0] != "fallback"]
    if with_shared_cus:
        # no CU partition: one-wave workgroups, seven per CU, beside the demodulator's (read at acg_create)
        tune("ACG_MSK_CUS", "0")
        dec = D.Decoder(nch, decim=M, ntaps=ntaps, nstreams=len(SIZES6), max_blocks=nblk, bitlog=False)
        dec.set_taps(taps)
        for k in range(3):
            out["shared-cus", k] = got = P.run(dec, k, nblk)
            P.check(got, k, "shared-cus")
        dec.close()
        names.append("shared-cus")
    for k in range(3):
        # run length, workgroup shape and who took which run change no sum
        for n in names[1:]:
            assert np.array_equal(out[n, k], out["default", k]), (n, k, int((out[n, k] != out["default", k]).sum()))
        # the fallback kernel adds in another order: close, and not the same bits -- so the others ran the direct kernel
        fb = out["fallback", k]
        assert np.all(np.abs(fb - out["default", k]) <= P.bar[k]), k
        assert not np.array_equal(fb, out["default", k]), k
    print("LEDGER %s M=%d ntaps=%d W=%d nblk=%d runs=%d: worst err/bar %.3f" % (fmt, M, ntaps, W, nblk, nrun, P.worst))


# ------------------------------------------------------------------------------------ direct kernels over many runs
@pytest.mark.parametrize("fmt,M", R.DIRECT, ids=["%s-%d" % c for c in R.DIRECT])
def test_fmt_direct_kernel_many_runs_streams_and_launch_shapes(D, O, fmt, M, tune):
    """fir_fmt_direct_kernel<FMT, CPR, W>, each of its eight instantiations: 40 channels on 6 streams (1, 3, 8, 11, 16 and 1
    channels, scrambled), >= 8192 runs per launch, input rows with a pitch (split: both planes, six rows each).  Launch
    shapes: default; one-wave workgroups, one per CU, with runs of 1, 2 and 8 bodies; two-wave workgroups; no CU partition
    (a second context); the fallback kernel.  Every call, channel and window within the bar of the exact value and of the
    oracle; all direct shapes bit-identical; the fallback within the bar of them and different in at least one bit."""
    direct_case(D, O, tune, fmt, M, M, SHAPES, True)


@pytest.mark.parametrize("fmt,M,ntaps", R.DIRECT_FEWER, ids=["%s-%d-%d" % c for c in R.DIRECT_FEWER])
def test_fmt_direct_kernel_fewer_taps_than_the_window(D, O, fmt, M, ntaps, tune):
    """the same launches with ntaps < M (tap columns beyond ntaps are written as zeros, nck < CPR): default shape, the shrunk
    one and the fallback"""
    direct_case(D, O, tune, fmt, M, ntaps, SHAPES_FEWER, False)


# ------------------------------------------------------------------------------------ the fallback kernel's shapes
@pytest.mark.parametrize("fmt,M", R.FALLBACK, ids=["%s-%d" % c for c in R.FALLBACK])
def test_fmt_fallback_kernel_shapes(D, O, fmt, M, tune):
    """fir_fmt_kernel<FMT>: CS16 M = 164 (41 chunks per window, the odd row stride) and 400 (two LDS slices); split planes at
    M = 8, 200 and 208 (the limit); real f32 at M = 240 and 800 forced onto it (2 x 30 and 4 x 50 chunks).  Seven channels on
    three streams, scrambled, 2 blocks, three (input, map) pairs cycled twice: the second round gives the bits of the first."""
    nch, nblk = sum(SIZES3), 2
    nwin = nblk * 1024
    rng = np.random.default_rng(500 * M + len(fmt))
    taps = make_tables(D, O, fmt, M, nch, M, 3 * M)
    P = Pairs(O, fmt, M, taps, SIZES3, nwin, rng)
    direct = (fmt, M) in R.DIRECT_W
    first = {}
    dec = D.Decoder(nch, decim=M, nstreams=len(SIZES3), max_blocks=nblk, bitlog=False)
    dec.set_taps(taps)
    if direct:
        for k in range(3):
            first["direct", k] = P.run(dec, k, nblk)
    tune("ACG_FIR_VARIANT", "3")
    for rnd in range(2):
        for k in range(3):
            got = P.run(dec, k, nblk)
            P.check(got, k, "round %d" % rnd)
            assert np.array_equal(first.setdefault(k, got), got), (rnd, k)
            if direct:
                assert np.all(np.abs(got - first["direct", k]) <= P.bar[k]) and not np.array_equal(got, first["direct", k]), k
    dec.close()
    print("LEDGER fallback %s M=%d: worst err/bar %.3f" % (fmt, M, P.worst))


@pytest.mark.parametrize("fmt,M", [(R.SPLIT, 216), (R.CS16, 166)])
def test_fmt_window_lengths_without_a_kernel_are_refused(D, fmt, M):
    """split planes longer than one LDS slice (M > 208) and a window that is no whole number of 16-byte chunks: ACG_EINVAL,
    nothing launched"""
    import torch
    from acarsdec_amd import _capi as K
    dec = D.Decoder(2, decim=M, nstreams=1, max_blocks=1, bitlog=False)
    t = torch.zeros(2 * 1024 * M * 4 + 64, dtype=torch.uint8, device="cuda")
    with pytest.raises(K.AcgError) as e:
        dec.process_samples(capi_fmt(fmt), t, 1, pitch=1024 * M * 4, plane=1024 * M * 2 if fmt == R.SPLIT else 0)
    assert e.value.code == K.EINVAL
    dec.close()


# ------------------------------------------------------------------------------------ several streams through the host feed
FREQS7 = [131450000, 131475000, 131525000, 131550000, 131725000, 131825000, 131850000]


@pytest.mark.parametrize("fmt,M", [(R.CS16, 200), (R.SPLIT, 160), (R.F32R, 200)], ids=["cs16", "split16", "f32r"])
def test_fmt_host_feed_with_several_streams(D, O, S, fmt, M):
    """acg_feed_samples_host with three rows (its 2-D copies, the carried partial window of every row): ACARS envelopes, a
    different channel set on each stream, fed in pieces of 5, M - 1, 1, 1000 M + 17 samples and the rest, so windows
    straddle feeds.  Blocks per channel bit-exact against the oracle fed from that channel's own stream; the last launch's dm
    within the bar of the exact value; the same samples from the device through process_samples give the same blocks."""
    rng = np.random.default_rng(90 + M + len(fmt))
    nch, nblk, ns = sum(SIZES3), 4, len(SIZES3)
    nout = nblk * 1024
    smap = scrambled_map(SIZES3, rng)
    rate = R.INTRATE * M
    if fmt == R.F32R:
        fc = D.airspy_choose_fc(FREQS7)
        taps = np.stack([D.airspy_taps(f, fc, rate) for f in FREQS7])
        otaps = [O.air_taps(f, fc, rate) for f in FREQS7]
    elif fmt == R.SPLIT:
        fc = D.choose_fc(FREQS7, M)[0]
        taps = np.stack([D.sdrplay_taps(float(f), fc) for f in FREQS7])
        otaps = [O.sdrplay_taps(float(f), fc) for f in FREQS7]
    else:
        fc = D.choose_fc(FREQS7, M)[0]
        taps = np.stack([D.soapy_taps(float(f), fc, M) for f in FREQS7])
        otaps = [O.soapy_taps(float(f), fc, M) for f in FREQS7]
    env = []
    for c in range(nch):
        a, _ = S.channel_audio(rng, nout, gap=(400, 900), text_len=(3, 25))
        env.append(0.5 * (1 + 0.5 * a))
    env = np.array(env)
    rows = []
    for s in range(ns):                                 # stream s carries the carriers of its own channels only
        chans = np.flatnonzero(smap == s)
        ph = np.linspace(0, 3, nch)[chans]
        if fmt == R.F32R:
            rows.append(S.real_f32_from_envelopes(env[chans], M, [fc - FREQS7[c] + rate / 4 for c in chans], phases=ph, scale=0.15,
                                                  noise=0.01, rng=rng))
        else:
            rows.append(S.iq_s16_from_envelopes(env[chans], M, [FREQS7[c] - fc for c in chans], phases=ph, scale=0.15, noise=0.01,
                                                rng=rng, full_scale=0.06 if fmt == R.SPLIT else 0.9))
    if fmt == R.SPLIT:
        x = (np.stack([r[0::2] for r in rows]), np.stack([r[1::2] for r in rows]))
    else:
        x = np.stack(rows)
    want, nfr = {}, 0
    for c in range(nch):
        ch = O.Channel(c)
        ch.demod(R.oracle(O, fmt, R.row_of(fmt, x, smap[c]), M, otaps[c], nout))
        want[c] = [O.frame_tuple(f) for f in ch.frames]
        nfr += len(want[c])
    assert nfr >= nch - 2
    want = {c: v for c, v in want.items() if v}

    per = 2 if fmt == R.CS16 else 1                     # array elements per sample
    total = nout * M
    dec = D.Decoder(nch, decim=M, nstreams=ns, max_blocks=nblk)
    dec.set_taps(taps)
    dec.set_channel_streams(smap)
    got, pos, last = [], 0, (0, 0)
    for n in (5, M - 1, 1, 1000 * M + 17, total):
        n = min(n, total - pos)
        if fmt == R.SPLIT:
            dec.feed(capi_fmt(fmt), x[0][:, pos: pos + n], x[1][:, pos: pos + n])
        else:
            dec.feed(capi_fmt(fmt), x[:, per * pos: per * (pos + n)])
        if (pos + n) // M > pos // M:
            last = (pos // M, (pos + n) // M)           # the windows this feed completed: one launch
        pos += n
        got += [D.frame_tuple(f) for f in dec.drain_frames()]
    assert pos == total and last == (1001, nout)
    assert by_channel(got) == want
    worst = 0.0
    for c in range(nch):
        ex = R.exact(fmt, R.row_of(fmt, x, smap[c]), M, taps[c], nout)
        dm = dec.dm(c, last[1] - last[0])
        r = np.abs(dm - ex[last[0]:]) / R.bar(ex, fmt)[last[0]:]
        worst = max(worst, float(r.max()))
        assert r.max() <= 1.0, (c, int(smap[c]), r.max(), int(r.argmax()))
    dec.close()
    print("LEDGER feed %s M=%d: worst err/bar %.3f" % (fmt, M, worst))

    dec = D.Decoder(nch, decim=M, nstreams=ns, max_blocks=nblk)
    dec.set_taps(taps)
    dec.set_channel_streams(smap)
    t, pitch, plane = to_device(fmt, x)
    dec.process_samples(capi_fmt(fmt), t, nblk, pitch, plane)
    assert by_channel([D.frame_tuple(f) for f in dec.drain_frames()]) == want
    dec.close()
