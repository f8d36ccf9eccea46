"""The shared model of the down-converter at any input rate (include/acarsdec_amd.h, "any input sample rate"): the window grid
in Python integers, the exact value of every output, inputs and tap tables, and the two end-to-end fixtures.  Used by
tests/test_rate_ref.py (CPU: pins these helpers and the C helpers against them) and tests/test_gpu_rate.py.

The definition: R the input rate, P / Q = R / 12500 in lowest terms, window k covers samples [s_k, s_(k+1)), s_k = floor(k P / Q),
L_k its length, and  dm_c[k] = scale_fmt / L_k * | sum_{i < L_k} v[s_k + i] t_c[i] |.  `exact` evaluates that with every product
and the whole sum in float64 on the f32 / integer operands as they are.  The bars are the project's written ones, imported from
format_ref / iq_format_ref, not restated.
"""
import math

import numpy as np

import format_ref as R
import iq_format_ref as Q

INTRATE = 12500
CU8, CS8, CS16, CF32 = "cu8", Q.CS8, R.CS16, Q.CF32
FORMATS = [CU8, CS8, CS16, CF32]
DTYPE = {CU8: np.uint8, CS8: np.int8, CS16: np.int16, CF32: np.float32}
SCALE = {CU8: 1.0 / 127.5, CS8: 1.0 / 128.0, CS16: 1.0 / 32768.0, CF32: 1.0}
# rtl.c:338-339 subtracts the float constant
U8_OFFSET = float(np.float32(127.37))
NPLANT = R.NPLANT
UP_STREAM, DOWN_STREAM, UP, DOWN = Q.UP_STREAM, Q.DOWN_STREAM, Q.UP, Q.DOWN
SCALED_CH, ZEROED_CH = R.SCALED_CH, R.ZEROED_CH

# the issue's rates, each for what it reaches
RATES = [2048000, 1024000, 2560000, 31250, 1999999, 3999999, 2500000]


def capi_fmt(fmt):
    from acarsdec_amd import _capi as K
    return {CU8: K.FMT_CU8, CS8: K.FMT_CS8, CS16: K.FMT_CS16, CF32: K.FMT_CF32}[fmt]


def sample_bytes(fmt):
    return 2 * np.dtype(DTYPE[fmt]).itemsize


# ---- the grid, in Python integers ------------------------------------------------------------------------------------------
def pq(rate):
    g = math.gcd(int(rate), INTRATE)
    return int(rate) // g, INTRATE // g


def decim(rate):
    return -(-int(rate) // INTRATE)


def start(rate, k):
    P, Q_ = pq(rate)
    return int(k) * P // Q_


def starts(rate, k0, n):
    """s_k0 .. s_(k0 + n): n + 1 Python integers"""
    P, Q_ = pq(rate)
    return [(int(k0) + i) * P // Q_ for i in range(int(n) + 1)]


def span(rate, k0, n):
    """samples of windows k0 .. k0 + n - 1"""
    return start(rate, k0 + n) - start(rate, k0)


def windows_fit(rate, k0, nsamples):
    """the whole windows from k0 on that fit into nsamples samples beginning at s_k0"""
    P, Q_ = pq(rate)
    n = int(nsamples) * Q_ // P
    while span(rate, k0, n + 1) <= nsamples:
        n += 1
    while n > 0 and span(rate, k0, n) > nsamples:
        n -= 1
    return n


def taps64(rate, offset_hz, n):
    """(cos, -sin) of 2 pi frac(offset i / rate) in float64 with libm (math.cos: what the C helper calls), rounded to float32"""
    out = np.zeros((n, 2), dtype=np.float32)
    for i in range(n):
        turns = float(offset_hz) * float(i) / float(rate)
        ph = 2.0 * math.pi * (turns - float(np.floor(turns)))         # (np.floor keeps the sign of -0.0, as C's floor does)
        out[i, 0] = np.float32(math.cos(ph))
        out[i, 1] = np.float32(-math.sin(ph))
    return out


# ---- the exact value -------------------------------------------------------------------------------------------------------
def complex_samples(fmt, row):
    """one stream's interleaved values -> complex128 samples, the operands as they are"""
    x = np.asarray(row)
    assert x.dtype == DTYPE[fmt], (x.dtype, fmt)
    x = x.reshape(-1).astype(np.float64)
    if fmt == CU8:
        x = x - U8_OFFSET
    return x[0::2] + 1j * x[1::2]


def exact(fmt, row, rate, taps, k0, nwin):
    """`row`: the stream's values beginning at sample s_k0; taps float32 [decim, 2] -> float64 [nwin]"""
    t = np.asarray(taps)
    M = decim(rate)
    assert t.dtype == np.float32 and t.shape == (M, 2)
    v = complex_samples(fmt, row)
    s = np.array(starts(rate, k0, nwin), dtype=np.int64)
    s -= s[0]
    L = np.diff(s)
    assert v.size >= s[-1] and L.min() >= M - 1 and L.max() <= M
    idx = s[:-1, None] + np.arange(M)[None, :]
    inside = np.arange(M)[None, :] < L[:, None]
    w = np.where(inside, v[np.minimum(idx, v.size - 1)], 0.0)
    tc = t[:, 0].astype(np.float64) + 1j * t[:, 1].astype(np.float64)
    return np.abs(w @ tc) * (SCALE[fmt] / L)


def bar(exact_dm, fmt):
    """CU8, CS8, CS16: 1e-5 |x| + 1e-6; CF32: 1e-5 |x| + 1e-6 max|x| over the channel's windows"""
    return R.bar(exact_dm, R.SPLIT if fmt == CF32 else R.CS16)


# ---- inputs and taps -------------------------------------------------------------------------------------------------------
def make_input(fmt, rate, nstreams, k0, nwin, rng, k=0, extra=0):
    """iq_format_ref.make_input's inputs placed on the grid: full range, one row per stream of span(k0, nwin) + extra samples that
    begin at s_k0; the extremes planted at the head of stream (j + k) % nstreams, grid windows [NPLANT k, NPLANT (k + 1)) of the
    row.  CU8: uint8 over [0, 255]; all 0, all 255, I = 255 with Q = 0.  CS8 / CS16 / CF32: as iq_format_ref / format_ref."""
    assert nstreams >= 3 and nwin >= NPLANT * (k + 1)
    s = starts(rate, k0, nwin)
    n = s[-1] - s[0] + int(extra)
    a, b = s[NPLANT * k] - s[0], s[NPLANT * (k + 1)] - s[0]
    st = [(j + k) % nstreams for j in range(3)]
    if fmt == CU8:
        x = rng.integers(0, 256, size=(nstreams, 2 * n), dtype=np.uint8)
        pats = ((0, 0), (255, 255), (255, 0))
    elif fmt == CS8:
        x = rng.integers(-128, 128, size=(nstreams, 2 * n), dtype=np.int8)
        pats = ((-128, -128), (127, 127), (127, -128))
    elif fmt == CS16:
        x = rng.integers(-32768, 32768, size=(nstreams, 2 * n), dtype=np.int16)
        pats = ((-32768, -32768), (32767, 32767), (32767, -32768))
    else:
        x = (rng.random((nstreams, 2 * n), dtype=np.float32) * np.float32(2) - np.float32(1)).astype(np.float32)
        x[x <= -1.0] = 0.0
        pats = ((1.0, 1.0), (-1.0, -1.0), (1.0, -1.0))
    for sidx, (vi, vq) in zip(st, pats):
        x[sidx, 2 * a: 2 * b: 2] = vi
        x[sidx, 2 * a + 1: 2 * b: 2] = vq
    if fmt == CF32:
        assert nstreams > DOWN_STREAM
        x[UP_STREAM] *= UP
        x[DOWN_STREAM] *= DOWN
    return x


def make_taps(mod, rate, nch, rng):
    """format_ref.make_taps' shapes on the rate path's tables (mod.rate_taps: acarsdec_amd.decoder): a different frequency per
    channel, channel SCALED_CH's table times 1/512, channel ZEROED_CH's with exact zeros at the odd indices"""
    ks = rng.permutation(np.concatenate([np.arange(-40, -1), np.arange(2, 41)]))[:nch]
    assert nch > max(SCALED_CH, ZEROED_CH)
    taps = np.stack([np.asarray(mod.rate_taps(rate, 12500.0 * int(k)), dtype=np.float32) for k in ks])
    taps[SCALED_CH] *= np.float32(1.0 / 512.0)
    taps[ZEROED_CH, 1::2] = 0.0
    return np.ascontiguousarray(taps)


# ---- the end-to-end fixtures: three synthetic ACARS channels on one stream -----------------------------------------------------
FREQS3 = [131525000, 131725000, 131825000]
E2E_RATE, E2E_NOUT = 2048000, 4 * 1024
E2E_SEED = {CU8: 31, CF32: 27}


def acars_stream(D, S, fmt, rate, nout, seed, nch=3):
    """test_gpu_iq_formats.acars_streams' traffic on the new synth: `nch` channels at FREQS3 on one clean stream at `rate`, nout
    windows.  Returns (row of the format's values, taps [nch, decim, 2], frames per channel)."""
    rng = np.random.default_rng(seed)
    fc = D.choose_fc(FREQS3, decim(rate))[0]
    offs = [FREQS3[c] - fc for c in range(nch)]
    taps = np.stack([D.rate_taps(rate, offs[c]) for c in range(nch)])
    env, frames = [], []
    for c in range(nch):
        a, fr = S.channel_audio(rng, nout, gap=(400, 900), text_len=(12, 40))
        env.append(0.5 * (1 + 0.5 * a))
        frames.append(fr)
    kw = dict(phases=np.linspace(0, 3, nch), scale=0.3, noise=0.004, rng=rng)
    synth = {CU8: S.iq_u8_at_rate, CS8: S.iq_s8_at_rate, CS16: S.iq_s16_at_rate, CF32: S.iq_cf32_at_rate}[fmt]
    row = synth(np.array(env), rate, offs, **kw)
    if fmt == CF32:
        row = row.view(np.float32)
    assert row.size == 2 * start(rate, nout)
    return row, taps, frames


def frame_fields(fr):
    """a transmitted frame of synth.acars_frame as the fields output.c's split of a downlink gives"""
    body = bytes(b & 0x7F for b in fr[5:-3])
    text = body[13:-1]
    assert body[12] == 0x02 and body[-1] == 0x03 and len(text) >= 12
    return dict(mode=body[0:1], addr=body[2:8], label=body[9:11], bid=body[11:12], no=text[0:4], fid=text[4:10], txt=text[10:])
