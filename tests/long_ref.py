"""The shared model of the channel filter over several windows (include/acarsdec_amd.h, "channel filters"; the kernel:
csrc/fir_long.hip).  Used by tests/test_long_ref.py (CPU: pins the C helper, shows that the bar catches wrong kernels, holds the
end-to-end fixtures decodable) and tests/test_gpu_long_fir.py.

The definition, at a rate R = 12500 M (Q == 1), J windows of taps t[n], n < J M, index 0 for the oldest sample:

    dm[k] = scale_fmt * | sum_{n < J M} v[(k - J + 1) M + n] t[n] |,      v[i] = 0 before the context's first sample.

`exact` evaluates that with every product and the whole sum in float64 on the f32 / integer operands as they are (CU8:
np.float32(I) - np.float32(127.37) in f32, then float64).  The tolerance is derived, not measured: a bound on the error of an f32
dot product, plus the final |.| and scale,

    bar[k] = scale_fmt * BAR_TERMS * 2^-24 * sum_n (|Re v_n| + |Im v_n|) (|Re t_n| + |Im t_n|)  +  2^-22 * exact[k]

over the J M samples of output k.  The worst-case bound for 2 J M products added in ANY order has BAR_TERMS = 2 J M + 16; with it
the variant "last tap of each segment omitted" stays under the bar at 16 % of the outputs at M = 320 (test_long_ref.py wants a
wrong kernel over it at 90 %), so the constant is shortened to what the contract's FIXED order of additions allows.  A product
passes through as many roundings as there are additions between it and the result (the products are fused, the operands exact):
  * its wave's accumulator chain: the window's ceil(M b / 16) chunks go through in K slices (csrc/fir_grid.h: at most 35 chunks
    and a third of a CU's LDS each), a wave takes at most ceil(chunks of the slice / 4) of them, so with S samples per chunk the
    chain is at most M / 4 + S / 4 + 3 K S / 4 <= M / 4 + 14 samples long for every format at M <= 320 (K S <= 16: two slices
    of 8-sample chunks for the 1-byte formats, three of 4, five of 2);
  * two additions across the four waves, one between the two halves of a component (re = rr - ii, im = ri + ir), J - 1 <= 3
    across the segments.
That is M / 4 + 20 roundings at most, each of relative size 2^-24, on a term of the sum of absolute values above (re and im
errors added, which bounds the error of |D|); BAR_TERMS = M / 4 + 24 leaves the second-order terms their room.  2^-22 exact[k]
covers |.| (the double-precision hypot, one narrowing) and the multiplication by scale_fmt.
"""
import math

import numpy as np

import rate_ref as RR

CU8, CS8, CS16, CF32 = RR.CU8, RR.CS8, RR.CS16, RR.CF32
MAXSEG = 4
U8_OFFSET32 = np.float32(127.37)


def complex_samples(fmt, row):
    """one stream's interleaved values -> complex128 samples, the operands as the kernel has them"""
    x = np.asarray(row).reshape(-1)
    assert x.dtype == RR.DTYPE[fmt], (x.dtype, fmt)
    if fmt == CU8:
        x = x.astype(np.float32) - U8_OFFSET32          # rounded once to f32, per sample (rtl.c:338-339)
        assert x.dtype == np.float32
    x = x.astype(np.float64)
    return x[0::2] + 1j * x[1::2]


def _windows(fmt, row_with_history, M, J, nwin, nzero):
    v = complex_samples(fmt, row_with_history)
    assert v.size >= (J - 1 + nwin) * M and 0 <= nzero <= J - 1
    w = v[: (J - 1 + nwin) * M].reshape(J - 1 + nwin, M).copy()
    w[:nzero] = 0.0                                     # windows before the context's first sample: v = 0, whatever the row holds
    return w


def _taps(taps, M, J):
    t = np.asarray(taps)
    assert t.dtype == np.float32 and t.shape == (J * M, 2), (t.dtype, t.shape)
    return (t[:, 0].astype(np.float64) + 1j * t[:, 1].astype(np.float64)).reshape(J, M)


def exact(fmt, row_with_history, M, J, taps, nwin, nzero=0):
    """`row_with_history`: the stream's values beginning J - 1 windows before output 0's own window ((J - 1 + nwin) M samples);
    the first `nzero` of those windows lie before the context's first sample.  taps float32 [J M, 2] -> float64 [nwin]"""
    w = _windows(fmt, row_with_history, M, J, nwin, nzero)
    tc = _taps(taps, M, J)
    d = np.zeros(nwin, dtype=np.complex128)
    for j in range(J):
        d += (w @ tc[j])[j: j + nwin]
    return np.abs(d) * RR.SCALE[fmt]


def BAR_TERMS(M, J):
    assert M <= 320 and 2 <= J <= MAXSEG
    return M / 4.0 + 24.0


def bar(fmt, row_with_history, M, J, taps, nwin, exact_dm, nzero=0):
    w = _windows(fmt, row_with_history, M, J, nwin, nzero)
    wa = np.abs(w.real) + np.abs(w.imag)
    tc = _taps(taps, M, J)
    ta = np.abs(tc.real) + np.abs(tc.imag)
    s = np.zeros(nwin)
    for j in range(J):
        s += (wa @ ta[j])[j: j + nwin]
    return RR.SCALE[fmt] * BAR_TERMS(M, J) * 2.0 ** -24 * s + 2.0 ** -22 * np.asarray(exact_dm)


def with_history(prev_rows, row, M, J):
    """the row of a call behind the last J - 1 windows of what came before it (prev_rows: the earlier calls' rows of one stream,
    oldest first; fewer samples than J - 1 windows: padded with zeros in front, which the caller masks with nzero)"""
    dt = np.asarray(row).dtype
    before = np.concatenate([np.asarray(p, dtype=dt).reshape(-1) for p in prev_rows]) if prev_rows else np.zeros(0, dtype=dt)
    need = 2 * (J - 1) * M
    before = before[-need:] if before.size >= need else np.concatenate([np.zeros(need - before.size, dtype=dt), before])
    return np.concatenate([before, np.asarray(row).reshape(-1)])


# ---- tap tables ------------------------------------------------------------------------------------------------------------
def kaiser_taps(rate, offset_hz, J, cutoff_hz=6250.0, beta=7.0):
    """the model of acg_channel_filter_taps: np.kaiser x np.sinc, DC gain 1, times (cos, -sin) of 2 pi frac(offset n / rate) with
    libm (math.cos: what the C helper calls), everything in float64, rounded once to float32 [J M, 2]"""
    assert rate % RR.INTRATE == 0
    n = J * (rate // RR.INTRATE)
    i = np.arange(n, dtype=np.float64)
    h = np.sinc(2.0 * float(cutoff_hz) / float(rate) * (i - 0.5 * (n - 1))) * np.kaiser(n, float(beta))
    h = h / h.sum()
    out = np.zeros((n, 2), dtype=np.float32)
    for k in range(n):
        turns = float(offset_hz) * float(k) / float(rate)
        ph = 2.0 * math.pi * (turns - float(np.floor(turns)))
        out[k, 0] = np.float32(h[k] * math.cos(ph))
        out[k, 1] = np.float32(h[k] * -math.sin(ph))
    return out


UNIT_SKEW_HZ = 3125.0


def unit_taps(rate, offset_hz, J):
    """the bare oscillator over all J windows: unit modulus, so every term of the sum counts.  (Repeated per window -- which it
    is at a multiple of 12.5 kHz -- the J segments would be one table and their order invisible: tap_tables puts the channels a
    quarter of the raster off it, a quarter turn from segment to segment.)"""
    return RR.taps64(rate, offset_hz, J * (rate // RR.INTRATE))


def tap_tables(kind, rate, J, nch, rng, D=None):
    """a different frequency per channel (rate_ref.make_taps' choice of offsets): kind "unit" or "kaiser" (the C helper's, D =
    acarsdec_amd.decoder)"""
    ks = rng.permutation(np.concatenate([np.arange(-40, -1), np.arange(2, 41)]))[:nch]
    if kind == "unit":
        return np.stack([unit_taps(rate, 12500.0 * int(k) + UNIT_SKEW_HZ, J) for k in ks])
    return np.stack([np.asarray(D.channel_filter_taps(rate, 12500.0 * int(k), J), dtype=np.float32) for k in ks])


# ---- the decodability fixtures: three ACARS channels and a strong carrier off the raster on one stream ---------------------------
E2E_RATE, E2E_NOUT, E2E_J = 2000000, 16 * 1024, 4
E2E_SEED = {CF32: 57, CS16: 58}
E2E_LEVEL = 16                      # the interferer's amplitude as a multiple of channel 0's carrier amplitude
E2E_OFFSET = 16667.0                # Hz above channel 0: the 8.33 kHz raster


def interferer_stream(D, S, fmt, level=E2E_LEVEL):
    """rate_ref.acars_stream's three channels at FREQS3 on one stream at 2.0 Msps, 16 384 windows, env = 0.5 (1 + 0.5 a), scale
    0.05, noise 0.0004, plus an unmodulated carrier E2E_OFFSET above channel 0 with `level` times its carrier amplitude.  Returns
    (row, boxcar taps [3, M, 2], filter taps [3, J M, 2], frames per channel)."""
    rate, nout = E2E_RATE, E2E_NOUT
    rng = np.random.default_rng(E2E_SEED[fmt])
    M = rate // RR.INTRATE
    fc = D.choose_fc(RR.FREQS3, M)[0]
    offs = [RR.FREQS3[c] - fc for c in range(3)]
    env, frames = [], []
    for c in range(3):
        a, fr = S.channel_audio(rng, nout, gap=(400, 900), text_len=(12, 40))
        env.append(0.5 * (1 + 0.5 * a))
        frames.append(fr)
    env.append(np.full(nout, 0.5 * level))
    kw = dict(phases=np.linspace(0, 3, 4), scale=0.05, noise=0.0004, rng=rng)
    synth = {CS16: S.iq_s16_at_rate, CF32: S.iq_cf32_at_rate}[fmt]
    row = synth(np.array(env), rate, offs + [offs[0] + E2E_OFFSET], **kw)
    if fmt == CF32:
        row = row.view(np.float32)
    assert row.size == 2 * M * nout
    box = np.stack([D.rate_taps(rate, offs[c]) for c in range(3)])
    filt = np.stack([D.channel_filter_taps(rate, offs[c], E2E_J) for c in range(3)])
    return row, box, filt, frames
