"""Exact references, inputs and models for the recordings' sample formats, complex int8 (ACG_FMT_CS8, SigMF ci8) and complex
float32 (ACG_FMT_CF32, SigMF cf32_le): shared by tests/test_iq_format_ref.py (CPU: pins these helpers) and
tests/test_gpu_iq_formats.py.  What tests/format_ref.py is for CS16 / split int16 / real f32; its tap tables, its planting scheme
and its written tolerances are imported, not restated.

The oracle knows neither format.  The references are independent of oracle/: |sum v*osc| of soapy.c:232-254 with only the sample
type changed, every product and the whole sum in float64, the f32 operands taken as they are, the format's power-of-two scale
applied (1/128 for int8, 1 for float32).
"""
import numpy as np

import format_ref as R
import mm_model as MM

CS8, CF32 = "cs8", "cf32"
SCALE = {CS8: 1.0 / 128.0, CF32: 1.0}
NPLANT = R.NPLANT
# CF32: the whole stream times 2^10 / 2^-20 -- a path through integers or f16 cannot pass those under the relative bar
UP_STREAM, DOWN_STREAM = 3, 4
UP, DOWN = np.float32(2.0 ** 10), np.float32(2.0 ** -20)

# the streaming kernels: fir_s8_direct_kernel<cpr> (tiles of 64 windows) and fir_fmt_direct_kernel<5, CPR, 16> (FIRX_LIST in
# csrc/fir.hip): (format, M) -> W, the windows of a tile; a run is two tiles
DIRECT_W = {(CS8, 160): 64, (CS8, 192): 64, (CS8, 200): 64, (CF32, 160): 16, (CF32, 192): 16, (CF32, 200): 16}
DIRECT = sorted(DIRECT_W)
# the workgroup-granular kernels: CS8 at the shortest window, an odd chunk count (168 -> 21) and the limit; CF32 at one chunk per
# window, an odd chunk count (164 -> 82, two LDS slices of 41), several slices (400 -> 4 x 50) and the limit (1024 -> 10 x 52, the last
# slice short)
FALLBACK = [(CS8, 8), (CS8, 168), (CS8, 320), (CF32, 2), (CF32, 164), (CF32, 400), (CF32, 1024)]
REFUSED = [(CS8, 164, "decim % 8"), (CS8, 328, "ACG_MAXDECIM"), (CF32, 161, "decim % 2"), (CF32, 1026, None)]


def capi_fmt(fmt):
    from acarsdec_amd import _capi as K
    return {CS8: K.FMT_CS8, CF32: K.FMT_CF32}[fmt]


def sample_bytes(fmt):
    return 2 if fmt == CS8 else 8


def _rg(fmt, row, M, nout):
    """one stream -> (I, Q) float64 [nout, M] each"""
    x = np.asarray(row)
    assert x.dtype == (np.int8 if fmt == CS8 else np.float32), x.dtype
    x = x.reshape(-1)[: nout * M * 2].astype(np.float64).reshape(nout, M, 2)
    return np.ascontiguousarray(x[:, :, 0]), np.ascontiguousarray(x[:, :, 1])


def exact(fmt, row, M, taps, nout):
    """taps [ntaps, 2] -> float64 [nout]; [k, ntaps, 2] -> [k, nout]"""
    r, g = _rg(fmt, row, M, nout)
    wr, wi = R._w64(taps, M)
    return R._mag(r @ wr - g @ wi, r @ wi + g @ wr, SCALE[fmt], taps)


def bar(exact_dm, fmt):
    """The project's written tolerances, unchanged: CS8 format_ref.bar's flat form 1e-5 |exact| + 1e-6 (its sums are scaled to the
    unit range like CS16's); CF32 the split-int16 form 1e-5 |exact| + 1e-6 max|exact| over the channel's windows (its sums are not
    confined to the unit range)."""
    return R.bar(exact_dm, R.SPLIT if fmt == CF32 else R.CS16)


def make_input(fmt, M, nstreams, nwin, rng, k=0):
    """Full-range input, one row per stream, the extremes planted as format_ref.make_input places them: pattern j at the head of
    stream (j + k) % nstreams, windows [NPLANT k, NPLANT (k + 1)).  CS8: int8 [nstreams, nwin M 2] uniform over [-128, 127]; all
    -128, all 127, I = 127 with Q = -128.  CF32: float32 [nstreams, nwin M 2] uniform in (-1, 1); (1, 1), (-1, -1), (1, -1);
    stream UP_STREAM is scaled by 2^10 and stream DOWN_STREAM by 2^-20 (exact), planted windows included."""
    assert nstreams >= 3 and nwin >= NPLANT * (k + 1)
    w0, w1 = NPLANT * k, NPLANT * (k + 1)
    s = [(j + k) % nstreams for j in range(3)]
    if fmt == CS8:
        x = rng.integers(-128, 128, size=(nstreams, nwin * M * 2), dtype=np.int8)
        pats = ((-128, -128), (127, 127), (127, -128))
    else:
        x = (rng.random((nstreams, nwin * M * 2), dtype=np.float32) * np.float32(2) - np.float32(1)).astype(np.float32)
        x[x <= -1.0] = 0.0                                # the open interval
        pats = ((1.0, 1.0), (-1.0, -1.0), (1.0, -1.0))
    for st, (vi, vq) in zip(s, pats):
        x[st, 2 * w0 * M: 2 * w1 * M: 2] = vi
        x[st, 2 * w0 * M + 1: 2 * w1 * M: 2] = vq
    if fmt == CF32:
        assert nstreams > DOWN_STREAM
        x[UP_STREAM] *= UP
        x[DOWN_STREAM] *= DOWN
    return x


def make_taps(mod, M, nch, rng, ntaps=None):
    """soapy.c's oscillator tables (acg_soapy_taps) as format_ref.make_taps shapes them: a different frequency per channel, one
    table times 1/512, one with exact zeros at the odd indices"""
    return R.make_taps(mod, R.CS16, M, nch, rng, ntaps)


# ---- the reference's own arithmetic, restated in numpy: what the bars leave room for ---------------------------------------
def sequential_f32(fmt, row, M, taps, nout):
    """soapy.c:232-254 in f32, term by term: D += v * osc[ind] with the complex product's four products, its difference and its
    sum each rounded, then the two additions; cabsf as glibc's; the scale.  float32 [nout]"""
    x = np.asarray(row).reshape(-1)[: nout * M * 2].astype(np.float32).reshape(nout, M, 2)
    t = np.zeros((M, 2), dtype=np.float32)
    t[: taps.shape[0]] = taps
    dr, di = np.zeros(nout, dtype=np.float32), np.zeros(nout, dtype=np.float32)
    for n in range(M):
        r, g, wr, wi = x[:, n, 0], x[:, n, 1], t[n, 0], t[n, 1]
        dr = dr + (r * wr - g * wi)
        di = di + (r * wi + g * wr)
    return MM.cabs(dr, di) * np.float32(SCALE[fmt])


def fold_f32(row, M, taps, nout):
    """CS8 as the u8 kernel family computes it: sum (x + 128) w - 128 (1 + j) sum w, every operation in f32 (the bytes xor 0x80
    are x + 128), then |D| / 128.  float32 [nout]"""
    x = np.asarray(row).reshape(-1)[: nout * M * 2].astype(np.float32).reshape(nout, M, 2) + np.float32(128)
    t = np.zeros((M, 2), dtype=np.float32)
    t[: taps.shape[0]] = taps
    dr, di = np.zeros(nout, dtype=np.float32), np.zeros(nout, dtype=np.float32)
    sr, si = np.float32(0), np.float32(0)
    for n in range(M):
        r, g, wr, wi = x[:, n, 0], x[:, n, 1], t[n, 0], t[n, 1]
        dr = dr + (r * wr - g * wi)
        di = di + (r * wi + g * wr)
        sr, si = sr + wr, si + wi
    dr = dr - np.float32(128) * (sr - si)
    di = di - np.float32(128) * (sr + si)
    return MM.cabs(dr, di) * np.float32(1.0 / 128.0)


# ---- the matrix pipe on int8 samples: mm_model's digits and exact sums, the constant term zero -----------------------------
def mm_samples(row, M, nout):
    """the int8 bytes as they are: float64 [nout, 2 M]"""
    x = np.asarray(row)
    assert x.dtype == np.int8
    return x.reshape(-1)[: nout * M * 2].reshape(nout, 2 * M).astype(np.float64)


def mm_sums(row, M, taps_list, nout, check_digits=True):
    """(constants, Sre, Sim): mm_model.exact_sums on the int8 samples"""
    ks = [MM.chan_consts(t, M) for t in taps_list]
    Sre, Sim = MM.exact_sums(mm_samples(row, M, nout), [k.q for k in ks], check_digits)
    return ks, Sre, Sim


def mm_model_dm(row, M, taps_list, nout, check_digits=True):
    """what fir_s8_mm_kernel writes for K tap tables on one int8 stream: re = f32(Sre scale) (one rounding; no constant), likewise
    im, glibc's cabsf, times 1/128 (exact).  float32 [K, nout]"""
    ks, Sre, Sim = mm_sums(row, M, taps_list, nout, check_digits)
    out = []
    for i, k in enumerate(ks):
        if not k.any:
            out.append(np.zeros(nout, dtype=np.float32))
            continue
        re = (Sre[i].astype(np.float64) * k.scale).astype(np.float32)
        im = (Sim[i].astype(np.float64) * k.scale).astype(np.float32)
        out.append(MM.cabs(re, im) * np.float32(1.0 / 128.0))
    return np.stack(out)
