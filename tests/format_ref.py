"""Exact references, inputs and tap tables for the sample-format down-converters (CS16 / split int16 / real f32):
shared by tests/test_format_ref.py (CPU: pins these helpers against the oracle) and tests/test_gpu_formats.py.

The references are independent of oracle/: |sum x*w| of soapy.c:232-254 / sdrplay.c:215-236 / air.c:299-338 with every
product and the whole sum in float64 -- the f32 operands taken as they are, the format's power-of-two output scale
applied -- i.e. what an infinitely precise evaluation of the reference's expression gives (the shape of exact_dm in
tests/test_gpu_round6.py).
"""
import numpy as np

INTRATE = 12500
CS16, SPLIT, F32R = "cs16", "split16", "f32r"
SCALE = {CS16: 1.0 / 32768.0, SPLIT: 0.25, F32R: 1.0}

# the eight instantiations of fir_fmt_direct_kernel<FMT, CPR, W> (FIRX_TRY in csrc/fir.hip): (format, M) -> W, the windows
# of a tile; a run is two tiles
DIRECT_W = {(CS16, 160): 32, (CS16, 192): 32, (CS16, 200): 32,
            (F32R, 200): 32, (F32R, 240): 16, (F32R, 480): 8, (F32R, 800): 8,
            (SPLIT, 160): 64}
DIRECT = sorted(DIRECT_W)
# fewer taps than the window: the kernel's zero tap columns (nck < CPR)
DIRECT_FEWER = [(f, M, M - 8) for f, M in DIRECT] + [(CS16, 200, 40)]
# the workgroup-granular fallback fir_fmt_kernel: an odd chunk count per window (164 -> 41), two / three / four LDS slices
# (400, 240 and 800 forced onto it), split planes at the shortest window, a length without a direct kernel and the limit
FALLBACK = [(CS16, 164), (CS16, 400), (SPLIT, 8), (SPLIT, 200), (SPLIT, 208), (F32R, 240), (F32R, 800)]
# every (format, M, ntaps) the GPU file runs
ALL_CASES = sorted(set([(f, M, M) for f, M in DIRECT] + DIRECT_FEWER + [(f, M, M) for f, M in FALLBACK]))


def _w64(taps, M):
    """[ntaps, 2] or [k, ntaps, 2] float32 -> float64 (wr, wi), each [M, k], the tail beyond ntaps zero"""
    t = np.asarray(taps)
    assert t.dtype == np.float32 and t.shape[-1] == 2 and t.shape[-2] <= M
    t = t.reshape(-1, t.shape[-2], 2)
    w = np.zeros((M, t.shape[0], 2), dtype=np.float64)
    w[: t.shape[1]] = t.astype(np.float64).transpose(1, 0, 2)
    return w[:, :, 0], w[:, :, 1]


def _mag(re, im, scale, taps):
    d = np.hypot(re, im).T * scale                       # [k, nout]
    return d[0] if np.asarray(taps).ndim == 2 else d


def exact_cs16(iq, M, taps, nout):
    """soapy.c:232-254: interleaved int16 I,Q; |D| / 32768.  taps [ntaps, 2] -> [nout]; [k, ntaps, 2] -> [k, nout]."""
    iq = np.asarray(iq)
    assert iq.dtype == np.int16
    x = iq.reshape(-1)[: nout * M * 2].astype(np.float64).reshape(nout, M, 2)
    r, g = np.ascontiguousarray(x[:, :, 0]), np.ascontiguousarray(x[:, :, 1])
    wr, wi = _w64(taps, M)
    return _mag(r @ wr - g @ wi, r @ wi + g @ wr, SCALE[CS16], taps)


def exact_split16(xi, xq, M, taps, nout):
    """sdrplay.c:215-236: an int16 I plane and an int16 Q plane; |D| / 4."""
    xi, xq = np.asarray(xi), np.asarray(xq)
    assert xi.dtype == np.int16 and xq.dtype == np.int16
    r = xi.reshape(-1)[: nout * M].astype(np.float64).reshape(nout, M)
    g = xq.reshape(-1)[: nout * M].astype(np.float64).reshape(nout, M)
    wr, wi = _w64(taps, M)
    return _mag(r @ wr - g @ wi, r @ wi + g @ wr, SCALE[SPLIT], taps)


def exact_f32r(x, M, taps, nout):
    """air.c:299-338: real float32 samples against complex taps; |D|."""
    x = np.asarray(x)
    assert x.dtype == np.float32
    s = x.reshape(-1)[: nout * M].astype(np.float64).reshape(nout, M)
    wr, wi = _w64(taps, M)
    return _mag(s @ wr, s @ wi, SCALE[F32R], taps)


def exact(fmt, row, M, taps, nout):
    """`row`: one stream as make_input returns it (split int16: the (I, Q) pair)"""
    if fmt == CS16:
        return exact_cs16(row, M, taps, nout)
    if fmt == SPLIT:
        return exact_split16(row[0], row[1], M, taps, nout)
    return exact_f32r(row, M, taps, nout)


def oracle(O, fmt, row, M, taps, nout):
    """the oracle (oracle/acars_oracle.c) on one stream and one table; it knows no ntaps: the tail taps are zero"""
    t = np.zeros((M, 2), dtype=np.float32)
    t[: taps.shape[0]] = taps
    if fmt == CS16:
        return O.fir_cs16(row, M, t, nout=nout)
    if fmt == SPLIT:
        return O.fir_split16(row[0], row[1], M, t, nout=nout)
    return O.fir_f32r(row, M, t, nout=nout)


def bar(exact_dm, fmt):
    """The project's written tolerance for dm (tests/test_gpu_parity.py), unchanged: 1e-5 |exact| + 1e-6 for CS16 and real
    f32; 1e-5 |exact| + 1e-6 max|exact| (over the channel's windows, the last axis) for split int16, whose sums are not
    scaled down to the unit range."""
    a = np.abs(np.asarray(exact_dm, dtype=np.float64))
    if fmt == SPLIT:
        return 1e-5 * a + 1e-6 * a.max(axis=-1, keepdims=True)
    return 1e-5 * a + 1e-6


def row_of(fmt, x, s):
    """stream s of an input of make_input"""
    return (x[0][s], x[1][s]) if fmt == SPLIT else x[s]


NPLANT = 3      # windows per planted pattern


def make_input(fmt, M, nstreams, nwin, rng, k=0):
    """Full-range input, one row per stream: int16 uniform over [-32768, 32767], f32 uniform in (-1, 1).  At the head of
    distinct streams NPLANT windows each of the extremes: int16 all -32768, all 32767, I = 32767 with Q = -32768; f32 all
    +1.0, all -1.0, all zero.  `k` numbers the inputs of one test: pattern j goes to stream (j + k) % nstreams at windows
    [NPLANT k, NPLANT (k + 1)), so that two inputs never carry the same planted window in the same place.
    Returns CS16: int16 [nstreams, nwin M 2]; split: (I, Q), int16 [nstreams, nwin M] each; f32: float32 [nstreams, nwin M]."""
    assert nstreams >= 3 and nwin >= NPLANT * (k + 1)
    w0, w1 = NPLANT * k, NPLANT * (k + 1)
    s = [(j + k) % nstreams for j in range(3)]
    if fmt == F32R:
        x = (rng.random((nstreams, nwin * M), dtype=np.float32) * np.float32(2) - np.float32(1)).astype(np.float32)
        x[x <= -1.0] = 0.0                                # the open interval
        for st, v in zip(s, (1.0, -1.0, 0.0)):
            x[st, w0 * M: w1 * M] = v
        return x
    if fmt == CS16:
        x = rng.integers(-32768, 32768, size=(nstreams, nwin * M * 2), dtype=np.int16)
        for st, (vi, vq) in zip(s, ((-32768, -32768), (32767, 32767), (32767, -32768))):
            x[st, 2 * w0 * M: 2 * w1 * M: 2] = vi
            x[st, 2 * w0 * M + 1: 2 * w1 * M: 2] = vq
        return x
    xi = rng.integers(-32768, 32768, size=(nstreams, nwin * M), dtype=np.int16)
    xq = rng.integers(-32768, 32768, size=(nstreams, nwin * M), dtype=np.int16)
    for st, (vi, vq) in zip(s, ((-32768, -32768), (32767, 32767), (32767, -32768))):
        xi[st, w0 * M: w1 * M] = vi
        xq[st, w0 * M: w1 * M] = vq
    return xi, xq


FC = 131000000
SCALED_CH, ZEROED_CH = 1, 2


def front_end_taps(mod, fmt, M, offset_hz):
    """The front end's own table for a channel `offset_hz` above the centre, float32 [M, 2].  `mod` is acarsdec_amd.decoder
    or oracle.oracle (both restate soapy.c:163-166, sdrplay.c:160-164, air.c:278-285).  sdrplay.c exists at M = 160 only:
    split planes at another window length take soapy.c's oscillator of that length, the same formula."""
    if fmt == F32R:
        air = getattr(mod, "airspy_taps", None) or mod.air_taps
        return air(FC + int(offset_hz), FC, INTRATE * M)
    if fmt == SPLIT and M == 160:
        return mod.sdrplay_taps(float(FC + offset_hz), FC)
    return mod.soapy_taps(float(FC + offset_hz), FC, M)


def make_taps(mod, fmt, M, nch, rng, ntaps=None):
    """[nch, ntaps, 2] float32: a DIFFERENT frequency per channel (a table taken from the wrong channel cannot pass), channel
    SCALED_CH's table times 1/512 (exact), channel ZEROED_CH's with exact zeros at the odd indices; ntaps < M cuts the
    tables short."""
    ntaps = M if ntaps is None else ntaps
    # offsets on the 12.5 kHz raster, 25 kHz <= |offset| <= 500 kHz: chooseFc never puts the centre closer than 2 * INTRATE
    # to a channel (rtl.c:158, sdrplay.c:69), and air.c keeps |offset| < Fs / 4
    ks = rng.permutation(np.concatenate([np.arange(-40, -1), np.arange(2, 41)]))[:nch]
    assert ks.size == nch and nch > max(SCALED_CH, ZEROED_CH)
    taps = np.stack([np.asarray(front_end_taps(mod, fmt, M, 12500 * int(k)), dtype=np.float32) for k in ks])
    taps[SCALED_CH] *= np.float32(1.0 / 512.0)
    taps[ZEROED_CH, 1::2] = 0.0
    return np.ascontiguousarray(taps[:, :ntaps])
