"""Channel filters over several windows, CPU side: the C helper acg_channel_filter_taps against the numpy model, the refusals that
need no GPU, the bar of tests/long_ref.py against wrong kernels (it must not hide one), and the end-to-end fixtures of
tests/test_gpu_long_fir.py: decodable with the filter, lost without it, before a GPU sees them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import rate_ref as RR
import long_ref as LR
from acarsdec_amd import _capi as K, decoder as D, synth as S
from oracle import oracle as O


# ------------------------------------------------------------------------------------ the C helper
@pytest.mark.parametrize("rate,nseg", [(2000000, 4), (2500000, 2), (100000, 3), (4000000, 4)])
def test_c_helper_equals_the_numpy_model(rate, nseg):
    """within 1 f32 ulp per component (the two evaluate I0 differently: a power series here, Chebyshev fits in numpy), DC gain 1"""
    M = rate // 12500
    for off in (0.0, 12500.0 * 3, -12500.0 * 17, 12500.0 * 40, 16667.3):
        got = D.channel_filter_taps(rate, off, nseg)
        want = LR.kaiser_taps(rate, off, nseg)
        assert got.shape == want.shape == (nseg * M, 2) and got.dtype == np.float32
        ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
        assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp), (rate, nseg, off)
        # back at DC: the taps times the conjugate oscillator add up to the prototype's gain
        n = np.arange(nseg * M, dtype=np.float64)
        osc = np.exp(2j * np.pi * np.mod(off * n / rate, 1.0))
        gain = ((got[:, 0].astype(np.float64) + 1j * got[:, 1].astype(np.float64)) * osc).sum()
        assert abs(gain - 1.0) < 1e-6, (rate, nseg, off, gain)
    # other cut-offs and windows go through the same code
    got = D.channel_filter_taps(rate, 25000.0, nseg, cutoff_hz=4000.0, beta=3.0)
    want = LR.kaiser_taps(rate, 25000.0, nseg, 4000.0, 3.0)
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.maximum(np.abs(got), np.abs(want))))


def test_c_helper_refusals_and_the_header():
    L = K.load()
    buf = (C.c_float * (2 * 5 * 320))()
    for rate in (2048000, 1999999, 12500, 0):
        assert L.acg_channel_filter_taps(rate, 0.0, 4, 6250.0, 7.0, buf) == K.EINVAL, rate
    for nseg in (0, 1, 5, -1):
        assert L.acg_channel_filter_taps(2000000, 0.0, nseg, 6250.0, 7.0, buf) == K.EINVAL, nseg
    assert L.acg_channel_filter_taps(2000000, 0.0, 4, 6250.0, 7.0, None) == K.EINVAL
    for cutoff, beta in ((0.0, 7.0), (-1.0, 7.0), (1000000.0, 7.0), (6250.0, -1.0), (float("nan"), 7.0)):
        assert L.acg_channel_filter_taps(2000000, 0.0, 4, cutoff, beta, buf) == K.EINVAL, (cutoff, beta)
    assert L.acg_channel_filter_taps(2000000, 0.0, 4, 6250.0, 0.0, buf) == K.OK          # beta 0: the rectangular window
    with pytest.raises(K.AcgError):
        D.channel_filter_taps(2048000, 0.0, 4)
    hdr = open(os.path.join(ROOT, "include", "acarsdec_amd.h")).read()
    assert re.search(r"#define\s+ACG_MAXSEG\s+4\b", hdr) and LR.MAXSEG == 4
    for name in ("acg_set_channel_filter", "acg_channel_filter_taps"):
        assert re.search(r"^int\s+%s\(" % name, hdr, flags=re.M), name
        assert name in K.SYMBOLS and hasattr(L, name)


def test_model_meets_the_boxcar_when_only_the_newest_segment_is_set():
    """taps zero but for the last window's, which hold the boxcar's table times 1 / M: the rate path's definition"""
    rate, M, J, nwin = 2500000, 200, 3, 40
    rng = np.random.default_rng(11)
    x = RR.make_input(RR.CS16, rate, 3, 0, nwin, rng)
    t = D.rate_taps(rate, 62500.0)
    long_t = np.zeros((J * M, 2), dtype=np.float32)
    long_t[(J - 1) * M:] = t
    mine = LR.exact(RR.CS16, LR.with_history([], x[1], M, J), M, J, long_t, nwin, nzero=J - 1) / M
    assert np.allclose(mine, RR.exact(RR.CS16, x[1], rate, t, 0, nwin), rtol=1e-12, atol=1e-15)


# ------------------------------------------------------------------------------------ the bar catches wrong kernels
@pytest.mark.parametrize("M", [160, 320])
@pytest.mark.parametrize("fmt", RR.FORMATS)
def test_the_bar_does_not_hide_a_wrong_kernel(fmt, M):
    """Full-range random input, unit-modulus taps, J = 4, two calls of 203 and 131 windows on six streams.  Each wrong variant
    exceeds the bar at 90 % of the outputs it touches at least: segments in reverse order, the oldest segment dropped, rows
    shifted by one window, the last tap of each segment omitted (all outputs); history taken as zeros in the second call (its
    first J - 1 outputs)."""
    J, rate, ns, n1, n2 = 4, 12500 * M, 6, 203, 131
    rng = np.random.default_rng(M + len(fmt))
    x1 = RR.make_input(fmt, rate, ns, 0, n1, rng, k=0)
    x2 = RR.make_input(fmt, rate, ns, n1, n2, rng, k=1)
    taps = LR.tap_tables("unit", rate, J, ns, np.random.default_rng(7))
    assert np.all(np.abs(np.hypot(taps[..., 0], taps[..., 1]) - 1) < 1e-6)
    over = {k: [] for k in ("reversed", "dropped", "shifted", "last tap", "zero history")}
    for c in range(ns):
        n = n1 + n2
        row = LR.with_history([], np.concatenate([x1[c], x2[c]]), M, J)
        ex = LR.exact(fmt, row, M, J, taps[c], n, nzero=J - 1)
        b = LR.bar(fmt, row, M, J, taps[c], n, ex, nzero=J - 1)
        assert np.all(b > 0)
        t = taps[c].reshape(J, M, 2)
        rev = np.ascontiguousarray(t[::-1]).reshape(J * M, 2)
        drop, last = t.copy(), t.copy()
        drop[0] = 0
        last[:, M - 1] = 0
        wrong = lambda tt: LR.exact(fmt, row, M, J, tt.reshape(J * M, 2), n, nzero=J - 1)
        over["reversed"].append(np.abs(wrong(rev) - ex) > b)
        over["dropped"].append(np.abs(wrong(drop) - ex) > b)
        over["last tap"].append(np.abs(wrong(last) - ex) > b)
        over["shifted"].append(np.abs(ex[:-1] - ex[1:]) > b[1:])             # output k made of output k - 1's windows
        row2 = LR.with_history([x1[c]], x2[c], M, J)
        ex2 = LR.exact(fmt, row2, M, J, taps[c], n2)
        assert np.allclose(ex2, ex[n1:], rtol=1e-12)                         # the second call continues the first
        z2 = LR.exact(fmt, row2, M, J, taps[c], n2, nzero=J - 1)
        over["zero history"].append((np.abs(z2 - ex2) > LR.bar(fmt, row2, M, J, taps[c], n2, ex2))[: J - 1])
        assert np.array_equal(z2[J - 1:], ex2[J - 1:])
    share = {k: float(np.concatenate(v).mean()) for k, v in over.items()}
    print("LEDGER long wrong variants %s M=%d: %s" % (fmt, M, ", ".join("%s %.3f" % kv for kv in share.items())))
    assert all(v >= 0.9 for v in share.values()), share


# ------------------------------------------------------------------------------------ the end-to-end fixtures
@pytest.mark.parametrize("fmt", [RR.CF32, RR.CS16])
def test_fixtures_decode_with_the_filter_and_not_without(fmt):
    """Three ACARS channels on one stream at 2.0 Msps and an unmodulated carrier 16 667 Hz above channel 0 at 16 x (24 dB) its
    carrier amplitude -- the level the issue names, and it separates the two definitions on the quantised rows.  The oracle on
    long_ref.exact (J = 4, cut-off 6250 Hz, beta 7) queues every transmitted frame of all three channels with err == 0; on
    rate_ref.exact, today's boxcar, fewer than half of channel 0's."""
    row, box, filt, frames = LR.interferer_stream(D, S, fmt)
    M, J, nout = LR.E2E_RATE // 12500, LR.E2E_J, LR.E2E_NOUT
    assert all(len(f) >= 2 for f in frames)
    rowh = LR.with_history([], row, M, J)
    for c in range(3):
        want = [fr[5:-3] for fr in frames[c]]
        ch = O.Channel(c)
        ch.demod(LR.exact(fmt, rowh, M, J, filt[c], nout, nzero=J - 1).astype(np.float32))
        got = [bytes(f.txt[: f.len]) for f in ch.frames]
        assert got == want and all(f.err == 0 for f in ch.frames), (fmt, c, len(got), len(want))
    ch = O.Channel(0)
    ch.demod(RR.exact(fmt, row, LR.E2E_RATE, box[0], 0, nout).astype(np.float32))
    want = [fr[5:-3] for fr in frames[0]]
    assert 2 * sum(bytes(f.txt[: f.len]) in want for f in ch.frames) < len(want), (fmt, len(ch.frames), len(want))
