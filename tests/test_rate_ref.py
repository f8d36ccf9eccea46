"""Any input rate, CPU side: the C helpers of the window grid (acg_rate_decim, acg_rate_window_starts, acg_rate_taps) against
Python integers and float64, the grid's properties, the refusals that need no GPU, the model's consistency with the integer
case, and the end-to-end fixtures of tests/test_gpu_rate.py: decodable before a GPU sees them."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import rate_ref as RR
import format_ref as R
from acarsdec_amd import _capi as K, decoder as D, synth as S
from oracle import oracle as O


def k0s(rate):
    return [0, 1061, RR.pq(rate)[1] - 1, 2 ** 40 + 7]


@pytest.mark.parametrize("rate", RR.RATES)
def test_c_grid_and_taps_equal_python(rate):
    M = RR.decim(rate)
    assert D.rate_decim(rate) == M == math.ceil(rate / 12500)
    for k0 in k0s(rate):
        got = D.rate_window_starts(rate, k0, 300)
        assert [int(v) for v in got] == RR.starts(rate, k0, 300) == S.rate_window_starts(rate, k0, 300), (rate, k0)
    for off in (25000.0, -487500.0, 131725000.0 - 131850000.0, 0.0, 12500.5):
        assert np.array_equal(D.rate_taps(rate, off).view(np.uint32), RR.taps64(rate, off, M).view(np.uint32)), (rate, off)
    t = D.rate_taps(rate, 25000.0)
    assert t.shape == (M, 2) and t[0].tolist() == [1.0, 0.0] and np.all(np.abs(np.hypot(t[:, 0], t[:, 1]) - 1) < 1e-6)


@pytest.mark.parametrize("rate", RR.RATES)
def test_window_lengths_are_floor_or_ceil_and_the_grid_repeats_after_q(rate):
    P, Q = RR.pq(rate)
    assert Q == 12500 // math.gcd(rate, 12500) and 12500 % Q == 0 and P * 12500 == rate * Q
    for k0 in k0s(rate):
        s = RR.starts(rate, k0, Q + 300)
        L = np.diff(np.array(s, dtype=object)).astype(np.int64)
        assert set(L.tolist()) <= {P // Q, -(-P // Q)}, (rate, k0)
        assert all(s[i + Q] - s[i] == P for i in range(300))
        assert RR.windows_fit(rate, k0, s[40] - s[0]) == 40 and RR.windows_fit(rate, k0, s[40] - s[0] - 1) == 39
    if Q == 1:
        assert RR.starts(rate, 5, 3) == [5 * P, 6 * P, 7 * P, 8 * P]
    if rate == 1999999:
        assert Q == 12500 and RR.span(rate, 0, 1) == 159 and RR.decim(rate) == 160       # window 0 is the short one
    if rate == 31250:
        assert (P, Q) == (5, 2) and RR.starts(rate, 0, 4) == [0, 2, 5, 7, 10]


def test_out_of_range_rates_and_the_header():
    L = K.load()
    buf = (C.c_ulonglong * 4)()
    taps = (C.c_float * 8)()
    for bad in (0, 12500, 24999, 12500 * K.MAXDECIM + 1, 2 ** 32 - 1):
        assert L.acg_rate_decim(bad) == K.EINVAL
        assert L.acg_rate_window_starts(bad, 0, 3, buf) == K.EINVAL
        assert L.acg_rate_taps(bad, 0.0, 4, taps) == K.EINVAL
    assert L.acg_rate_decim(25000) == 2 and L.acg_rate_decim(12500 * K.MAXDECIM) == K.MAXDECIM
    assert L.acg_rate_window_starts(2048000, 0, -1, buf) == K.EINVAL and L.acg_rate_window_starts(2048000, 0, 3, None) == K.EINVAL
    assert L.acg_rate_taps(2048000, 0.0, 0, taps) == K.EINVAL and L.acg_rate_taps(2048000, 0.0, 4, None) == K.EINVAL
    hdr = open(os.path.join(ROOT, "include", "acarsdec_amd.h")).read()
    assert re.search(r"#define\s+ACG_FMT_CU8\s+6\b", hdr) and K.FMT_CU8 == 6
    for name in ("acg_rate_decim", "acg_rate_window_starts", "acg_rate_taps", "acg_set_input_rate", "acg_process_rate_dev",
                 "acg_feed_rate_host"):
        assert re.search(r"^int\s+%s\(" % name, hdr, flags=re.M), name
        assert name in K.SYMBOLS and hasattr(L, name)


def test_model_meets_the_integer_case_and_the_synth_holds_windows_on_the_grid():
    """Q == 1: the model is format_ref's exact value with the 1 / M moved out of the table.  And the synth's membership rule: a
    unit envelope on a zero-offset carrier is one constant sample per window, so every window's exact value is its envelope."""
    rate, M, nwin = 2500000, 200, 40
    rng = np.random.default_rng(5)
    x = R.make_input(R.CS16, M, 3, nwin, rng)
    t = D.rate_taps(rate, 62500.0)
    mine = RR.exact(RR.CS16, x[1], rate, t, 7, nwin)
    theirs = R.exact_cs16(x[1], M, t, nwin) / M
    assert np.allclose(mine, theirs, rtol=1e-12, atol=1e-15)
    for r in (2048000, 31250, 1999999):
        env = rng.random((1, 50))
        z = S.iq_complex_at_rate(env, r, [0.0], scale=1.0)
        row = np.empty(2 * z.size, dtype=np.float32)
        row[0::2], row[1::2] = z.real, z.imag
        ones = np.zeros((RR.decim(r), 2), dtype=np.float32)
        ones[:, 0] = 1
        assert z.size == RR.start(r, 50)
        assert np.allclose(RR.exact(RR.CF32, row, r, ones, 0, 50), env[0].astype(np.float32), rtol=1e-6)


@pytest.mark.parametrize("fmt", [RR.CU8, RR.CF32])
def test_end_to_end_fixtures_are_decodable_before_a_gpu_sees_them(fmt):
    """The two fixtures of tests/test_gpu_rate.py's end-to-end test: the oracle's demodulator on the float64 model's dm, rounded
    to f32, queues every transmitted frame of every channel (neighbour leakage is no exact null at L in {163, 164})."""
    row, taps, frames = RR.acars_stream(D, S, fmt, RR.E2E_RATE, RR.E2E_NOUT, RR.E2E_SEED[fmt])
    assert all(len(f) >= 1 for f in frames)
    for c in range(3):
        dm = RR.exact(fmt, row, RR.E2E_RATE, taps[c], 0, RR.E2E_NOUT).astype(np.float32)
        ch = O.Channel(c)
        ch.demod(dm)
        got = [bytes(f.txt[: f.len]) for f in ch.frames]
        want = [fr[5:-3] for fr in frames[c]]
        assert got == want and all(f.err == 0 for f in ch.frames), (fmt, c, len(got), len(want))
