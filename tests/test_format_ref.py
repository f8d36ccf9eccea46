"""The float64 references and the generators of tests/format_ref.py against the oracle (CPU): for every (format, M, ntaps)
tests/test_gpu_formats.py runs, at 2048 windows of the same full-range input, the oracle's sequential f32 sum stays within
HALF of the project's dm tolerance of the exact value.  That pins the references on the machine where the oracle is itself
pinned to the reference (tests/test_oracle_vs_ref.py), and shows that the tolerance leaves room: the oracle is an IEEE
-O2 -ffp-contract=off build, so the figures are deterministic (0.02 - 0.12 of the bar)."""
import numpy as np
import pytest

import format_ref as R
from oracle import oracle as O


@pytest.mark.parametrize("fmt,M,ntaps", R.ALL_CASES, ids=["%s-%d-%d" % c for c in R.ALL_CASES])
def test_oracle_is_within_half_the_bar_of_the_exact_reference(fmt, M, ntaps):
    rng = np.random.default_rng(31 * M + ntaps)
    nstreams, nch, nout = 3, 7, 2048
    x = R.make_input(fmt, M, nstreams, nout, rng)
    taps = R.make_taps(O, fmt, M, nch, rng, ntaps)
    assert taps.shape == (nch, ntaps, 2) and taps.dtype == np.float32
    assert len({t.tobytes() for t in taps}) == nch                      # no two channels share a table
    worst = 0.0
    for c in range(nch):
        row = R.row_of(fmt, x, c % nstreams)
        want = R.exact(fmt, row, M, taps[c], nout)
        got = R.oracle(O, fmt, row, M, taps[c], nout)
        assert want.shape == got.shape == (nout,) and np.all(np.isfinite(want))
        worst = max(worst, float((np.abs(got - want) / R.bar(want, fmt)).max()))
    print("%s M=%d ntaps=%d: oracle err / bar = %.3f" % (fmt, M, ntaps, worst))
    assert worst <= 0.5, worst


@pytest.mark.parametrize("fmt", [R.CS16, R.SPLIT, R.F32R])
def test_inputs_span_the_range_and_carry_the_planted_extremes(fmt):
    M, nwin = 16, 512
    a = R.make_input(fmt, M, 3, nwin, np.random.default_rng(1), k=0)
    b = R.make_input(fmt, M, 3, nwin, np.random.default_rng(1), k=1)
    lo, hi = (np.float32(-1), np.float32(1)) if fmt == R.F32R else (-32768, 32767)
    for x, k in ((a, 0), (b, 1)):
        w0, w1 = R.NPLANT * k, R.NPLANT * (k + 1)
        heads = []
        for j in range(3):
            row = R.row_of(fmt, x, (j + k) % 3)
            if fmt == R.CS16:
                heads.append((row[2 * w0 * M: 2 * w1 * M: 2], row[2 * w0 * M + 1: 2 * w1 * M: 2]))
            elif fmt == R.SPLIT:
                heads.append((row[0][w0 * M: w1 * M], row[1][w0 * M: w1 * M]))
            else:
                heads.append((row[w0 * M: w1 * M],) * 2)
        want = ((1, 1), (-1, -1), (0, 0)) if fmt == R.F32R else ((lo, lo), (hi, hi), (hi, lo))
        for (i, q), (vi, vq) in zip(heads, want):
            assert np.all(i == vi) and np.all(q == vq)
    flat = np.concatenate([np.ravel(p) for p in (a if fmt == R.SPLIT else (a,))])
    if fmt == R.F32R:
        assert flat.dtype == np.float32 and flat.min() >= -1 and flat.max() <= 1 and np.abs(flat).max() == 1
        assert flat.min() < -0.99 and flat[np.abs(flat) < 1].max() > 0.99
    else:
        assert flat.dtype == np.int16 and flat.min() == lo and flat.max() == hi
        assert np.unique(flat >> 12).size == 16                        # every top nibble: the whole range, both signs


def test_bar_is_the_written_tolerance():
    e = np.array([[0.0, 2.0, -4.0], [1.0, 0.5, 0.25]])
    assert np.array_equal(R.bar(e, R.CS16), 1e-5 * np.abs(e) + 1e-6)
    assert np.array_equal(R.bar(e, R.F32R), 1e-5 * np.abs(e) + 1e-6)
    assert np.array_equal(R.bar(e, R.SPLIT), 1e-5 * np.abs(e) + 1e-6 * np.array([[4.0], [1.0]]))


def test_exact_references_take_a_batch_of_tables():
    rng = np.random.default_rng(3)
    for fmt in (R.CS16, R.SPLIT, R.F32R):
        M = 24
        x = R.make_input(fmt, M, 3, 64, rng)
        taps = R.make_taps(O, fmt, M, 4, rng, ntaps=16)
        row = R.row_of(fmt, x, 1)
        both = R.exact(fmt, row, M, taps, 64)
        assert both.shape == (4, 64)
        for c in range(4):
            assert np.allclose(both[c], R.exact(fmt, row, M, taps[c], 64), rtol=1e-13, atol=0)
        assert np.all(both[R.SCALED_CH] < both.max()) and np.all(taps[R.ZEROED_CH, 1::2] == 0)
