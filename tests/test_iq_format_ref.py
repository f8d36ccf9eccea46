"""The references of tests/test_gpu_iq_formats.py (tests/iq_format_ref.py), pinned on the CPU: the float64-exact values of complex
int8 and complex float32 input against a numpy restatement of the reference's sequential f32 loop (soapy.c:232-254 with the
sample type changed) and, for int8, of the fold form the u8 kernel family computes -- both must sit far inside the bars the
kernels are held to, so that a kernel that misses a bar is wrong, not unlucky -- and the matrix-pipe model on int8 samples.
"""
import numpy as np
import pytest

import format_ref as R
import iq_format_ref as Q
import mm_model as MM

NWIN, NSTREAMS = 64, 6


@pytest.fixture(scope="module")
def D():
    from acarsdec_amd import decoder
    return decoder


@pytest.mark.parametrize("fmt", [Q.CS8, Q.CF32])
@pytest.mark.parametrize("M", [8, 160, 200, 1024])
def test_exact_references_against_the_sequential_f32_loop(D, fmt, M):
    """Full-range input with the extremes planted (CF32: one stream times 2^10, one times 2^-20): the sequential f32 loop -- and
    for int8 the fold form sum (x + 128) w - 128 (1 + j) sum w -- stays within the bar around the float64-exact value (the figure is printed: a few hundredths)
    on every stream and table (CS8: 1e-5 |exact| + 1e-6; CF32: 1e-5 |exact| + 1e-6 max|exact| over the channel's windows)."""
    rng = np.random.default_rng(77 * M + len(fmt))
    x = Q.make_input(fmt, M, NSTREAMS, NWIN, rng)
    taps = Q.make_taps(D, M, NSTREAMS, np.random.default_rng(M))
    # the planted windows are where make_input says
    pats = ((-128, -128), (127, 127), (127, -128)) if fmt == Q.CS8 else ((1.0, 1.0), (-1.0, -1.0), (1.0, -1.0))
    for s, (vi, vq) in enumerate(pats):
        head = x[s, : 2 * Q.NPLANT * M].reshape(-1, 2)
        assert np.all(head[:, 0] == vi) and np.all(head[:, 1] == vq)
        assert not np.all(x[s, 2 * Q.NPLANT * M: 2 * (Q.NPLANT + 1) * M: 2] == vi)
    if fmt == Q.CF32:
        assert np.abs(x[Q.UP_STREAM]).max() > 512 and 0 < np.abs(x[Q.DOWN_STREAM]).max() < 2.0 ** -20
    worst = 0.0
    for s in range(NSTREAMS):
        ex = Q.exact(fmt, x[s], M, taps[s], NWIN)
        b = Q.bar(ex, fmt)
        assert ex.shape == (NWIN,) and np.all(ex >= 0) and ex.max() > 0
        forms = [Q.sequential_f32(fmt, x[s], M, taps[s], NWIN)] + ([Q.fold_f32(x[s], M, taps[s], NWIN)] if fmt == Q.CS8 else [])
        for got in forms:
            assert got.dtype == np.float32
            r = np.abs(got.astype(np.float64) - ex) / b
            worst = max(worst, float(r.max()))
            assert r.max() <= 1.0, (fmt, M, s, float(r.max()), int(r.argmax()))
    # the scaled streams' values follow the scale: the relative bar is what holds them
    if fmt == Q.CF32:
        assert Q.exact(fmt, x[Q.UP_STREAM], M, taps[0], NWIN).max() > 50 * Q.exact(fmt, x[0], M, taps[0], NWIN)[Q.NPLANT:].max()
        assert Q.exact(fmt, x[Q.DOWN_STREAM], M, taps[0], NWIN).max() < 1e-3
    print("LEDGER %s M=%d: the f32 forms' worst err/bar %.4f" % (fmt, M, worst))


def test_exact_references_are_the_cs16_reference_on_the_same_numbers(D):
    """int8 samples widened to int16 times 256, and float32 samples that are int16 values: format_ref.exact_cs16 gives the same
    sums (scaled by the formats' powers of two) -- the new references restate the same expression"""
    M, rng = 200, np.random.default_rng(5)
    taps = Q.make_taps(D, M, 3, rng)
    x8 = Q.make_input(Q.CS8, M, 3, 16, rng)
    x16 = (x8.astype(np.int16) * np.int16(256)).astype(np.int16)
    for s in range(3):
        a, b = Q.exact(Q.CS8, x8[s], M, taps[s], 16), R.exact_cs16(x16[s], M, taps[s], 16)
        assert np.array_equal(a, b), s
        xf = x16[s].astype(np.float32)
        c = Q.exact(Q.CF32, xf, M, taps[s], 16)
        assert np.array_equal(c, b * 32768.0), s
    many = Q.exact(Q.CS8, x8[0], M, taps, 16)
    assert many.shape == (3, 16) and np.array_equal(many[1], Q.exact(Q.CS8, x8[0], M, taps[1], 16))


@pytest.mark.parametrize("M,ntaps", [(160, 160), (192, 192), (200, 200), (200, 192)])
def test_matrix_model_on_int8_samples(D, M, ntaps):
    """mm_model's digits and exact sums on the int8 samples, the constant term zero: the digit recombination is exact (exact_sums
    checks it), the model is within 2e-7 relative of the float64 value, and its integer sums are the u8 model's on the same bytes
    xor 0x80 -- the two kernels differ only in that xor and the constant.  All-(-128) windows included."""
    rng = np.random.default_rng(31 * M + ntaps)
    nout = 96
    x = rng.integers(-128, 128, size=nout * M * 2, dtype=np.int8)
    x[: 3 * 2 * M] = -128
    x[5 * 2 * M: 7 * 2 * M] = 127
    taps = Q.make_taps(D, M, 11, rng, ntaps)
    taps[4] *= np.float32(2.0 ** -9)
    taps[6] = 0
    tl = [taps[c] for c in range(11)]
    ks, Sre, Sim = Q.mm_sums(x, M, tl, nout, check_digits=True)
    u8 = (x.view(np.uint8) ^ np.uint8(0x80))
    assert np.array_equal(MM.samples(u8, M, nout), Q.mm_samples(x, M, nout))
    Ure, Uim = MM.exact_sums(MM.samples(u8, M, nout), [k.q for k in ks], check_digits=False)
    assert np.array_equal(Sre, Ure) and np.array_equal(Sim, Uim)
    got = Q.mm_model_dm(x, M, tl, nout, check_digits=False)
    assert got.dtype == np.float32 and got.shape == (11, nout) and np.all(got[6] == 0) and not np.signbit(got[6]).any()
    for c in range(11):
        if c == 6:
            continue
        ex = Q.exact(Q.CS8, x, M, taps[c], nout)
        err = np.abs(got[c].astype(np.float64) - ex)
        assert np.all(err <= 2e-7 * ex + 1e-9), (c, float((err / (ex + 1e-9)).max()))
        # ... and apart from the constant it is the u8 model: the same bytes as u8 give a value that differs by the dc term only
    # the all-(-128) windows: every digit sum at its extreme, still exact
    assert np.abs(Sre[:, :3]).max() > 0 and np.array_equal(Sre[:, 0], Sre[:, 1])


def test_python_layer_names_the_formats():
    from acarsdec_amd import _capi as K
    from acarsdec_amd import synth as S
    assert (K.FMT_CS8, K.FMT_CF32) == (4, 5)
    env = np.full((1, 4), 0.5)
    s8 = S.iq_s8_from_envelopes(env, 8, [0.0], scale=4.0)
    assert s8.dtype == np.int8 and s8.size == 64 and s8[0] == 127 and s8[1] == 0          # rint(127 x), clipped
    s8 = S.iq_s8_from_envelopes(env, 8, [0.0], phases=[np.pi], scale=4.0)
    assert s8[0] == -128
    c = S.iq_cf32_from_envelopes(env, 8, [3125.0], scale=0.25)
    assert c.dtype == np.complex64 and c.size == 32
    assert np.array_equal(c, S.iq_complex_from_envelopes(env, 8, [3125.0], scale=0.25).astype(np.complex64))
