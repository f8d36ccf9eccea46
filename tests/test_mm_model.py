"""tests/mm_model.py, the bit-exact model the matrix-pipe down-converters are held to (tests/test_gpu_mm_shapes.py), checked on
the CPU: it sits inside the two bars the kernels carry (2e-7 of the f64-exact value, 1e-5 of the oracle), and equality with it
tells apart what the 2e-7 bar cannot."""
import numpy as np
import pytest

import mm_model as MM
from oracle import oracle as O

SHAPES = [(200, 200), (160, 160), (192, 192), (200, 192), (160, 37)]
NOUT = 512


def inputs(M, ntaps, nch=4):
    rng = np.random.default_rng(500 * M + ntaps)
    iq = rng.integers(0, 256, size=NOUT * M * 2, dtype=np.uint8)
    iq[: 4 * M] = 0                                  # the extremes of the u8 range: two windows each
    iq[4 * M: 8 * M] = 255
    iq[8 * M: 12 * M] = 128
    iq[12 * M: 16 * M: 2] = 255
    iq[12 * M + 1: 16 * M: 2] = 0
    taps = [O.rtl_taps(131000000 + 25000 * int(k), 131000000, M)[:ntaps] for k in rng.integers(-40, 41, size=nch)]
    return iq, taps


def bar_2e7(dm, ex):
    return bool(np.all(np.abs(dm.astype(np.float64) - ex) <= 2e-7 * ex + 1e-9))


@pytest.mark.parametrize("M,ntaps", SHAPES)
def test_model_sits_inside_both_bars(M, ntaps):
    """rtl tap tables at the five (M, ntaps) of test_matrix_pipe_shared_stream_kernel: the model is within 2e-7 |ex| + 1e-9 of
    the f64-exact value of rtl.c:349-351's sum and within the project's 1e-5 |dm| + 1e-6 of the oracle's down-converter."""
    iq, taps = inputs(M, ntaps)
    dm = MM.model_dm_many(iq, M, taps, NOUT)
    assert dm.dtype == np.float32 and dm.shape == (len(taps), NOUT)
    worst = 0.0
    for c, tp in enumerate(taps):
        assert np.array_equal(dm[c], MM.model_dm(iq, M, tp, NOUT))                  # (one table at a time: the same bits)
        ex = MM.exact_dm(iq, M, tp, NOUT)
        err = np.abs(dm[c].astype(np.float64) - ex)
        worst = max(worst, float((err / (ex + 1e-3)).max()))
        assert np.all(err <= 2e-7 * ex + 1e-9), (c, float((err / (ex + 1e-9)).max()))
        want = O.fir_u8(iq, M, tp, nout=NOUT, ntaps=ntaps)
        assert np.all(np.abs(dm[c] - want) <= 1e-5 * np.abs(want) + 1e-6), c
    print("model vs f64-exact, worst relative error at M=%d ntaps=%d: %.3e" % (M, ntaps, worst))


def test_model_edges():
    """an all-zero table gives +0.0 everywhere; a table scaled by a power of two gives the scaled outputs exactly (its own
    exponent, the same digits); taps 2^12 below the largest are cut at 2^-31 of it and the result stays inside the 2e-7 bar."""
    M = 160
    iq, taps = inputs(M, M, nch=1)
    z = MM.model_dm(iq, M, np.zeros((M, 2), np.float32), NOUT)
    assert np.array_equal(z.view(np.uint32), np.zeros(NOUT, np.uint32))
    base = MM.model_dm(iq, M, taps[0], NOUT)
    for sh in (-9, -40):
        got = MM.model_dm(iq, M, taps[0] * np.float32(2.0 ** sh), NOUT)
        assert np.array_equal(got.view(np.uint32), (base * np.float32(2.0 ** sh)).view(np.uint32)), sh
    big = taps[0].copy()
    big[17] *= np.float32(4096.0)
    k = MM.chan_consts(big, M)
    assert np.abs(k.q).max() > 2 ** 29 and np.abs(np.delete(k.q, 17, axis=0)).max() < 2 ** 19
    assert bar_2e7(MM.model_dm(iq, M, big, NOUT), MM.exact_dm(iq, M, big, NOUT))


@pytest.mark.parametrize("M,ntaps", [(160, 160), (192, 192), (200, 200)])
def test_equality_with_the_model_catches_what_the_2e7_bar_lets_through(M, ntaps):
    """Three deliberately wrong variants of the arithmetic on the same input, each compared with the model bit for bit and
    against the 2e-7 bar:
      f32 twice     the sum is scaled and rounded to f32, the channel's constant added, and the result rounded again -- changes
                    bits in several per cent of the outputs and PASSES the 2e-7 bar: the bar cannot tell one rounding from two;
      lost digit    one 32-byte k-step of one channel misses its lowest digit plane (at most 2^-23 of the largest tap per tap) --
                    changes bits in ~45 % of the outputs; on this input it also fails the bar, in a few windows;
      stale tile    tile t (32 windows) is computed from the bytes of tile t - 2 -- changes bits and fails the bar.
    Recorded (rtlMult 160 / 192 / 200, 512 windows): f32 twice 62 / 127 / 73 outputs changed, inside the bar; lost digit 225 /
    239 / 248, outside; stale tile 32, outside.  Only equality catches all three whatever the input."""
    iq, taps = inputs(M, ntaps, nch=1)
    tp = taps[0]
    k = MM.chan_consts(tp, M)
    s = MM.samples(iq, M, NOUT)
    Sre, Sim = MM.exact_sums(s, [k.q])
    Sre, Sim = Sre[0], Sim[0]
    good = MM.finish(Sre, Sim, k)
    assert np.array_equal(good, MM.model_dm(iq, M, tp, NOUT))
    ex = MM.exact_dm(iq, M, tp, NOUT)
    assert bar_2e7(good, ex)

    def twice(S, dc):
        return ((S.astype(np.float64) * k.scale).astype(np.float32).astype(np.float64) + dc).astype(np.float32)
    v_twice = MM.cabs(twice(Sre, k.dc_re), twice(Sim, k.dc_im))

    kstep = 3                                                                       # bytes 96..127 of every window: taps 48..63
    d0 = np.zeros_like(k.q)
    d0[16 * kstep: 16 * kstep + 16] = MM.digits(k.q)[0][16 * kstep: 16 * kstep + 16]
    Lre, Lim = MM.exact_sums(s, [d0], check_digits=False)
    v_digit = MM.finish(Sre - Lre[0], Sim - Lim[0], k)

    v_stale = good.copy()
    t = 5
    v_stale[32 * t: 32 * t + 32] = good[32 * (t - 2): 32 * (t - 2) + 32]

    seen = {}
    for name, v in (("f32 twice", v_twice), ("lost digit", v_digit), ("stale tile", v_stale)):
        changed = int(np.count_nonzero(v.view(np.uint32) != good.view(np.uint32)))
        seen[name] = (changed, bar_2e7(v, ex))
        print("%-10s  M=%d: %d of %d outputs change bits; passes the 2e-7 bar: %s" % (name, M, changed, NOUT, seen[name][1]))
        assert changed > 0, name
    assert seen["f32 twice"][0] > NOUT // 50 and seen["f32 twice"][1]               # the point: wrong, and inside the bar
    assert not seen["stale tile"][1] and seen["stale tile"][0] >= 16
