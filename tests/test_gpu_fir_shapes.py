"""The u8 wave-private down-converter (csrc/fir.hip, fir_u8_direct_kernel) in every launch shape its launcher can give it --
the shapes tests/test_gpu_formats.py takes the format kernels through -- and in the launch with fewer runs than waves.  Runs on
the GPU box only (-m gpu).

Tolerance: the project's written one for dm against the oracle, 1e-5 |x| + 1e-6; between launch shapes of the same kernel: none
(run length, workgroup shape and who took which run change no sum).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES3 = [3, 2, 2]                  # 7 channels on 3 streams
SWITCHES = ("ACG_FIR_WAVES_PER_WG", "ACG_FIR_WG_PER_CU", "ACG_FIR_RUN_PAIRS", "ACG_FIR_VARIANT")
# launch shapes of one context, in the order they run: (name, WAVES_PER_WG, WG_PER_CU, RUN_PAIRS, VARIANT)
SHAPES = [("default", None, None, None, None),
          ("1wave-pairs1", 1, 1, 1, None),
          ("1wave-pairs2", 1, 1, 2, None),
          ("1wave-pairs8", 1, 1, 8, None),
          ("2waves", 2, 1, None, None),
          ("fallback", None, None, None, 3)]


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


def within_bar(got, want):
    return np.abs(got - want) <= 1e-5 * np.abs(want) + 1e-6


def make_taps(O, M, ntaps, nch, rng):
    win = np.hamming(ntaps) / np.hamming(ntaps).mean() * (M / ntaps)
    return np.stack([(O.rtl_taps(131000000 + 25000 * int(rng.integers(-40, 41)), 131000000, M)[:ntaps] * win[:, None]).astype(np.float32)
                     for c in range(nch)])


def make_input(rng, nrows, nwin, M):
    """random bytes with the extremes of the u8 range in runs: whole windows of 0 and of 255, a run of each that starts and ends
    inside a window, and the two alternating"""
    iq = rng.integers(0, 256, size=(nrows, nwin * M * 2), dtype=np.uint8)
    w = 2 * M
    for r in range(nrows):
        a = int(rng.integers(0, nwin - 40))
        iq[r, a * w: (a + 3) * w] = 0
        iq[r, (a + 5) * w: (a + 8) * w] = 255
        iq[r, (a + 10) * w + 7: (a + 11) * w + 33] = 255
        iq[r, (a + 13) * w + 5: (a + 14) * w + 91] = 0
        iq[r, (a + 20) * w: (a + 22) * w: 2] = 0
        iq[r, (a + 20) * w + 1: (a + 22) * w: 2] = 255
    return iq


def set_shape(tune, shape):
    for name, v in zip(SWITCHES, shape[1:]):
        tune(name, None if v is None else str(v))


@pytest.mark.parametrize("M", [160, 192, 200])
def test_u8_direct_kernel_launch_shapes_are_bit_identical(D, O, M, tune):
    """fir_u8_direct_kernel<20 / 24 / 25>: 7 channels on 3 streams with a scrambled map (the row lookup; the shared-stream
    kernels switched off), 2 callbacks = 16 two-tile bodies per channel, so runs of 1, 2 and 8 bodies all divide; fewer taps
    than the window (zero tap columns); runs of 0 and 255 in the input.  Launch shapes: default; one-wave workgroups, one per
    CU, with runs of 1, 2 and 8 bodies; two-wave workgroups.  dm within the bar of the oracle in every shape and bit-identical
    across them; the workgroup-granular kernel (ACG_FIR_VARIANT=3) adds in another order: within the bar, and not the same
    bits -- so the others ran the wave-private kernel."""
    import torch
    rng = np.random.default_rng(9000 + M)
    nch, nblk, ntaps = sum(SIZES3), 2, M - 40
    nwin = nblk * 1024
    assert (nwin // 64 // 2) % 8 == 0
    smap = np.repeat(np.arange(len(SIZES3)), SIZES3)
    rng.shuffle(smap)
    smap = smap.astype(np.int32)
    taps = make_taps(O, M, ntaps, nch, rng)
    iq = make_input(rng, len(SIZES3), nwin, M)
    want = np.stack([O.fir_u8(iq[smap[c]], M, taps[c], nout=nwin, ntaps=ntaps) for c in range(nch)])
    dev = torch.from_numpy(iq).cuda()
    tune("ACG_FIR_SHARED", "0")                         # (read when the stream map is set) one row lookup per channel, no groups
    dec = D.Decoder(nch, decim=M, ntaps=ntaps, nstreams=len(SIZES3), max_blocks=nblk, bitlog=False)
    dec.set_taps(taps)
    dec.set_channel_streams(smap)
    out = {}
    for shape in SHAPES:                                # the switches are read at every launch
        set_shape(tune, shape)
        dec.fir_only(dev, nblk, dev.stride(0))
        out[shape[0]] = got = np.stack([dec.dm(c, nwin) for c in range(nch)])
        err = np.abs(got - want) / (1e-5 * np.abs(want) + 1e-6)
        print("LEDGER u8 M=%d %s: worst err/bar %.3f" % (M, shape[0], err.max()))
        assert within_bar(got, want).all(), (shape[0], float(err.max()), np.unravel_index(int(err.argmax()), err.shape))
    dec.close()
    for name in [s[0] for s in SHAPES[1:-1]]:
        assert np.array_equal(out[name], out["default"]), (name, int((out[name] != out["default"]).sum()))
    assert not np.array_equal(out["fallback"], out["default"])


def test_u8_direct_kernel_one_run_for_four_waves_three_launches(D, O, tune):
    """One channel, one callback, four-wave workgroups and ACG_FIR_RUN_PAIRS=8: 8 bodies = ONE run for four waves.  Three waves
    find no run of their own, probe every shard, find nothing and sign off; the last wave out re-arms the dispenser, and that is
    what the next launch starts from: three launches in a row on one context, each on its own input (a stale dm cannot pass),
    each within the bar of the oracle."""
    import torch
    M, ntaps, nwin = 200, 160, 1024
    rng = np.random.default_rng(77)
    taps = make_taps(O, M, ntaps, 1, rng)
    tune("ACG_FIR_WAVES_PER_WG", "4")
    tune("ACG_FIR_RUN_PAIRS", "8")
    dec = D.Decoder(1, decim=M, ntaps=ntaps, nstreams=1, max_blocks=1, bitlog=False)
    dec.set_taps(taps)
    wants = []
    for k in range(3):
        iq = make_input(rng, 1, nwin, M)
        want = O.fir_u8(iq[0], M, taps[0], nout=nwin, ntaps=ntaps)
        dev = torch.from_numpy(iq).cuda()
        dec.fir_only(dev, 1, dev.stride(0))
        got = dec.dm(0, nwin)
        assert within_bar(got, want).all(), (k, float((np.abs(got - want) / (1e-5 * np.abs(want) + 1e-6)).max()))
        wants.append(want)
    dec.close()
    # the three inputs ask for three different answers: nine windows in ten differ by more than the bar
    for j in range(3):
        for k in range(j):
            assert within_bar(wants[j], wants[k]).mean() < 0.1, (j, k)
