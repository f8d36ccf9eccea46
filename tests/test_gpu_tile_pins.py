"""The three tile down-converters bit for bit (csrc/fir_tile_kernel.h: fir_u8_persist_kernel, fir_u8_shared_kernel, fir_fmt_kernel):
dm of seeded inputs against tests/golden/fir_tile_pins.npz, recorded by tests/golden/make_fir_tile_pins.py before the kernels were
given one skeleton.  The other tests of these kernels compare against float64 or the oracle with a bar and would not notice
another order of additions, which the shared-stream kernel's and the host feed's bit identities rest on.  Runs on the GPU box only
(-m gpu)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_fir_tile_pins as P  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = [c["name"] for c in P.CASES]


@pytest.fixture(scope="module")
def D():
    from acarsdec_amd import decoder
    from acarsdec_amd import _capi as K
    assert K.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return decoder


@pytest.fixture(scope="module")
def K():
    from acarsdec_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def pins():
    z = np.load(P.PATH)
    return {k: z[k] for k in z.files}


def same_bits(got, want, what):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    diff = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert diff.size == 0, "%s: %d of %d outputs differ, the first at channel %d window %d: %r, recorded %r" % (
        what, len(diff), got.size, diff[0][0], diff[0][1], got[tuple(diff[0])], want[tuple(diff[0])])


def test_the_fixture_holds_every_case(pins):
    assert sorted(pins) == sorted(n + s for n in IDS for s in ("/dm", "/crc"))


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_dm_is_the_recorded_bits(D, K, pins, tune, c):
    """The inputs are regenerated: their CRCs first, so that another generator is reported as such; then every bit of dm (the
    device calls twice: the second round gives the bits of the first)."""
    x, taps, smap = P.inputs(c)
    assert np.array_equal(P.crcs(x, taps), pins[c["name"] + "/crc"]), "%s: the generated input or taps are not the recorded ones" % c["name"]
    same_bits(P.run(D, K, tune, c, x, taps, smap), pins[c["name"] + "/dm"], c["name"])


@pytest.mark.parametrize("feed", sorted(P.FEED_OF))
def test_feed_pieces_are_the_bits_of_one_device_call(pins, feed):
    """the ragged launches of the host feed against the first windows of the whole callback on the same input"""
    n = sum(P.PIECES)
    same_bits(pins[feed + "/dm"], np.ascontiguousarray(pins[P.FEED_OF[feed] + "/dm"][:, :n]), feed)


@pytest.mark.parametrize("name", ["shared-u8-M200", "shared-u8-M160", "shared-s8-M200", "shared-s8-M160"])
def test_shared_stream_pins_are_the_one_channel_kernels_bits(D, K, pins, tune, name):
    """the same input and stream map with one (channel, tile) per unit (ACG_FIR_SHARED=0, ACG_FIR_VARIANT=3): the recorded bits of
    the shared-stream kernel"""
    c = next(c for c in P.CASES if c["name"] == name)
    x, taps, smap = P.inputs(c)
    same_bits(P.run(D, K, tune, c, x, taps, smap, tunes=dict(P.PLAIN)), pins[name + "/dm"], name)
