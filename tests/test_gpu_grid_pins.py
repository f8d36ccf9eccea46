"""The two grid down-converters bit for bit (csrc/fir_rate.hip, csrc/fir_long.hip, their shared skeleton csrc/fir_grid_kernel.h):
dm of seeded inputs against tests/golden/fir_grid_pins.npz, recorded by tests/golden/make_fir_grid_pins.py before the kernels were
given one skeleton.  The other tests of these kernels compare against float64 with a derived bar and would not notice another
order of additions, which the contract of fir_long.hip and the derivation of long_ref.bar rest on.  Runs on the GPU box only
(-m gpu)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_fir_grid_pins as P  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def D():
    from acarsdec_amd import decoder
    from acarsdec_amd import _capi as K
    assert K.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return decoder


@pytest.fixture(scope="module")
def pins():
    z = np.load(P.PATH)
    return {k: z[k] for k in z.files}


def test_the_fixture_holds_every_case(pins):
    assert sorted(pins) == sorted(n + s for n, _ in P.CASES for s in ("/dm", "/crc"))


@pytest.mark.parametrize("name,case", P.CASES, ids=[n for n, _ in P.CASES])
def test_dm_is_the_recorded_bits(D, pins, name, case):
    """The inputs are regenerated: their CRCs first, so that another generator is reported as such; then every bit of dm."""
    rate, box, filt, rows = P.inputs(name, case, D)
    assert np.array_equal(P.crcs(box, filt, rows), pins[name + "/crc"]), "%s: the generated input or taps are not the recorded ones" % name
    got = P.run(D, case[0], rate, box, filt, rows)
    want = pins[name + "/dm"]
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (P.streams(case[0]), sum(P.CALLS))
    diff = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert diff.size == 0, "%s: %d of %d outputs differ, the first at channel %d window %d: %r, recorded %r" % (
        name, len(diff), got.size, diff[0][0], diff[0][1], got[tuple(diff[0])], want[tuple(diff[0])])
