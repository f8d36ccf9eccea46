"""The byte closes that end a segment of msk_lean.hip -- SYN2 with SYN, ~SYN or neither, a SOH1 that is no SOH, the byte behind a
block -- at every exit of the unrolled segment loop (tests/test_close_inputs.py builds the tracks and proves on the CPU that they
get there): in the lean kernel's closing period frame_bit<true>() (msk_common.h) applies them by selects, in msk.hip's kernel
decode_acars() does, after every bit.  After EVERY call, on every channel: the lean kernel (8 lanes per channel in both
workgroup shapes, 4 lanes) and the inline kernel (ACG_MSK_NOLEAN=1) leave the same state record, text under assembly, blocks with their stamps and bit records, byte
for byte (test_gpu_lean.py's snapshot), and each is the oracle's with no tolerance (test_gpu_msk_exact.py's comparison: the loop's
doubles as bit patterns, framing state, soh_back, text, blocks, bit records).  One ragged schedule, 8192 + 4096 samples, puts a
close next to a call boundary."""
import pytest

import test_close_inputs as T
from test_gpu_lean import run
from test_gpu_msk_exact import differences, limit

pytestmark = pytest.mark.gpu

SHAPES = [("lean8", 8, None), ("lean8-cus0", 8, 0), ("lean4", 4, None)]


@pytest.fixture(scope="module")
def D():
    from acarsdec_amd import decoder
    from acarsdec_amd import _capi as K
    assert K.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return decoder


def against_the_oracle(D, K, sched, name, bitlog):
    """one decoder over the tracks in calls of `sched`, held to the oracle after every call"""
    x = T.tracks()
    want = T.oracle_run(sched)
    with limit():
        dec = D.Decoder(T.NCH, max_blocks=8, bitlog=bitlog)
    a0 = 0
    for i, n in enumerate(sched):
        with limit():
            dec.demod_msk(x[:, a0:a0 + n])
            dec.sync()
            diff = differences(dec, K, want[i], bitlog, True)
        if diff:
            _, ch, field, got, ref = diff[0]
            raise AssertionError("%s kernel, bit log %d, calls %s, call %d, channel %d: %s is %s, the oracle has %s  [%d differences in this call]"
                                 % (name, bitlog, sched, i, ch, field, got, ref, len(diff)))
        a0 += n
    dec.close()


@pytest.mark.parametrize("sched", [T.CALLS, T.RAGGED], ids=["even", "ragged"])
@pytest.mark.parametrize("name,lpc,cus", SHAPES, ids=[s[0] for s in SHAPES])
def test_closes_that_end_a_segment_are_the_inline_kernels_and_the_oracles(D, tune, name, lpc, cus, sched):
    from acarsdec_amd import _capi as K
    tune("ACG_MSK_LPC", str(lpc))
    if cus is not None:
        tune("ACG_MSK_CUS", str(cus))
    x = T.tracks()[:, : sum(sched)]
    with limit():
        lean = run(D, K, x, sched, bitlog=False)
        lean_log = run(D, K, x, sched, bitlog=True)
    for bitlog in (True, False):
        against_the_oracle(D, K, sched, name, bitlog)
    tune("ACG_MSK_NOLEAN", "1")
    with limit():
        inline = run(D, K, x, sched, bitlog=False)
        inline_log = run(D, K, x, sched, bitlog=True)
    for bitlog in (True, False):
        against_the_oracle(D, K, sched, "inline (%d lanes)" % lpc, bitlog)
    nblocks = 0
    for i, (a, b, c, d) in enumerate(zip(lean, lean_log, inline, inline_log)):
        for what, j in (("state records", 0), ("text under assembly", 1), ("blocks", 2)):
            assert a[j] == c[j], "call %d: %s of the lean and the inline kernel differ" % (i, what)
            assert a[j] == b[j] and c[j] == d[j], "call %d: %s with / without bit log differ" % (i, what)
        assert b[3] == d[3], "call %d: bits per channel differ" % i
        assert b[4] == d[4], "call %d: bit records {soft symbol, level} differ" % i
        nblocks += len(a[2])
    assert nblocks > 40
