"""msk_lean_wide.hip -- the lean demodulator with 16 lanes per channel (4 channels per wave, four-wave workgroups), the default of
contexts up to 1024 channels -- against the 8-lane kernel and against the oracle.  The width only decides which channels share a wave's segments: the operations
of a channel, their operands and their order are the same, so everything is compared bit for bit -- the channel state records,
the text under assembly, the blocks with their stamps, the bits per channel and every bit record {soft symbol, level}
(test_gpu_lean.py's snapshot), after every call, with the bit log and without.

Shapes (the smallest that can go wrong): 1, 3, 4, 5, 9 and 17 channels -- a partial wave that replicates its last channel, one and
two workgroups, padding waves of a workgroup that idle -- in calls of 1, 2, 1, 2 callbacks chained on one context, so that segments
and the dm window (refilled every 64 samples) straddle calls; and ACG_MSK_CUS=0 (no
CU partition, one-wave workgroups), where the launcher falls back to 8 lanes and must deliver the same.

Traffic: tests/test_close_inputs.py's tracks (syncs in both polarities, so that a ~SYN turns kept records; text, CRC bytes, damaged
SYN / SOH, blocks that end at DLE, two noise channels with their false syncs, a silent and a constant channel), rows reordered so
that the first channels are one of each kind.  On the 16 tracks in their own order and the sibling's schedules (8192 + 8192 and
8192 + 4096 samples) the kernel is held to the oracle with no tolerance, the way tests/test_gpu_lean_closes.py holds 8 and 4 lanes.

Not here: a bit log too short for its call.  bit_cap = max_len / 4 + 8 records against ~max_len / 5.2 bits per call, so
`nb + SEG > bit_cap` cannot be reached through the library (tests/test_gpu_lean_parked_log.py says the same), and a capacity shrunk
for a test would be unsafe: behind that rule a segment of nbits - 1 bits is still stored without a clamp, at every width."""
import pytest

import test_close_inputs as T
from test_gpu_lean import run
from test_gpu_lean_closes import against_the_oracle
from test_gpu_msk_exact import limit

pytestmark = pytest.mark.gpu

# one of each kind first: traffic found as ~SYN, traffic found as SYN, noise, silence, then the rest (17: the first row again)
ORDER = [1, 2, 0, 7, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15, 1]
CALLS = [1024, 2048, 1024, 2048]
_eight = {}


@pytest.fixture(scope="module")
def D():
    from acarsdec_amd import decoder
    from acarsdec_amd import _capi as K
    assert K.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return decoder


def rows(nch):
    return T.tracks()[ORDER[:nch], : sum(CALLS)]


def eight_lanes(D, K, tune, nch):
    """the 8-lane kernel's snapshots of every call, with and without the bit log: made once per channel count"""
    if nch not in _eight:
        tune("ACG_MSK_LPC", "8")
        with limit():
            _eight[nch] = (run(D, K, rows(nch), CALLS, bitlog=True), run(D, K, rows(nch), CALLS, bitlog=False))
    return _eight[nch]


CASES = [(nch, lpc, None) for nch in (1, 3, 4, 5, 9, 17) for lpc in (16,)] + [(nch, lpc, 0) for nch in (5, 17) for lpc in (16,)]


@pytest.mark.parametrize("nch,lpc,cus", CASES, ids=["%dch-%dlanes%s" % (n, l, "" if c is None else "-cus0") for n, l, c in CASES])
def test_wide_lane_groups_deliver_what_eight_lanes_deliver(D, tune, nch, lpc, cus):
    from acarsdec_amd import _capi as K
    ref_log, ref = eight_lanes(D, K, tune, nch)
    tune("ACG_MSK_LPC", str(lpc))
    if cus is not None:
        tune("ACG_MSK_CUS", str(cus))
    with limit():
        got_log = run(D, K, rows(nch), CALLS, bitlog=True)
        got = run(D, K, rows(nch), CALLS, bitlog=False)
    nbits = 0
    for i, (a, b, c, d) in enumerate(zip(got_log, got, ref_log, ref)):
        for what, j in (("state records", 0), ("text under assembly", 1), ("blocks", 2)):
            assert a[j] == c[j], "call %d: %s of %d and 8 lanes per channel differ (bit log on)" % (i, what, lpc)
            assert b[j] == d[j], "call %d: %s of %d and 8 lanes per channel differ (bit log off)" % (i, what, lpc)
            assert a[j] == b[j], "call %d: %s with / without bit log differ" % (i, what)
        assert a[3] == c[3], "call %d: bits per channel differ" % i
        assert a[4] == c[4], "call %d: bit records {soft symbol, level} differ" % i
        nbits += len(a[4]) // 8
    assert nbits > 1000 * nch                                    # (about 1180 bits per channel in 6144 samples)
    if nch >= 3:
        assert sum(len(s[2]) for s in got) >= 1                  # the short call sequence does decode blocks


@pytest.mark.parametrize("sched", [T.CALLS, T.RAGGED], ids=["even", "ragged"])
@pytest.mark.parametrize("lpc", [16])
def test_wide_lane_groups_are_the_oracles(D, tune, lpc, sched):
    from acarsdec_amd import _capi as K
    tune("ACG_MSK_LPC", str(lpc))
    for bitlog in (True, False):
        against_the_oracle(D, K, sched, "lean%d" % lpc, bitlog)
