"""The conditions on the inputs of tests/test_gpu_uptime.py, checked with the oracle alone: the traffic has blocks under way where
the counters cross 2^31 / 2^32, for every base that test presets; and the oracle itself, preset, restates a run from 0 shifted.
These are conditions, not measurements: an input that misses one gets another seed, never a smaller number."""
import numpy as np
import pytest

import uptime_traffic as U

NEED = 12                                    # channels, of 24


@pytest.fixture(scope="module")
def base():
    """the oracle's run from 0, even cuts: per channel the (end_bit, end_sample, soh_sample) of its blocks"""
    calls = U.oracle_run(U.EVEN_CUTS)
    out = {c: [] for c in range(U.NCH)}
    for frames, _, _ in calls:
        for c, lst in frames.items():
            out[c] += [k[6:9] for k in lst]
    return out


def test_traffic_shape_and_density(base):
    x = U.traffic()
    assert x.shape == (24, 6 * 8192) and x.dtype == np.float32
    assert U.traffic() is x and not x.flags.writeable            # shared, unchanged
    assert all(len(v) >= 2 for v in base.values())
    for c, v in base.items():
        assert all(0 <= ss < es < U.NSAMP for _, es, ss in v) and v == sorted(v)


@pytest.mark.parametrize("sample_base,pow2", [b for b in U.SAMPLE_BASES if b[1]])
def test_blocks_straddle_every_sample_boundary(base, sample_base, pow2):
    """at least 12 channels have a block whose SOH lies below the power of two and whose closing bit lies at or above it"""
    at = pow2 - sample_base
    assert 0 < at < U.NSAMP
    n = sum(any(ss < at <= es for _, es, ss in v) for v in base.values())
    print("boundary %d samples in: %d channels" % (at, n))
    assert n >= NEED, (at, n)


@pytest.mark.parametrize("at", [pow2 - b for b in U.SINK_BASES for pow2 in (1 << 31, 1 << 32) if 0 < pow2 - b < U.NSAMP])
def test_blocks_straddle_the_sink_bases_boundaries(base, at):
    """the same for the places where the sinks' bases (multiples of 12500) put the boundary"""
    assert at in (8648, 4796, 29796)
    n = sum(any(ss < at <= es for _, es, ss in v) for v in base.values())
    assert n >= NEED, (at, n)


@pytest.mark.parametrize("bit_base,pow2", [b for b in U.BIT_BASES if b[1]])
def test_blocks_on_both_sides_of_every_bit_boundary(base, bit_base, pow2):
    at = pow2 - bit_base
    assert at >= 2000
    n = sum(any(eb < at for eb, _, _ in v) and any(eb >= at for eb, _, _ in v) for v in base.values())
    print("boundary %d bits in: %d channels" % (at, n))
    assert n >= NEED, (at, n)


def test_every_cut_set_covers_the_traffic():
    for cuts in (U.EVEN_CUTS, U.RAGGED_CUTS):
        assert cuts[0] == 0 and cuts[-1] == U.NSAMP and cuts == sorted(set(cuts))
    assert all((b - a) % 32 == 0 for a, b in zip(U.EVEN_CUTS[:-1], U.EVEN_CUTS[1:]))
    assert sum((b - a) % 32 != 0 for a, b in zip(U.RAGGED_CUTS[:-1], U.RAGGED_CUTS[1:])) >= 5
    # the call boundary the bases 2^32 - 16384 +- 1 are placed around
    assert 16384 in U.EVEN_CUTS and ((1 << 32) - 16384, 1 << 32) in U.SAMPLE_BASES


@pytest.mark.parametrize("cuts", [U.EVEN_CUTS, U.RAGGED_CUTS], ids=["even", "ragged"])
@pytest.mark.parametrize("sb,bb", [((1 << 32) - 5000, (1 << 32) - 900), ((1 << 40) + 12345, 1 << 36), ((1 << 31) - 8648, (1 << 31) - 2000)])
def test_preset_oracle_is_the_run_from_zero_shifted(cuts, sb, bb):
    """Channel.preset: the blocks, the framing states and the distances back to the SOH of a run from 0, call by call, with
    end_bit shifted by the bit base and end_sample / soh_sample by the sample base: the oracle's counters are 64-bit throughout"""
    zero, shifted = U.oracle_run(cuts), U.oracle_run(cuts, sb, bb)
    assert len(zero) == len(shifted) == len(cuts) - 1
    total = 0
    for (f0, s0, d0), (f1, s1, d1) in zip(zero, shifted):
        assert s0 == s1 and d0 == d1 and f0.keys() == f1.keys()
        for c in f0:
            assert [k[:6] + (k[6] + bb, k[7] + sb, k[8] + sb) for k in f0[c]] == f1[c], c
            total += len(f0[c])
        assert all(0 < d < 65536 for d in d0.values())
    assert total >= 3 * U.NCH
    assert sum(len(d) for _, _, d in zero) >= 3 * U.NCH          # channels caught inside a block at the end of a call
