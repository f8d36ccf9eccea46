"""msk_lean_wide.hip -- msk_lean_kernel with 16 lanes per channel -- in the product's assembly (CPU only).

A period's instruction stream does not depend on the group width: above 6 lanes every lane mixes at most one sample, and the
lanes without one mix into the ring's spare row.  So the periods of the wide kernels are held to the figures pinned for the 8-lane
kernel (tests/test_lean_slots.py: waits, no-operations, register copies and length of periods 2-8, period by period), compiled
the way that test compiles msk_lean.hip; the dm window's refill lies outside the periods, and this test holds it there.  No kernel of the unit
uses scratch, and each holds exactly the sixteen shift-register updates (v_addc_co_u32) of the eight periods of a segment."""
import os
import re
import shutil
import subprocess

import pytest

from test_lean_issue_order import periods
from test_lean_slots import COPIES, LENGTH, NOPS, WAITS, figures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = {"waits": WAITS, "nops": NOPS, "copies": COPIES, "length": LENGTH}


@pytest.fixture(scope="module")
def unit():
    """({(lpc, wpg, log): [instruction]}, the whole assembly text) of msk_lean_wide.hip under the product's flags"""
    from acarsdec_amd import _build as B
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "acarsdec_amd", "csrc")
    flags = [f for n, f, _ in B.UNITS if n == "msk_lean_wide.hip"][0]
    assert set(B.MSK_LEAN_FLAGS) <= set(flags) and set(flags) - set(B.MSK_LEAN_FLAGS) <= {"--offload-compress"}, flags
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include")] +
                       B.MSK_LEAN_FLAGS + ["-S", "-o", "-", os.path.join(csrc, "msk_lean_wide.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for line in r.stdout.splitlines():
        m = re.match(r"^_Z15msk_lean_kernelILi(\d+)ELi(\d+)ELb([01])EEv7MskArgs:", line)
        if m:
            cur = (int(m.group(1)), int(m.group(2)), m.group(3) == "1")
            out[cur] = []
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur and not line.lstrip().startswith(";") and line.strip() and not re.match(r"^\.?\w+:", line.strip()):
            out[cur].append(line.split(";")[0].strip())
    return out, r.stdout


def test_the_unit_holds_the_wide_kernels_of_four_wave_workgroups_only(unit):
    kernels, _ = unit
    assert kernels and all(lpc == 16 and wpg == 4 for lpc, wpg, _ in kernels), sorted(kernels)
    for lpc in {k[0] for k in kernels}:
        assert (lpc, 4, True) in kernels, (lpc, "a width is launched with a bit log or not at all")


def test_no_kernel_uses_scratch(unit):
    kernels, text = unit
    for key, body in kernels.items():
        assert not any("scratch_" in l for l in body), key
    sizes = re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", text)
    assert len(sizes) == len(kernels) and all(int(s) == 0 for s in sizes), sizes


def test_a_segment_is_eight_periods_with_two_shift_register_updates_each(unit):
    kernels, _ = unit
    for key, body in kernels.items():
        assert sum(l.startswith("v_addc_co_u32_e64") for l in body) == 16, key


def test_a_period_is_within_the_bounds_pinned_for_eight_lanes(unit):
    kernels, _ = unit
    logged = [k for k in sorted(kernels) if k[2]]
    assert logged
    for key in logged:
        fig = figures(kernels[key])
        for what, most in BOUND.items():
            over = [k + 2 for k, (got, m) in enumerate(zip(fig[what], most)) if got > m]
            assert not over, ("<%d,%d,true>" % key[:2], what, "periods over the bound", over, fig[what], most)


def test_the_refill_of_the_dm_window_stays_outside_the_periods(unit):
    """a period loads nothing from memory, and the one exec-mask save it holds is the guarded commit block of front(), as with
    8 lanes: the refill's loads belong to the segment's head"""
    kernels, _ = unit
    for key, body in kernels.items():
        for k, w in enumerate(periods(body)[1:]):
            assert not any(l.startswith(("global_load", "buffer_load", "flat_load")) for l in w), (key, k + 2)
            assert sum(l.startswith(("s_and_saveexec", "s_or_saveexec")) for l in w) <= 1, (key, k + 2)
