"""The issue slots of a bit period of msk_lean.hip that carry no arithmetic, pinned in the product's assembly (CPU only).

One wave per SIMD runs the period, and what paces it is the number of slots it issues: a wait, a no-operation or a register copy
takes one like an fma does (profiles/LEDGER.md round 10: two `s_nop 0` more cost 0.24 % of the kernel).  Round 10 took eight of
them out of a period -- the three counted waits in front of the five old taps became one, the two `s_nop 0` in front of the phase
picks of steps 5 and 6 are filled by the fifth clock step, the three copies of a series constant into an fma's accumulator are
gone -- and this test keeps them out.  Read off `msk_lean_kernel<8,4,true>` (the bench's kernel) and `<8,1,true>`, compiled with
the product's flags, in periods 2-8 of the unrolled segment (period k + 1 lies between the shift-register pairs of periods k and
k + 1; period 1 has no pair in front of it):

 (a) a period holds at most as many `s_waitcnt`, `s_nop` and `v_mov_b32` + `v_mov_b64` as it does in the tree that made the change,
     and is at most as long: the lists below, period by period;
 (b) each of those figures is below the parent's (7 waits, 2 no-operations, 8 copies, 262 instructions), asserted on the lists;
 (c) with the switch that takes a step back (kept for same-tree A/B builds, profiles/probe/build_ab.py) its figure is over the
     bound again, i.e. (a) can fail: ACG_LEAN_AB_WAIT0 the waits and the length, ACG_LEAN_AB_NOP0 the no-operations,
     ACG_LEAN_AB_HORN0 the copies.

The order of a period, its chains' layout, where the bit records leave, registers and scratch are pinned by
test_lean_issue_order.py, test_lean_chain_layout.py and test_lean_record_store.py."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from test_lean_issue_order import periods

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = [(8, 4, True), (8, 1, True)]
# periods 2..8 of the tree that made the change
WAITS = [6, 5, 5, 5, 6, 5, 5]
NOPS = [0, 0, 0, 0, 0, 0, 0]
COPIES = [3, 2, 2, 2, 2, 2, 4]
LENGTH = [256, 255, 254, 254, 254, 254, 258]
PARENT = {"waits": 7, "nops": 2, "copies": 8, "length": 262}
BACK = ["-DACG_LEAN_AB_WAIT0", "-DACG_LEAN_AB_NOP0", "-DACG_LEAN_AB_HORN0"]


def compile_lean(extra):
    """{(lpc, wpg, log): [instruction]} of msk_lean.hip under the product's flags + extra"""
    from acarsdec_amd import _build as B
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    csrc = os.path.join(ROOT, "acarsdec_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include")] +
                       B.MSK_LEAN_FLAGS + extra + ["-S", "-o", "-", os.path.join(csrc, "msk_lean.hip")], capture_output=True, text=True, timeout=900)
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
    assert len(out) == 8, sorted(out)
    return out


@pytest.fixture(scope="module")
def builds():
    """the product's assembly and the three with one step taken back, compiled side by side"""
    if not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    with ThreadPoolExecutor(max_workers=4) as ex:
        got = list(ex.map(compile_lean, [[]] + [[f] for f in BACK]))
    return dict(zip(["product"] + BACK, got))


def figures(body):
    """per period 2..8: waits, no-operations, register copies, length"""
    per = periods(body)[1:]
    count = lambda w, *names: sum(l.split(" ")[0].rsplit("_e32", 1)[0].rsplit("_e64", 1)[0] in names for l in w)
    return {"waits": [count(w, "s_waitcnt") for w in per], "nops": [count(w, "s_nop") for w in per],
            "copies": [count(w, "v_mov_b32", "v_mov_b64") for w in per], "length": [len(w) for w in per]}


BOUND = {"waits": WAITS, "nops": NOPS, "copies": COPIES, "length": LENGTH}


def over(fig, what):
    return [k + 2 for k, (got, most) in enumerate(zip(fig[what], BOUND[what])) if got > most]


def test_the_bounds_are_below_the_parents_figures():
    for what, most in BOUND.items():
        assert len(most) == 7 and max(most) < PARENT[what], (what, most, PARENT[what])


@pytest.mark.parametrize("key", KERNELS)
def test_a_period_keeps_its_idle_slots_out(builds, key):
    fig = figures(builds["product"][key])
    for what in BOUND:
        assert not over(fig, what), ("<%d,%d,true>" % key[:2], what, "periods over the bound", over(fig, what), fig[what], BOUND[what])


@pytest.mark.parametrize("key", KERNELS)
@pytest.mark.parametrize("switch,what", [("-DACG_LEAN_AB_WAIT0", "waits"), ("-DACG_LEAN_AB_WAIT0", "length"),
                                         ("-DACG_LEAN_AB_NOP0", "nops"), ("-DACG_LEAN_AB_HORN0", "copies")])
def test_a_step_taken_back_is_over_its_bound(builds, key, switch, what):
    fig = figures(builds[switch][key])
    assert len(over(fig, what)) == 7, (switch, "<%d,%d,true>" % key[:2], what, fig[what], BOUND[what])
