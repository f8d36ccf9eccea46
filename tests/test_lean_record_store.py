"""Where msk_lean.hip's bit records leave the kernel, pinned in the product's assembly (CPU only).

With a bit log every period of a segment used to end in a `global_store_dwordx2` of all 64 lanes (the eight lanes of a channel's
group storing the identical record): one wave per SIMD runs this loop, so the issue of that store -- 64 addresses and 64 records
read from the register file -- is paid in full on the chain that sets the bit rate (the log cost 3.2 % of the kernel, alone on the
chip as beside the down-converter: profiles/LEDGER.md).  Now lane g of a group KEEPS records g, g + LPC, ... (two selects a period)
and one store per lane behind the segment's framing writes them.  Read off `msk_lean_kernel<8,4,true>` (the bench's kernel) and
`<8,1,true>`, compiled with the product's flags:

 (a) between the loop's refill -- its pair of `global_load_dwordx4` -- and the last period's shift-register pair lies no
     `global_store_*` at all: the eight periods are free of vector-memory stores;
 (b) with -DACG_LEAN_AB_REC0, the order before (kept for same-tree A/B builds, profiles/probe/build_ab.py), the same stretch
     holds at least seven, i.e. (a) can fail;
 (c) none of the eight instantiations uses scratch, and none needs more registers than the order before."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compile_lean(extra):
    """{(lpc, wpg, log): (instructions, next_free_vgpr, scratch bytes)} of msk_lean.hip under the product's flags + extra"""
    from acarsdec_amd import _build as B
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "acarsdec_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include")] +
                       B.MSK_LEAN_FLAGS + extra + ["-S", "-o", "-", os.path.join(csrc, "msk_lean.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur, body = {}, None, None
    for line in r.stdout.splitlines():
        m = re.match(r"^_Z15msk_lean_kernelILi(\d+)ELi(\d+)ELb([01])EEv7MskArgs:", line)
        s = line.strip()
        if m:
            cur = (int(m.group(1)), int(m.group(2)), m.group(3) == "1")
            body = []
            out[cur] = [body, None, None]
        elif cur and s.startswith(".amdhsa_next_free_vgpr"):
            out[cur][1] = int(s.split()[1])
        elif cur and s.startswith(".amdhsa_private_segment_fixed_size"):
            out[cur][2] = int(s.split()[1])
        elif s.startswith(".end_amdhsa_kernel"):
            cur = None
        elif cur and body is not None and s and not s.startswith((";", ".")) and not re.match(r"^\.?\w+:", s):
            body.append(line.split(";")[0].strip())
    assert len(out) == 8 and all(v[1] is not None and v[2] is not None for v in out.values()), sorted(out)
    return out


@pytest.fixture(scope="module")
def product():
    return compile_lean([])


@pytest.fixture(scope="module")
def before():
    return compile_lean(["-DACG_LEAN_AB_REC0"])


def stores_in_the_periods(body):
    """the global_store_* between the loop's refill loads and the last period's shift-register pair"""
    marks = [i for i, l in enumerate(body) if l.startswith("v_addc_co_u32_e64")]
    assert len(marks) == 16, len(marks)
    loads = [i for i, l in enumerate(body[:marks[0]]) if l.startswith("global_load_dwordx4")]
    assert len(loads) >= 2 and loads[-1] - loads[-2] == 1, "the refill's pair of loads in front of the first period"
    assert marks[0] - loads[-1] <= 300, ("the first period follows the refill", marks[0] - loads[-1])
    return [l for l in body[loads[-1] + 1:marks[-1] + 1] if l.startswith("global_store_")]


@pytest.mark.parametrize("wpg", [4, 1])
def test_the_periods_hold_no_vector_memory_store(product, wpg):
    got = stores_in_the_periods(product[(8, wpg, True)][0])
    assert got == [], got


@pytest.mark.parametrize("wpg", [4, 1])
def test_the_order_before_held_a_store_in_every_period(before, wpg):
    got = stores_in_the_periods(before[(8, wpg, True)][0])
    assert len(got) >= 7 and all(l.startswith("global_store_dwordx2") for l in got), got


def test_no_scratch_and_no_more_registers_than_before(product, before):
    for key in sorted(product):
        body, vgpr, scratch = product[key]
        assert scratch == 0 and not any(l.startswith("scratch_") for l in body), key
        assert vgpr <= before[key][1], (key, vgpr, before[key][1])
