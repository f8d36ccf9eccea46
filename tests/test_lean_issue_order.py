"""The issue order of a bit period of msk_lean.hip, pinned against compiler drift (CPU only: the product's own assembly).

One wave per SIMD runs the demodulator, so nothing hides an LDS round trip that the period's own instruction stream does not
cover.  The kernel therefore issues (csrc/msk_lean.hip, front()):

    tap phase -> h[] taps and old ring entries (reads) -> the mixer's sin/cos -> ring write -> newest-tap reads
    -> the five old taps' arithmetic -> wave-wide test -> bit decision

and this test reads that order off the assembly of `msk_lean_kernel<8,4,true>` (the bench's kernel) and `<8,1,true>`, compiled
with the product's flags, for each of the eight periods of a segment:

 (a) behind the ring's ds_write2_b64 come the three newest-tap ds_read2_b64 with no LDS wait in between, and at least 10
     vector instructions -- the five old taps, a v_pk_mul_f32 and a v_pk_add_f32 each, are among them -- lie between the ring
     write and the first wait that retires one of those three reads;
 (b) no wait between the last h[] read and the ring write retires an h[] read, and at least 20 vector instructions (the
     sin/cos: 23, msk_common.h) lie between the last h[] read and the first wait that does (the 20 is this test's own
     figure: most of the sin/cos, whose latency cover is the point);
 (c) the period holds no unconditional s_branch: "every lane fired, the segment goes on" falls through.

How (a) and (b) are worded: a wait `s_waitcnt lgkmcnt(N)` retires everything but the youngest N LDS operations, so whether it
waits for a given read follows from N and the operations issued since.  The plainer wording "no s_waitcnt lgkmcnt at all" in
those two spans cannot hold for both at once (the old taps' arithmetic needs the h[] reads, so a wait for them lies either in
front of the ring write or inside the span of (a)), and the mixer's own table entry needs a wait in front of the ring write:
what is pinned is that those waits are COUNTED ones that leave the reads in question in flight."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kernels():
    from acarsdec_amd import _build as B
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "acarsdec_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include")] +
                       B.MSK_LEAN_FLAGS + ["-S", "-o", "-", os.path.join(csrc, "msk_lean.hip")], capture_output=True, text=True, timeout=900)
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


def periods(body):
    """the instruction windows of the eight periods of a segment: period k + 1 lies between the shift-register pair
    (v_addc_co_u32) of period k and that of period k + 1; period 0 in a window of the same length in front of the first pair"""
    marks = [i for i, l in enumerate(body) if l.startswith("v_addc_co_u32_e64")]
    assert len(marks) == 16, len(marks)
    gaps = [marks[i + 2] - marks[i] for i in range(0, 14, 2)]
    assert max(gaps) <= 300, ("the eight periods are laid out one behind the other", gaps)
    return [body[marks[0] - min(gaps):marks[0]]] + [body[marks[i]:marks[i + 2]] for i in range(0, 14, 2)]


def lgkm_wait(ins):
    """N of `s_waitcnt ... lgkmcnt(N)`, None for any other instruction"""
    if not ins.startswith("s_waitcnt"):
        return None
    m = re.search(r"lgkmcnt\((\d+)\)", ins)
    return int(m.group(1)) if m else None


def first_wait_retiring(w, first, start):
    """index of the first wait at or behind `start` that retires the LDS operation at index `first` or a younger one"""
    for i in range(start, len(w)):
        n = lgkm_wait(w[i])
        if n is not None and n < sum(1 for l in w[first:i] if l.startswith("ds_")):
            return i
    raise AssertionError("no wait retires the reads issued at %d" % first)


@pytest.mark.parametrize("wpg", [4, 1])
def test_a_period_covers_its_lds_round_trips(kernels, wpg):
    body = kernels[(8, wpg, True)]
    for k, w in enumerate(periods(body)):
        where = "<8,%d,true> period %d" % (wpg, k)
        # what counts on lgkmcnt in a period is LDS only: no scalar loads, no messages
        assert not any(l.startswith(("s_load", "s_buffer_load", "s_sendmsg")) for l in w), where
        writes = [i for i, l in enumerate(w) if l.startswith("ds_write2_b64")]
        assert len(writes) == 1, (where, writes)
        iw = writes[0]
        # ---- (a)
        ds_behind = [i for i in range(iw + 1, len(w)) if w[i].startswith("ds_")][:3]
        assert len(ds_behind) == 3 and all(w[i].startswith("ds_read2_b64") for i in ds_behind), (where, [w[i] for i in ds_behind])
        assert not any(lgkm_wait(l) is not None for l in w[iw:ds_behind[2]]), where
        ia = first_wait_retiring(w, ds_behind[0], ds_behind[2] + 1)
        valu = [l for l in w[iw:ia] if l.startswith("v_")]
        assert len(valu) >= 10, (where, len(valu))
        assert sum(l.startswith("v_pk_mul_f32") for l in valu) >= 5 and sum(l.startswith("v_pk_add_f32") for l in valu) >= 5, (where, valu)
        # ---- (b): the h[] taps are the only 32-bit LDS reads in front of the ring write (ds_read2_b32 x 5 and one ds_read_b32
        # right behind them; the ring is read in 64-bit entries, the sin/cos table in 128-bit ones)
        h2 = [i for i in range(iw) if w[i].startswith("ds_read2_b32")]
        assert len(h2) == 5, (where, h2)
        first_h = h2[0]
        last_h = max(i for i in range(first_h, iw) if re.match(r"ds_read2?_b32\b", w[i]))
        ib = first_wait_retiring(w, first_h, last_h + 1)
        assert ib > iw, (where, "a wait in front of the ring write retires an h[] read", w[ib])
        assert sum(l.startswith("v_") for l in w[last_h:ib]) >= 20, where
        # ---- (c)
        assert not any(l.startswith("s_branch") for l in w), where
