"""Where msk_lean.hip lays out the VCO phase steps and the clock steps of a bit period, pinned against compiler drift (CPU only:
the product's own assembly).

A period takes up to six samples; each costs a phase step (v_add_f64, v_cmp_le_f64 against 2 pi, v_cndmask_b32, and the wrap:
v_fmac_f64 / v_fma_f64 by 2 pi) and a clock step (v_cvt_f64_f32, v_add_f64, v_cvt_f32_f64).  The two chains need nothing from
each other, and one wave per SIMD issues in order, so the kernel lays all six steps of both out side by side in ONE block behind
the loop filter, in front of the test on `quick` (csrc/msk_lean.hip, front()); left alone the compiler moves phase steps 2-6
under that test, behind the clock steps.  Read off the assembly of `msk_lean_kernel<8,4,true>` (the bench's kernel), `<8,1,true>`
and `<4,1,true>`, compiled with the product's flags, for each of the eight periods of a segment:

 (1) all six wrap fmas of the period lie in front of the period's first s_and_saveexec_b64 (the test on `quick`);
 (2) in that span, counting only the operations of the two chains (phase: the add whose sum is compared with 2 pi, that compare,
     the wrap fma; clock: the two converts and the add between them), never two whole steps of one chain (six operations) follow
     each other without an operation of the other chain in between: at most five do (in the product's assembly the longest run
     is the compare and fma of one phase step and the whole next one, in period 0; four elsewhere), so the chains are
     interleaved step by step and neither waits for the other to finish;
 (3) the block guarded by `quick` (from that s_and_saveexec_b64 to the s_or_b64 that restores exec) holds commits only: no
     v_add_f64, no f64 fma, no narrowing convert (the compares of a committed clock with the threshold, and the widening of
     their operand, are there);
 (4) a laid-out period of `<8,1,true>` is 250..300 instructions long (tests/test_host_logic.py holds the same window; here so that
     an A/B arm that becomes the default cannot leave it unnoticed).

Period 0 has no shift-register pair in front of it to mark its start, so its span is the window in front of ITS s_and_saveexec_b64
that is as long as the longest span of periods 1..7.  A period holds that one exec-save and no other (the sixth clock step had a
block of its own), which is pinned as well.

That (1) can fail is checked on the old order, compiled from the same source with -DACG_LEAN_AB_VCO0 -DACG_LEAN_AB_SPEC0
-DACG_LEAN_AB_PICK0: exactly one wrap fma then lies in front of the test, in each of the periods 1..7.  (-DACG_LEAN_AB_VCO0 alone does not
bring the old order back: with the lane's phase pick issued beside each step, the steps' values are used outside the guarded
block, which is what keeps the compiler from moving them; that switch only takes the scheduling holds out.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = [(8, 4, True), (8, 1, True), (4, 1, True)]
OLD_ORDER = ["-DACG_LEAN_AB_VCO0", "-DACG_LEAN_AB_SPEC0", "-DACG_LEAN_AB_PICK0"]


def compile_lean(extra):
    from acarsdec_amd import _build as B
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
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
def product():
    return compile_lean([])


@pytest.fixture(scope="module")
def old_order():
    return compile_lean(OLD_ORDER)


def fronts(body, first=True):
    """per period: (the span in front of the test on `quick`, the guarded block behind it), and the lengths of periods 1..7.
    first=False: periods 1..7 only."""
    marks = [i for i, l in enumerate(body) if l.startswith("v_addc_co_u32_e64")]
    assert len(marks) == 16, len(marks)
    starts = [marks[i] for i in range(0, 16, 2)]            # the pair that closes period k opens period k + 1
    tests = [next(i for i in range(starts[k - 1], starts[k]) if body[i].startswith("s_and_saveexec_b64")) for k in range(1, 8)]
    where = [(starts[k], t) for k, t in enumerate(tests)]
    if first:
        # period 0: the nearest exec-save in front of the first pair (a period of the product holds one exec-save, see the test),
        # with a span as long as the longest of the others
        t0 = max(i for i in range(starts[0]) if body[i].startswith("s_and_saveexec_b64"))
        where.insert(0, (t0 - max(t - lo for lo, t in where), t0))
    out = []
    for lo, t in where:
        end = next(i for i in range(t, len(body)) if re.match(r"s_or_b64 exec, exec, ", body[i]))
        out.append((body[lo:t], body[t:end]))
    return out, [starts[k] - starts[k - 1] for k in range(1, 8)]


def chains(span):
    """the span's operations of the two chains in issue order, as a string of P (phase) and C (clock), and the number of wrap fmas.
    2 pi is the SGPR pair against which the span's v_cmp_le_f64 compare (`2 pi <= sum`)."""
    pairs = {m.group(1) for l in span for m in [re.match(r"v_cmp_le_f64_e64 s\[\d+:\d+\], (s\[\d+:\d+\]), v\[\d+:\d+\]$", l)] if m}
    assert len(pairs) == 1, pairs
    twopi = pairs.pop()
    seq, wraps = "", 0
    for i, l in enumerate(span):
        ops = [o.strip() for o in l.split(" ", 1)[1].split(",")] if " " in l else []
        if re.match(r"v_fmac?_f64", l) and twopi in ops[1:]:
            seq += "P"
            wraps += 1
        elif l.startswith("v_cmp_le_f64") and twopi in ops:
            seq += "P"
        elif l.startswith(("v_cvt_f64_f32", "v_cvt_f32_f64")):
            seq += "C"
        elif l.startswith("v_add_f64"):
            # whose sum is it?  The first instruction behind it that reads the sum tells (registers are reused along the span)
            use = next((m for m in span[i + 1:] if ops[0] in [o.strip() for o in m.split(" ", 1)[-1].split(",")][1:]), "")
            if use.startswith("v_cvt_f32_f64"):
                seq += "C"
            elif use.startswith("v_cmp_le_f64") and twopi in use:
                seq += "P"
    return seq, wraps


@pytest.mark.parametrize("key", KERNELS)
def test_phase_and_clock_steps_are_laid_out_side_by_side(product, key):
    body = product[key]
    spans, lengths = fronts(body)
    # the test on `quick` is the only exec-save of a period (the sixth clock step had one of its own): eight from the nearest one
    # in front of the first shift-register pair to the last pair
    marks = [i for i, l in enumerate(body) if l.startswith("v_addc_co_u32_e64")]
    t0 = max(i for i in range(marks[0]) if body[i].startswith("s_and_saveexec_b64"))
    assert sum(l.startswith("s_and_saveexec_b64") for l in body[t0:marks[-1]]) == 8, key
    if key == (8, 1, True):
        assert all(250 <= n <= 300 for n in lengths), lengths                                             # (4)
    for k, (span, guarded) in enumerate(spans):
        where = "<%d,%d,true> period %d" % (key[0], key[1], k)
        seq, wraps = chains(span)
        assert wraps == 6, (where, wraps, seq)                                                           # (1)
        assert len(guarded) <= 40, (where, "the guarded block closes right behind the test", len(guarded))
        if k > 0:                                                                                        # (period 0's span may start inside its first step)
            # six steps of each, three of their operations each; the clock is known before the period starts, so the widening
            # that opens its first step may lie in front of the shift-register pair
            assert seq.count("C") >= 17 and seq.count("P") >= 18, (where, seq)
        assert max(len(r) for r in re.findall(r"P+|C+", seq)) <= 5, (where, seq)                         # (2)
        assert not any(re.match(r"v_add_f64|v_fmac?_f64|v_cvt_f32_f64", l) for l in guarded), (where, guarded)   # (3)
        assert any(l.startswith("v_cndmask_b32") for l in guarded), where


def test_the_old_order_fails_the_first_condition(old_order):
    for key in KERNELS:
        spans, _ = fronts(old_order[key], first=False)
        for k, (span, guarded) in enumerate(spans):
            seq, wraps = chains(span)
            assert wraps == 1, (key, k + 1, wraps, seq)
