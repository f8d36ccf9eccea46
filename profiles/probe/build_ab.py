"""A/B builds of the demodulator for same-box timing: python profiles/probe/build_ab.py NAME[@REV][:-DFLAG[,-DFLAG...]] ...
Each NAME becomes acarsdec_amd/lib/ab/libNAME.so = the product objects with msk.hip and msk_lean.hip recompiled under the given
flags.  With @REV the demodulator's sources (msk.hip, msk_lean.hip, msk_common.h) are taken from that git revision: the arms whose
verdict is closed (profiles/LEDGER.md) are no longer in the tree, and the revision named there still has their switches
(NAME@REV:-DSWITCH).  profiles/probe/run_ab.sh times them all on one box through ACARSDEC_AMD_LIB.  Measurement aid
only; nothing here is loaded by the product.
The switches msk_lean.hip keeps may be given by their short names: a flag without a leading dash is taken as -DACG_LEAN_AB_<FLAG>
(VCO0, SPEC0, PICK0, REC0), R08PARENT stands for the first three, the order before round 8, and REC0 is the order before round 9
(a bit record stored by all 64 lanes in every period).  Round 10's steps, each the order before it: WAIT0 (the compiler's three waits
in front of the old taps), NOP0 (the clock in the hold of step 5), HORN0 (the Horner steps of the mixer's series left to the compiler);
R10PARENT stands for all three.  CLOSE0 (round 11): the lean kernel's closing period without frame_bit()'s select paths for the
byte closes in SYN2, SOH1 and END -- every close that is neither `hunt` nor `plain` through decode_acars(), as in msk.hip."""
import os, subprocess, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
from acarsdec_amd import _build as B

MSK_FLAGS = B.MSK_FLAGS                 # the product's recipe (acarsdec_amd/_build.py)
GROUPS = {"R08PARENT": ["VCO0", "SPEC0", "PICK0"], "R10PARENT": ["WAIT0", "NOP0", "HORN0"]}
SOURCES = ("msk.hip", "msk_lean.hip", "msk_common.h")
B.build_lib()
out = os.path.join(B.LIBDIR, "ab")
os.makedirs(out, exist_ok=True)
for spec in sys.argv[1:]:
    name, _, flags = spec.partition(":")
    name, _, rev = name.partition("@")
    flags = [g for f in flags.split(",") if f for g in GROUPS.get(f, [f])]
    flags = [f if f.startswith(("-", "DROP=")) else "-DACG_LEAN_AB_" + f for f in flags]
    drop = [f[5:] for f in flags if f.startswith("DROP=")]          # DROP=substr: leave out the product flags containing it
    flags = [f for f in flags if not f.startswith("DROP=")]
    base = []
    it = iter(MSK_FLAGS)
    for f in it:
        if f == "-mllvm":
            v = next(it)
            if not any(d in v for d in drop):
                base += [f, v]
        elif not any(d in f for d in drop):
            base.append(f)
    srcdir, inc = B.CSRC, ["-I" + B.INC, "-I" + B.CSRC]
    if rev:
        # the revision's demodulator sources in a directory of their own, in front of the tree's on the include path
        srcdir = os.path.join(out, "src_%s" % name)
        os.makedirs(srcdir, exist_ok=True)
        for f in SOURCES + ("msk_lean_kernel.h",):
            r = subprocess.run(["git", "show", "%s:acarsdec_amd/csrc/%s" % (rev, f)], cwd=ROOT, capture_output=True, text=True)
            if r.returncode != 0 and f == "msk_lean_kernel.h":
                continue                               # (revisions before round 12 have the kernel's text in msk_lean.hip itself)
            r.check_returncode()
            open(os.path.join(srcdir, f), "w").write(r.stdout)
        inc = ["-I" + srcdir] + inc
    cc = [B.hipcc(), "--offload-arch=gfx950", "-std=c++17", "-fPIC"] + inc
    obj = os.path.join(out, "msk_%s.o" % name)
    B._run(cc + base + flags + ["-c", os.path.join(srcdir, "msk.hip"), "-o", obj])
    # msk_lean.hip under the same flags, with machine sinking left on as in the product's recipe
    obj2 = os.path.join(out, "msk_lean_%s.o" % name)
    lean_base = [f for i, f in enumerate(base) if not (f == "-disable-machine-sink" or (f == "-mllvm" and i + 1 < len(base) and base[i + 1] == "-disable-machine-sink"))]
    B._run(cc + lean_base + flags + ["-c", os.path.join(srcdir, "msk_lean.hip"), "-o", obj2])
    # every other unit of the product library as build_lib() left it
    objs = [os.path.join(B.OBJDIR, n + ".o") for n, _, in_product in B.UNITS if in_product and n not in ("msk.hip", "msk_lean.hip")]
    objs += [os.path.join(B.OBJDIR, "host_setup.o"), obj, obj2]
    lib = os.path.join(out, "lib%s.so" % name)
    B._run([B.hipcc(), "--offload-arch=gfx950", "-shared", "-o", lib] + objs + ["-ldl", "-lm"])
    print(lib)
