"""A/B builds of the demodulator for same-box timing: python profiles/probe/build_ab.py NAME[:-DFLAG[,-DFLAG...]] ...
Each NAME becomes acarsdec_amd/lib/ab/libNAME.so = the product objects with msk.hip recompiled under the given flags
(a git revision may be given as NAME@REV:flags to take msk.hip from history).  profiles/probe/run_ab.sh times them all
on one box through ACARSDEC_AMD_LIB.  Measurement aid only; nothing here is loaded by the product.
Switches of msk_lean.hip may be given by their short names: a flag without a leading dash is taken as -DACG_LEAN_AB_<FLAG>
(round 7: TAPS0, PIN0, TAB0, BRS0; round 8: VCO0, SPEC0, PICK0, TAPSF1), and R07PARENT / R08PARENT stand for every old-order
switch of that round, the arm whose msk_lean assembly is the parent commit's."""
import os, subprocess, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
from acarsdec_amd import _build as B

MSK_FLAGS = B.MSK_FLAGS                 # the product's recipe (acarsdec_amd/_build.py)
GROUPS = {"R07PARENT": ["TAPS0", "PIN0", "TAB0", "BRS0"], "R08PARENT": ["VCO0", "SPEC0", "PICK0"]}
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
    src = os.path.join(B.CSRC, "msk.hip")
    if rev:
        src = os.path.join(out, "msk_%s.hip" % name)
        open(src, "w").write(subprocess.run(["git", "show", "%s:acarsdec_amd/csrc/msk.hip" % rev], cwd=ROOT, capture_output=True, text=True, check=True).stdout)
    obj = os.path.join(out, "msk_%s.o" % name)
    B._run([B.hipcc(), "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-I" + B.INC, "-I" + B.CSRC] + base + flags + ["-c", src, "-o", obj])
    # msk_lean.hip (round 6) under the same flags: its A/B switches are ACG_LEAN_AB_*
    obj2 = os.path.join(out, "msk_lean_%s.o" % name)
    lean_base = [f for i, f in enumerate(base) if not (f == "-disable-machine-sink" or (f == "-mllvm" and i + 1 < len(base) and base[i + 1] == "-disable-machine-sink"))]
    B._run([B.hipcc(), "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-I" + B.INC, "-I" + B.CSRC] + lean_base + flags + ["-c", os.path.join(B.CSRC, "msk_lean.hip"), "-o", obj2])
    # every other unit of the product library as build_lib() left it
    objs = [os.path.join(B.OBJDIR, n + ".o") for n, _, in_product in B.UNITS if in_product and n not in ("msk.hip", "msk_lean.hip")]
    objs += [os.path.join(B.OBJDIR, "host_setup.o"), obj, obj2]
    lib = os.path.join(out, "lib%s.so" % name)
    B._run([B.hipcc(), "--offload-arch=gfx950", "-shared", "-o", lib] + objs + ["-ldl", "-lm"])
    print(lib)
