"""Idle time on the demodulator stream, from a rocprofv3 trace of bench.py:
rocprofv3 --kernel-trace --hip-trace -f csv -d DIR -o NAME -- python bench.py --gpus 1
python profiles/probe/stream_gaps.py DIR [warm-up launches, default 66 = 3 steps of 22 calls]
Per launch of the demodulator kernel: its duration, and the gap between the end of the launch before it and its start.  The
launches of warm-up run with timing mode 1 (a start and an end record around every demodulator launch), the timed region with
mode 2 (benchlib/timing.py: none on that stream), so the two groups are the same stream with four and with two packets between
two kernels.  A gap above 100 us is a step boundary or a host wait, not the stream's packets: counted apart."""
import csv, glob, os, sys
from collections import Counter

d = sys.argv[1]
nwarm = int(sys.argv[2]) if len(sys.argv) > 2 else 66


def rows(suffix):
    out = []
    for p in sorted(glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True)):
        with open(p, newline="") as f:
            out += list(csv.DictReader(f))
    return out


def q(v, f):
    v = sorted(v)
    return v[min(len(v) - 1, int(f * len(v)))] if v else float("nan")


def line(name, v):
    if not v:
        print("%-44s none" % name)
        return
    print("%-44s n=%4d  mean %8.2f  min %8.2f  p10 %8.2f  median %8.2f  p90 %8.2f  max %8.2f us" % (
        name, len(v), sum(v) / len(v), min(v), q(v, 0.1), q(v, 0.5), q(v, 0.9), max(v)))


k = rows("kernel_trace.csv")
msk = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in k if "msk_lean_kernel" in r["Kernel_Name"]))
fir = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in k if r["Kernel_Name"].startswith("fir_") or " fir_" in r["Kernel_Name"]]
print("kernels: %d rows, %d demodulator launches, %d down-converter launches" % (len(k), len(msk), len(fir)))
for name, lo, hi in (("warm-up (timing mode 1)", 0, nwarm), ("timed region (timing mode 2)", nwarm, len(msk))):
    part = msk[lo:hi]
    dur = [(e - s) / 1e3 for s, e in part]
    gap = [(part[i + 1][0] - part[i][1]) / 1e3 for i in range(len(part) - 1)]
    small = [g for g in gap if g <= 100.0]
    big = [g for g in gap if g > 100.0]
    print("--", name)
    line("  kernel duration", dur)
    line("  gap to the launch before, <= 100 us", small)
    line("  gap to the launch before, > 100 us", big)
    if part:
        span = (part[-1][1] - part[0][0]) / 1e3
        print("  span %.1f us: kernels %.2f %%, small gaps %.2f %%, large gaps %.2f %%" % (
            span, 100 * sum(dur) / span, 100 * sum(small) / span, 100 * sum(big) / span))
line("down-converter duration (all)", fir)
h = rows("hip_api_trace.csv")
if h:
    c = Counter(r["Function"] for r in h)
    print("HIP calls:", ", ".join("%s %d" % kv for kv in c.most_common(14)))
