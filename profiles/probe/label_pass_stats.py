"""Sums the kernel dispatches of a rocprofv3 --kernel-trace database of profiles/probe/label_pass_cost.py per width (1024, then
16 384 channels): launches, total and mean time per kernel.  Usage: python profiles/probe/label_pass_stats.py <labels_results.db>"""
import sqlite3, collections, sys
c=sqlite3.connect(sys.argv[1])
rows=c.execute("select name, start, end, grid_x from kernels order by start").fetchall()
# two runs (1024 then 16384 channels): split where the split kernel's workgroup count jumps, i.e. by msk grid
short=lambda n: n.split('(')[0].replace('void ','')
runs=[[],[]]
# find the first msk launch whose grid is the 16384-channel one (largest)
mskg=[r[3] for r in rows if 'msk' in r[0]]
big=max(mskg)
first_big=min(r[1] for r in rows if 'msk' in r[0] and r[3]==big)
for r in rows:
    runs[1 if r[1]>=first_big else 0].append(r)
for w,run in zip((1024,16384),runs):
    agg=collections.defaultdict(lambda:[0,0.0])
    for n,s,e,g in run:
        a=agg[short(n)]; a[0]+=1; a[1]+=(e-s)/1e3
    print("== %d channels" % w)
    for k,(cnt,us) in sorted(agg.items(), key=lambda x:-x[1][1]):
        print("  %-40s %4d launches %10.1f us total %8.2f us/launch" % (k,cnt,us,us/cnt))
