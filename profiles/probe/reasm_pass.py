"""What the reassembly pass costs: pass_ms of acg_selftest_reasm beside the flight pass (acg_selftest_flights_sharded, one shard: label
pass + flight pass) on the same records, in one process.  `python profiles/probe/reasm_pass.py [runs]`; the first run of each arm is
the warm-up and stays out of the median.  Kernel by kernel: the same under `rocprofv3 --kernel-trace --stats`."""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import reasm_cases as RC  # noqa: E402
from acarsdec_amd import _capi as K  # noqa: E402

L = K.load(lab=True)
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7


def reasm_ms(msgs):
    n = len(msgs)
    arr = RC.pack(msgs)
    b = (C.c_int * 1)(n)
    cfg = K.ReasmConfig(1700000000, 0, 1024, 0)
    status = (C.c_ubyte * n)()
    done = (K.ReasmMsg * n)()
    cap = n * 242 + 16
    text = C.create_string_buffer(cap)
    nd, dr = C.c_int(0), C.c_int(0)
    ms = (C.c_float * 1)()
    out = []
    for _ in range(REPS):
        rc = L.acg_selftest_reasm(arr, b, 1, C.byref(cfg), None, status, done, n, text, cap, C.byref(nd), C.byref(dr), ms)
        assert rc == K.OK, rc
        out.append(ms[0])
    return out, nd.value, sum(1 for s in status if s != K.REASM_SKIPPED)


def flight_ms(msgs):
    n = len(msgs)
    arr = RC.pack(msgs)
    b = (C.c_int * 1)(n)
    cfg = K.FlightConfig(1700000000, 0, 600, 4096)
    snaps = (K.Flight * 4096)()
    sn = (C.c_int * 1)()
    routes = (K.Route * max(n, 1))()
    nr = C.c_int(0)
    dr = (C.c_int * 1)()
    ms = (C.c_float * 1)()
    out = []
    for _ in range(REPS):
        rc = L.acg_selftest_flights_sharded(arr, b, 1, 1, C.byref(cfg), None, snaps, 4096, sn, routes, n, C.byref(nr), dr, ms)
        assert rc == K.OK, rc
        out.append(ms[0])
    return out, sn[0]


def bench_shaped(n=4000):
    """a take like the bench's: nearly all single-block downlinks from many aircraft, one chain in fifty"""
    import random
    rng = random.Random(3)
    out = []
    t = 100000
    for i in range(n):
        t += rng.randint(1, 40)
        chain = i % 50 == 0
        out.append(RC.msg(addr=b"B%05d" % rng.randrange(600), label=b"H1", bid=b"%d" % (i % 10), no=b"M%02dA" % (i % 100), be=RC.ETB if chain else RC.ETX,
                          txt=RC.text_of(i, rng.randint(20, 200)), end_sample=t, chn=i % 1024, back=rng.randint(500, 10000)))
    return out


res = {}
for name, msgs in (("bench_shaped_4000", bench_shaped()), ("random_20000", RC.random_traffic())):
    r, ndone, nev = reasm_ms(msgs)
    f, nfl = flight_ms(msgs)
    res[name] = dict(records=len(msgs), events=nev, completed=ndone, flights=nfl, reasm_ms=[round(v, 4) for v in r], flight_ms=[round(v, 4) for v in f],
                     reasm_median=round(statistics.median(r[1:]), 4), flight_median=round(statistics.median(f[1:]), 4))
print(json.dumps(res))
