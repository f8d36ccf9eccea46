"""What a monitor frame costs: acg_flight_monitor_text beside acg_flight_snapshot on the SAME table in ONE process, host wall
clock around each call (launches, the device passes, the copy of the result, the synchronise), the two alternated inside every
round.  The table is filled through the whole chain: synthetic downlinks from more aircraft than the table holds, so that it is
full (the live count is printed; a table stops taking new aircraft a little before its last slot, acarsdec_amd.h).

    python profiles/probe/flight_text.py [rounds]

Prints per table size (1024 and 16384 slots): live entries, frame bytes, median / min / max in ms of both calls; then the same
for the route pass (acg_drain_routes_json) over the routes that traffic queued."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from acarsdec_amd import _capi as K, decoder as D, synth as S  # noqa: E402


def traffic(nch, per_channel, seed=5):
    """[nch, n] float32: per channel `per_channel` downlinks, every one from an aircraft of its own"""
    rng = np.random.default_rng(seed)
    chunk, gap = 4096, 1100
    one = S.msk_audio(S.frame_bits(S.acars_frame(text=b"M01AXY0123EGLLKJFK0815", addr=b".N00000", label=b"QP", bid=b"4")), phase0=0.0).size
    n = 2000 + per_channel * (one + gap)
    n += (-n) % chunk
    x = np.zeros((nch, n), dtype=np.float32)
    k = 0
    for c in range(nch):
        pos = 1000 + int(rng.integers(0, 500))
        for _ in range(per_channel):
            fr = S.acars_frame(text=b"M01A" + (b"XY%04d" % (k % 10000)) + b"EGLLKJFK0815", addr=b".%06d" % k, label=b"QP", bid=b"4")
            a = S.msk_audio(S.frame_bits(fr), phase0=float(rng.uniform(0, 2 * np.pi)))
            x[c, pos:pos + a.size] = 0.06 * a
            pos += a.size + gap
            k += 1
    return x, chunk


def measure(x, chunk, slots, rounds):
    nch = x.shape[0]
    dec = D.Decoder(nch, decim=8, ntaps=8, max_blocks=chunk // 1024, repair=True, bitlog=False)
    dec.enable_flights(t0=(1700000000, 0), mdly=600, max_flights=slots)
    dec.enable_flight_text(16, "st1")
    got = 0
    for s in range(0, x.shape[1], chunk):
        dec.demod_msk(x[:, s:s + chunk])
        got += len(dec.drain_msgs(max_msgs=65536))
    snap = (K.Flight * slots)()
    text = C.create_string_buffer(K.MONITOR_HDR_LEN + slots * K.MONITOR_ROW_MAX)
    n, dropped, nb, nrows = C.c_int(0), C.c_int(0), C.c_size_t(0), C.c_int(0)
    t_snap, t_text = [], []
    for r in range(5 + rounds):
        t0 = time.perf_counter()
        rc1 = dec.L.acg_flight_snapshot(dec.ctx, snap, slots, C.byref(n), C.byref(dropped))
        t1 = time.perf_counter()
        rc2 = dec.L.acg_flight_monitor_text(dec.ctx, -1, text, len(text), C.byref(nb), C.byref(nrows), None)
        t2 = time.perf_counter()
        assert rc1 == K.OK and rc2 == K.OK and nrows.value == n.value, (rc1, rc2)
        if r >= 5:
            t_snap.append((t1 - t0) * 1e3)
            t_text.append((t2 - t1) * 1e3)
    f = lambda t: "%.3f / %.3f / %.3f" % (float(np.median(t)), min(t), max(t))
    print("slots %d: messages %d, live entries %d, frame %d bytes (snapshot %d bytes); ms median / min / max over %d rounds: "
          "acg_flight_snapshot %s, acg_flight_monitor_text %s" % (slots, got, n.value, nb.value, 120 * n.value, rounds, f(t_snap), f(t_text)), flush=True)
    # the route pass on the routes this traffic queued: with no room for the lines the call runs all of it (keys, sort, measure,
    # scan, render, the counters' copy), answers ACG_EAGAIN and consumes nothing, so it can be repeated; what it leaves out is
    # the copy of the lines
    t_route = []
    for r in range(5 + rounds):
        t0 = time.perf_counter()
        rc = dec.L.acg_drain_routes_json(dec.ctx, None, 0, C.byref(nb), C.byref(nrows))
        t_route.append((time.perf_counter() - t0) * 1e3)
        assert rc == (K.EAGAIN if nrows.value else K.OK), rc
    dec.close()
    print("slots %d: route pass over %d queued routes, %d bytes of lines; ms median / min / max over %d rounds: %s"
          % (slots, nrows.value, nb.value, rounds, f(t_route[5:])), flush=True)


if __name__ == "__main__":
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    x, chunk = traffic(2048, 10)
    for slots in (1024, 16384):
        measure(x, chunk, slots, rounds)
