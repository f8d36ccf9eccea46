"""What the channel map of acg_set_channel_numbers costs the sinks' passes, and what acg_sink_keys costs.

    python profiles/probe/sink_channel_map.py [rounds] [LIB ...]

The JSON and the text (-o 2 with date and "F:") passes over 16 384 records of 1024 channels (the records of text_sink.py's wide
traffic, repeated with fresh end_bits), timed by acg_lab_time_sink_passes: HIP events around each renderer's launches on an
otherwise idle device.  One process per arm and round, the arms ALTERNATED round by round in one call, so drift of the box shows
as a spread inside every arm and not as a difference between them:

  LIB ...    other builds of the library (the parent commit's, built from a worktree), each an arm of its own: the records come
             from this tree's library, the timed passes are that library's (it need not export what this tree added);
  tree       this tree's library, no map;
  tree+map   this tree's library with ACG_SINK_MAP=1: the passes look every record's number up (slot l -> 1023 - l).

Per arm: the medians of the rounds' medians (30 timed passes a round) and their range over the rounds -- the arm's own run-to-run
range, which is what a difference between two arms has to exceed.  Then acg_sink_keys after a drain of 16 384 JSON lines would need
a context that holds them; its cost is taken where it is the same: a copy of nrecs x 8 bytes behind a sink call of the wide
traffic (1024 channels, about 4000 lines), wall clock around the C call, median of 200."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
N, NCH, REPS = 16384, 1024, 30


def one_round(use_map, lib=None):
    """in a process of its own: [JSON median, text median] ms"""
    from acarsdec_amd import decoder as D, _capi as K
    import text_sink as TS
    L = K.load()
    if lib:
        L = C.CDLL(lib)
        L.acg_lab_time_sink_passes.restype, L.acg_lab_time_sink_passes.argtypes = K.LAB_SYMBOLS["acg_lab_time_sink_passes"]
    if use_map:
        K.tune("ACG_SINK_MAP", "1")
    base = TS.drain_all(TS.wide(), NCH)
    buf = (K.Msg * N)()
    sz = C.sizeof(K.Msg)
    for i in range(N):                                           # the wide traffic's records again and again, keys kept distinct
        C.memmove(C.addressof(buf) + i * sz, C.addressof(base[i % len(base)]), sz)
        buf[i].end_bit = base[i % len(base)].end_bit + 100000 * (i // len(base))
    jcfg = D.json_config(TS.T0, "STN1", "acarsdec", "3.7")
    tcfg = D.text_config("std", TS.T0, station_id="STN1", date=True, freq=True)
    ms = np.zeros(2 * REPS, dtype=np.float32)
    rc = L.acg_lab_time_sink_passes(buf, N, C.byref(jcfg), C.byref(tcfg), NCH, 5, REPS, ms.ctypes.data)
    assert rc == K.OK, rc
    return [float(np.median(ms[:REPS])), float(np.median(ms[REPS:]))]


def keys_cost():
    from acarsdec_amd import decoder as D, _capi as K
    import text_sink as TS
    y = TS.wide()
    dec = D.Decoder(NCH, decim=8, ntaps=8, max_blocks=TS.CHUNK // 1024, repair=True, bitlog=False)
    dec.enable_json(TS.T0, "STN1", "acarsdec", "3.7")
    dec.set_channel_numbers(np.arange(NCH)[::-1].copy())
    for s in range(0, y.shape[1], TS.CHUNK):
        dec.demod_msk(y[:, s:s + TS.CHUNK])
    nlines = len(dec.drain_json(max_lines=8192).split(b"\n")) - 1
    keys = np.zeros(8192, dtype=np.uint64)
    n = C.c_int(0)
    took = []
    for _ in range(220):
        t = time.perf_counter()
        rc = dec.L.acg_sink_keys(dec.ctx, K.SINK_JSON, keys.ctypes.data, len(keys), C.byref(n))
        took.append(time.perf_counter() - t)
        assert rc == K.OK and n.value == nlines
    dec.close()
    took = np.array(took[20:]) * 1e6
    return nlines, float(np.median(took)), float(took.min()), float(took.max())


def main(rounds, libs):
    arms = [(os.path.basename(l), [os.path.abspath(l)], "0") for l in libs] + [("tree", [], "0"), ("tree+map", [], "1")]
    got = {name: [] for name, _, _ in arms}
    for r in range(rounds):
        for name, env, use_map in arms:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--round", use_map] + env, capture_output=True, text=True, timeout=300,
                                 check=True).stdout
            got[name].append(json.loads(out.strip().splitlines()[-1]))
            print("round %d %-12s JSON %.4f ms  text %.4f ms" % (r, name, *got[name][-1]), flush=True)
    for name, _, _ in arms:
        a = np.array(got[name])
        print("%-12s %d records: JSON passes median %.4f ms (rounds %.4f .. %.4f) | text passes median %.4f ms (rounds %.4f .. %.4f)" % (
            name, N, np.median(a[:, 0]), a[:, 0].min(), a[:, 0].max(), np.median(a[:, 1]), a[:, 1].min(), a[:, 1].max()), flush=True)
    print("acg_sink_keys: %d keys, median %.1f us (min %.1f, max %.1f)" % keys_cost(), flush=True)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if len(sys.argv) > 2 and sys.argv[1] == "--round":
        print(json.dumps(one_round(sys.argv[2] == "1", sys.argv[3] if len(sys.argv) > 3 else None)))
    else:
        main(int(sys.argv[1]) if len(sys.argv) > 1 else 5, sys.argv[2:])
