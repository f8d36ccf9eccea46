"""What an import costs the owner of a flight table shared by several contexts: the device time of the owner's part of a round
(HIP events inside acg_selftest_flights_sharded: the upload of the imported events, the label pass, the flight pass) for the
LARGEST round of tests/test_gpu_flight_shard.py's random traffic through four tables `c mod 4`, against the same round through
ONE table (nothing imported, no channel map: the launches every context made before export / import existed).

    python profiles/probe/flight_shard_pass.py [reps]

Prints, per arm, the round's records, events, imported events and its pass time over `reps` runs (median, min, max, ms), then the
same for the sum over all rounds."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from acarsdec_amd import decoder as D, _capi as K  # noqa: E402
import flight_model as FM  # noqa: E402
from test_gpu_flights import LABELS_B, T0, model_kw, random_records  # noqa: E402


def main(reps):
    rng = np.random.default_rng(20261021)
    n, nsh = 20000, 4
    recs = random_records(K, rng, n, 600, 64)
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(int(rng.integers(1, 501)), n - sum(sizes)))
    kw = dict(downlink_only=True, skip_empty=True, labels=LABELS_B)
    big = int(np.argmax(sizes))
    at = sum(sizes[:big])
    evs = [e for e in (FM.event_of(recs[i], T0, **model_kw(kw)) for i in range(at, at + sizes[big])) if e is not None]
    imported = sum(e.chn % nsh != 0 for e in evs)
    print("largest round: %d records, %d events, %d of them imported at the owner of %d shards (%d B uploaded)"
          % (sizes[big], len(evs), imported, nsh, imported * 88))
    nb = len(sizes)
    f = D.make_msg_filter(**kw)
    cfg = K.FlightConfig(T0[0], T0[1], 2, 2048)
    snaps, routes = (K.Flight * (1024 * nb))(), (K.Route * n)()
    out = {1: [], nsh: []}
    for r in range(reps + 1):                                   # (the first run of each arm is for nothing)
        for shards in (1, nsh) if r % 2 == 0 else (nsh, 1):
            snap_n, nroutes, dropped, ms = (C.c_int * nb)(), C.c_int(0), (C.c_int * nb)(), (C.c_float * nb)()
            rc = K.load().acg_selftest_flights_sharded(recs, (C.c_int * nb)(*sizes), nb, shards, C.byref(cfg), C.byref(f), snaps, len(snaps), snap_n,
                                                       routes, len(routes), C.byref(nroutes), dropped, ms)
            assert rc == K.OK, rc
            if r:
                out[shards].append((ms[big], sum(ms)))
    # the yardstick's second term: ONE upload of the imported events' bytes from pageable host memory, HIP events around it
    import torch
    host, dev = torch.zeros(imported * 88, dtype=torch.uint8), torch.empty(imported * 88, dtype=torch.uint8, device="cuda:0")
    e0, e1, up = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), []
    for r in range(reps + 1):
        e0.record()
        dev.copy_(host, non_blocking=True)
        e1.record()
        e1.synchronize()
        if r:
            up.append(e0.elapsed_time(e1))
    print("upload of %d B alone: median %.4f min %.4f max %.4f ms" % (imported * 88, np.median(up), min(up), max(up)))
    for shards in (1, nsh):
        a = np.array(out[shards])
        print("%d table(s): largest round median %.4f min %.4f max %.4f ms | all %d rounds median %.3f min %.3f max %.3f ms"
              % (shards, np.median(a[:, 0]), a[:, 0].min(), a[:, 0].max(), nb, np.median(a[:, 1]), a[:, 1].min(), a[:, 1].max()))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 15)
