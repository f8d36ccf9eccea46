"""The combined outputs pass against the two sink passes it replaces (LEDGER, "Combined outputs"): acg_lab_time_output_passes over
n designed records (tests/outputs_records.py lab_records, the plain module the GPU test takes them from), arm A = json.hip's
passes followed by text.hip's, arm B = outs.hip's pass with legs {JSON, that text format}, alternated within every round; HIP
events on one stream; the lab library.
  python profiles/probe/outputs_pass.py [n=4096] [rounds=3] [reps=200] [warmup=20]
Prints, per text format and round, each arm's (min, median, max) in ms as one JSON line."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from acarsdec_amd import _capi as K, decoder as D      # noqa: E402
import outputs_records as T                            # noqa: E402


def main():
    n, rounds, reps, warm = (int(sys.argv[1 + i]) if len(sys.argv) > 1 + i else d for i, d in enumerate((4096, 3, 200, 20)))
    L = K.load(lab=True)
    recs = T.lab_records(np.random.default_rng(n), n, K)
    buf = (K.Msg * n).from_buffer_copy(recs.tobytes())
    for name, leg in (("std+date+freq", ("std", dict(date=True, freq=True))), ("sv", "sv")):
        cfg = D.outputs_config(["json", leg], T.T0_LAB, b"STN1", b"acarsdec", b"3.7")
        for rnd in range(rounds):
            ms = np.zeros(2 * reps, dtype=np.float32)
            rc = L.acg_lab_time_output_passes(buf, n, C.byref(cfg), T.NCH_LAB, warm, reps, ms.ctypes.data)
            assert rc == K.OK, rc
            a, b = ms[:reps], ms[reps:]
            stat = lambda v: [round(float(v.min()), 4), round(float(np.median(v)), 4), round(float(v.max()), 4)]
            print(json.dumps({"text": name, "n": n, "round": rnd, "A_json_then_text_ms": stat(a), "B_combined_ms": stat(b)}))


if __name__ == "__main__":
    main()
