"""What the shared-stream vector kernel (csrc/fir_tile_kernel.h: fir_u8_shared_kernel) costs per launch.

    python profiles/probe/shared_fir.py [calls per round] [rounds] [tree to import acarsdec_amd from]

One process, 256 streams feeding 16 channels each (4096 channels), 2 callbacks (2048 windows) per call, ACG_FIR_MM=0 so that the
matrix pipe does not take the launch, ACG_F_TIMING with acg_set_timing(2): HIP events around every down-converter launch while the
demodulator runs beside it, as in a real call.  Arms, alternated in every round after two unrecorded calls each:
  shared-u8-200, shared-u8-160   acg_process_iq_u8_dev: fir_u8_shared_kernel<true, false>
  shared-s8-200                  acg_process_samples_dev, complex int8: fir_u8_shared_kernel<true, true>
Per arm: ms per launch (median, min, max over the rounds) and launches per call."""
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from acarsdec_amd import decoder as D, _capi as K  # noqa: E402

NS, PER, NBLK = 256, 16, 2
NCH, NWIN = NS * PER, NBLK * 1024


def make_arm(name, buf):
    rng = np.random.default_rng(1)
    _, kind, M = name.split("-")
    M = int(M)
    dec = D.Decoder(NCH, decim=M, nstreams=NS, max_blocks=NBLK, bitlog=False, timing=True)
    dec.set_taps(np.stack([D.soapy_taps(131e6 + 12500.0 * int(k), 131000000, M) for k in rng.integers(2, 40, NCH)]))
    dec.set_channel_streams(np.repeat(np.arange(NS), PER).astype(np.int32))
    pitch = NWIN * M * 2
    if kind == "s8":
        assert dec.samples_launch(K.FMT_CS8, NBLK).family == K.FIR_SHARED_VECTOR
        call = lambda: dec.process_samples(K.FMT_CS8, buf, NBLK, pitch, 0)
    else:
        assert dec.launch_shape(NBLK).kernel == 0
        call = lambda: dec.in_callback(buf, nblocks=NBLK, pitch=pitch)
    dec.set_timing(2)
    return dec, call


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    assert os.path.dirname(os.path.dirname(os.path.abspath(D.__file__))) == ROOT, D.__file__
    assert K.load().acg_device_count() > 0
    K.tune("ACG_FIR_MM", "0")
    g = torch.Generator(device="cuda").manual_seed(2)
    u8 = torch.randint(0, 256, (NS * NWIN * 200 * 2 + 64,), dtype=torch.uint8, device="cuda", generator=g)
    names = ["shared-u8-200", "shared-s8-200", "shared-u8-160"]
    arms = {n: make_arm(n, u8) for n in names}
    rec = {n: [] for n in names}
    launches = {}
    for r in range(rounds):
        for n in names:
            dec, call = arms[n]
            for _ in range(2):
                call()
            dec.sync()
            dec.timing()
            for _ in range(calls):
                call()
            dec.sync()
            t = dec.timing()
            dec.drain_frames_raw()
            rec[n].append(t["fir_ms"] / t["fir_launches"])
            launches[n] = t["fir_launches"] / calls
    out = {"device": torch.cuda.get_device_name(0), "tree": ROOT, "nch": NCH, "streams": NS, "windows_per_call": NWIN, "calls_per_round": calls, "rounds": rounds}
    for n in names:
        v = sorted(rec[n])
        out[n] = dict(ms_per_launch=dict(median=v[len(v) // 2], min=v[0], max=v[-1]), launches_per_call=launches[n])
    for n in names:
        arms[n][0].close()
    print(json.dumps(out, indent=1))


main()
