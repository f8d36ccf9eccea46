"""What the rate down-converter (csrc/fir_rate.hip) costs beside its sibling, the workgroup-granular kernels of whole windows.

    python profiles/probe/rate_fir.py [calls per round] [rounds]

One process, 4096 channels on one stream each, 2 callbacks (2048 windows) per call, ACG_F_TIMING with acg_set_timing(2): HIP
events around every down-converter launch while the demodulator runs beside it, as in a real call.  Arms, alternated in every
round after two unrecorded calls each:
  rate-cf32, rate-cs16, rate-cu8   acg_process_rate_dev at 2 048 000 Hz (L in {163, 164}): the new kernel
  cf32-164, cs16-164    acg_process_samples_dev at M = 164: fir_fmt_kernel<CF32 / CS16>, the same structure without the grid
  u8-164                acg_process_iq_u8_dev at M = 164: 164 is no multiple of 8, so this is the exact-order kernel (one thread per
                        output), what the u8 entry point has at that length today
  u8-168                ... at M = 168: fir_u8_persist_kernel, the u8 path's workgroup-granular kernel at the nearest length it takes
Per arm: ms per launch (median, min, max over the rounds), launches per call, input bytes per second of launch time / 8 TB/s."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from acarsdec_amd import decoder as D, _capi as K  # noqa: E402

NCH, NBLK, RATE, HBM = 4096, 2, 2048000, 8e12
NWIN = NBLK * 1024


def make_arm(name, buf):
    rng = np.random.default_rng(1)
    if name.startswith("rate"):
        fmt, bps = {"rate-cf32": (K.FMT_CF32, 8), "rate-cs16": (K.FMT_CS16, 4), "rate-cu8": (K.FMT_CU8, 2)}[name]
        M = D.rate_decim(RATE)
        dec = D.Decoder(NCH, decim=M, max_blocks=NBLK, bitlog=False, timing=True)
        dec.set_taps(np.stack([D.rate_taps(RATE, 12500.0 * int(k)) for k in rng.integers(2, 40, NCH)]))
        dec.set_input_rate(RATE)
        nsamp = NWIN * M                                    # 2048 windows fit from any grid position
        pitch = (nsamp * bps + 15) & ~15
        call = lambda: dec.process_rate(fmt, buf, nsamp, pitch)
        nbytes = NCH * NWIN * RATE / 12500.0 * bps
    else:
        kind, M = name.split("-")
        M = int(M)
        dec = D.Decoder(NCH, decim=M, max_blocks=NBLK, bitlog=False, timing=True)
        dec.set_taps(np.stack([D.soapy_taps(131e6 + 12500.0 * int(k), 131000000, M) for k in rng.integers(2, 40, NCH)]))
        bps = {"cf32": 8, "cs16": 4, "u8": 2}[kind]
        pitch = NWIN * M * bps
        if kind != "u8":
            call = lambda: dec.process_samples(K.FMT_CF32 if kind == "cf32" else K.FMT_CS16, buf, NBLK, pitch, 0)
        else:
            call = lambda: dec.in_callback(buf, nblocks=NBLK, pitch=pitch)
        nbytes = NCH * NWIN * M * bps
    assert buf.numel() * buf.element_size() >= NCH * pitch, (name, "the rows lie outside the buffer")
    dec.set_timing(2)
    return dec, call, nbytes


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    assert K.load().acg_device_count() > 0
    big = NCH * NWIN * 168 * 8 + 64                          # the widest arm's rows
    f32 = torch.empty(big // 4, dtype=torch.float32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(2)
    step = 1 << 28
    for o in range(0, f32.numel(), step):
        f32[o: o + step].uniform_(-1.0, 1.0, generator=g)
    u8 = torch.randint(0, 256, (NCH * NWIN * 168 * 2 + 64,), dtype=torch.uint8, device="cuda", generator=g)
    names = ["rate-cf32", "cf32-164", "rate-cs16", "cs16-164", "rate-cu8", "u8-164", "u8-168"]
    arms = {n: make_arm(n, u8 if "u8" in n else f32) for n in names}             # (int16 samples: any bytes, 4 per sample)
    rec = {n: [] for n in names}
    launches = {}
    for r in range(rounds):
        for n in names:
            dec, call, _ = arms[n]
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
    out = {"device": torch.cuda.get_device_name(0), "nch": NCH, "windows_per_call": NWIN, "calls_per_round": calls, "rounds": rounds}
    for n in names:
        v = sorted(rec[n])
        med = v[len(v) // 2]
        per_launch = arms[n][2] / launches[n]
        out[n] = dict(ms_per_launch=dict(median=med, min=v[0], max=v[-1]), launches_per_call=launches[n], bytes_per_launch=per_launch,
                      of_hbm=dict(median=per_launch / (med * 1e-3) / HBM, best=per_launch / (v[0] * 1e-3) / HBM))
    for n in names:
        arms[n][0].close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
