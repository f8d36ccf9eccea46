"""What a channel filter over several windows (csrc/fir_long.hip) costs beside the plain rate kernel of the same process.

    python profiles/probe/long_fir.py [calls per round] [rounds]

One process, 2.0 Msps (M = 160), 2 callbacks (2048 windows) per call, ACG_F_TIMING with acg_set_timing(2): HIP events around every
down-converter launch while the demodulator runs beside it, as in a real call.  Arms, alternated in every round after two
unrecorded calls each:
  <fmt>-off, <fmt>-J2, <fmt>-J4   4096 channels on one stream each, fmt in cu8, cs16, cf32: the rate kernel, then the filter
  shared-<fmt>-J4                 2048 streams x 8 channels (the vector kernel re-reads the stream per channel)
Per arm: ms per launch (median, min, max over the rounds' means), launches per call, the streams' input bytes per second of
launch time / 8 TB/s, and channel-samples per second."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from acarsdec_amd import decoder as D, _capi as K  # noqa: E402

RATE, M, NBLK, HBM = 2000000, 160, 2, 8e12
NWIN = NBLK * 1024
FMTS = {"cu8": (K.FMT_CU8, 2), "cs16": (K.FMT_CS16, 4), "cf32": (K.FMT_CF32, 8)}


def filter_tables(nch, J):
    rng = np.random.default_rng(J)
    one = {int(k): D.channel_filter_taps(RATE, 12500.0 * int(k), J) for k in range(2, 40)}
    return np.stack([one[int(k)] for k in rng.integers(2, 40, nch)])


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    assert K.load().acg_device_count() > 0
    g = torch.Generator(device="cuda").manual_seed(2)
    nstreams = 4096
    f32 = torch.empty(nstreams * NWIN * M * 2 + 16, dtype=torch.float32, device="cuda")
    step = 1 << 28
    for o in range(0, f32.numel(), step):
        f32[o: o + step].uniform_(-1.0, 1.0, generator=g)
    u8 = torch.randint(0, 256, (nstreams * NWIN * M * 2 + 64,), dtype=torch.uint8, device="cuda", generator=g)
    rng = np.random.default_rng(1)
    box = {n: np.stack([D.rate_taps(RATE, 12500.0 * int(k)) for k in rng.integers(2, 40, n)]) for n in (4096, 16384)}
    wide = D.Decoder(4096, decim=M, max_blocks=NBLK, bitlog=False, timing=True)
    shared = D.Decoder(16384, decim=M, nstreams=2048, max_blocks=NBLK, bitlog=False, timing=True)
    shared.set_channel_streams(np.arange(16384, dtype=np.int32) // 8)
    for dec, n in ((wide, 4096), (shared, 16384)):
        dec.set_taps(box[n])
        dec.set_input_rate(RATE)
        dec.set_timing(2)
    tables = {(4096, 2): filter_tables(4096, 2), (4096, 4): filter_tables(4096, 4), (16384, 4): filter_tables(16384, 4)}
    arms = []                                                   # (name, decoder, channels, streams, J, format)
    for f in FMTS:
        arms += [("%s-off" % f, wide, 4096, 4096, 0, f), ("%s-J2" % f, wide, 4096, 4096, 2, f), ("%s-J4" % f, wide, 4096, 4096, 4, f)]
    arms += [("shared-%s-J4" % f, shared, 16384, 2048, 4, f) for f in FMTS]
    rec = {a[0]: [] for a in arms}
    launches = {}
    for r in range(rounds):
        for name, dec, nch, ns, J, f in arms:
            fmt, bps = FMTS[f]
            dec.set_channel_filter(tables[(nch, J)] if J else None)
            nsamp = NWIN * M
            pitch = nsamp * bps
            buf = u8 if f == "cu8" else f32                     # (int16 samples: any bytes, 4 per sample)
            assert buf.numel() * buf.element_size() >= ns * pitch
            call = lambda: dec.process_rate(fmt, buf, nsamp, pitch)
            for _ in range(2):
                call()
            dec.sync()
            dec.timing()
            for _ in range(calls):
                call()
            dec.sync()
            t = dec.timing()
            dec.drain_frames_raw()
            rec[name].append(t["fir_ms"] / t["fir_launches"])
            launches[name] = t["fir_launches"] / calls
    out = {"device": torch.cuda.get_device_name(0), "rate": RATE, "windows_per_call": NWIN, "calls_per_round": calls, "rounds": rounds}
    for name, dec, nch, ns, J, f in arms:
        v = sorted(rec[name])
        med = v[len(v) // 2]
        per_launch = ns * NWIN * M * FMTS[f][1] / launches[name]
        chs = nch * NWIN * M / launches[name]
        out[name] = dict(ms_per_launch=dict(median=med, min=v[0], max=v[-1]), launches_per_call=launches[name], stream_bytes_per_launch=per_launch,
                         of_hbm=dict(median=per_launch / (med * 1e-3) / HBM, best=per_launch / (v[0] * 1e-3) / HBM),
                         channel_msps=dict(median=chs / (med * 1e-3) / 1e6, best=chs / (v[0] * 1e-3) / 1e6))
    wide.close()
    shared.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
