"""What byte closes that end a segment, and the short segments behind them, cost the lean demodulator: the kernel alone (bit log on,
nothing running beside it) on three inputs of the same shape,
  (a) traffic as the bench builds it (synth.channel_audio, gap (3125, 12500), text of 20-220 characters, AM depth 0.5, envelope
      noise for 20 dB), a pool of 64 distinct channels so that the eight channels of a wave differ, walked call by call;
  (b) silence (all-zero dm): no sync is ever found, every segment has its 8 periods, no period closes a segment msk.hip's way;
  (c) noise.
A period's arithmetic does not depend on the data, so (a) - (b) is all that tails and short segments cost: the ceiling of any
change to how a close is framed or a period leaves the segment loop (profiles/probe/lean_segment_stats.py counts the events).
python profiles/probe/msk_lean_closes.py [channels] [blocks per call] [calls per window] [rounds]
ACARSDEC_AMD_LIB names the library (profiles/probe/build_ab.py arms); the last line is the three means for a script to pick up."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
import torch
from acarsdec_amd import decoder as D, synth as S, _capi as K

nch = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
nblk = int(sys.argv[2]) if len(sys.argv) > 2 else 8
ncall = int(sys.argv[3]) if len(sys.argv) > 3 else 16
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 3
L = K.load()
n = nblk * 1024
total = n * ncall
POOL = 64
CARRIER, DEPTH, SNR_DB = 0.5, 0.5, 20.0
sigma = CARRIER * 10 ** (-SNR_DB / 20) / 2 ** 0.5
pool = np.empty((POOL, total), dtype=np.float32)
for i in range(POOL):
    rng = np.random.default_rng(0xACA25 + i)
    a, _ = S.channel_audio(rng, total, gap=(3125, 12500), text_len=(20, 220))
    pool[i] = S.envelope(a, depth=DEPTH, carrier=CARRIER, noise=sigma, rng=rng)
idx = torch.arange(nch, device="cuda") % POOL
inputs = {
    "a traffic": torch.from_numpy(pool).cuda()[idx].contiguous(),
    "b silence": torch.zeros((nch, total), dtype=torch.float32, device="cuda"),
    "c noise": torch.from_numpy(np.random.default_rng(7).normal(0.5, 0.2, size=(POOL, total)).astype(np.float32)).cuda()[idx].contiguous(),
}
dec = D.Decoder(nch, decim=8, ntaps=8, max_blocks=nblk, bitlog=True, timing=True)
st = torch.cuda.Stream()
torch.cuda.set_stream(st)
bits = n / 5.2083
res = {k: [] for k in inputs}
for rnd in range(rounds):
    for name, d in inputs.items():
        dec.reset()
        nf = 0
        for w in range(2):                       # the first pass over the track warms up, the second is the window
            dec.timing()
            for c in range(ncall):
                assert L.acg_process_dm_dev(dec.ctx, d.data_ptr() + 4 * c * n, total, n, st.cuda_stream) == 0   # (pitch, len)
                nf += dec.drain_frames_raw(65536)[0]
            tim = dec.timing()
        ms = tim["msk_ms"] / ncall
        res[name].append(ms)
        print("%-9s nch=%d blk=%d: kernel %.4f ms per call (%.3f us/bit/wave), %d launches, %d blocks in two passes" % (
            name, nch, nblk, ms, ms * 1e3 / bits, tim["msk_launches"], nf), flush=True)
m = {k: float(np.mean(v)) for k, v in res.items()}
a, b, c = m["a traffic"], m["b silence"], m["c noise"]
print("windows: " + "; ".join("%s %s" % (k, " ".join("%.4f" % x for x in v)) for k, v in res.items()))
print("means: a %.4f  b %.4f  c %.4f ms per call; a - b = %.4f ms = %.2f %% of a; c - b = %.4f ms = %.2f %% of c" % (
    a, b, c, a - b, 100 * (a - b) / a, c - b, 100 * (c - b) / c))
