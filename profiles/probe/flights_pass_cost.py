"""What the flight table's pass (flight.hip) costs: acg_collect_msgs_oooi per call, lag 2, ACG_F_REPAIR, beside the running
down-converter and demodulator in one process, on the bench's traffic (benchlib/case.py: ACARS/MSK frames of 20-220
characters every 0.25-1 s per channel, AM depth 0.5, 20 dB SNR, decimation 200) -- with the table off (the yardstick: the same
call as before the table existed), with the table on, and with the table on while EVERY channel carries the same aircraft
(one segment of the walk holds all events).  256 distinct tracks are modulated on the host and spread over the channels.

    python profiles/probe/flights_pass_cost.py 1024 16384

Prints per width and case: collects, messages, ms per collect call (mean / median / max), ms per step (a pass over the
batch) and the whole-step rate in channel-samples per second."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from acarsdec_amd import decoder as D, synth as S, _capi as K  # noqa: E402

M, CB, NTRACK = 200, 8, 256
CARRIER, DEPTH, SCALE, SNR_DB = 0.5, 0.5, 0.25, 20.0


def track(rng, nout, hot):
    """synth.channel_audio's traffic (random downlinks, 20-220 characters, a gap of 0.25-1 s); hot: one address for all"""
    out = np.zeros(nout)
    pos = int(rng.integers(800, 3125))
    while True:
        addr = b".HOT001" if hot else b"." + bytes(rng.integers(0x41, 0x5B, size=6).astype(np.uint8).tolist())
        fr = S.acars_frame(text=S.random_text(rng, 20, 220), mode=b"2", addr=addr, label=bytes(rng.integers(0x30, 0x3A, size=2).astype(np.uint8).tolist()),
                           bid=bytes([int(rng.integers(0x30, 0x3A))]))
        a = S.msk_audio(S.frame_bits(fr), phase0=float(rng.uniform(0, 2 * np.pi)))
        if pos + a.size + 64 > nout:
            return out
        out[pos:pos + a.size] = a
        pos += a.size + int(rng.integers(3125, 12500))


def run(nch, nblk, steps, hot, table):
    L = K.load()
    dev = torch.device("cuda:0")
    nout = nblk * 1024
    row = nout * M * 2
    iq = torch.empty((nch, row), dtype=torch.uint8, device=dev)
    trk = np.stack([CARRIER * (1.0 + DEPTH * track(np.random.default_rng(1000 + i), nout, hot)) for i in range(NTRACK)]).astype(np.float32)
    d_trk = torch.from_numpy(trk).to(dev)
    rng = np.random.default_rng(nch)
    off = rng.integers(-48, 49, size=nch) * 25000.0
    off[np.abs(off) < 25000] = 50000.0
    d_idx = (torch.arange(nch, dtype=torch.int32, device=dev) % NTRACK).contiguous()
    d_off = torch.from_numpy(off.astype(np.float32)).to(dev)
    d_ph = torch.from_numpy(rng.uniform(0, 2 * np.pi, nch).astype(np.float32)).to(dev)
    sigma = SCALE * CARRIER * (M / (2.0 * 10 ** (SNR_DB / 10.0))) ** 0.5
    assert L.acg_synth_iq_u8_dev(iq.data_ptr(), row, nch, nout, M, d_trk.data_ptr(), nout, d_idx.data_ptr(), d_off.data_ptr(),
                                 d_ph.data_ptr(), SCALE, sigma, 0xACA25, None) == 0
    torch.cuda.synchronize()
    dec = D.Decoder(nch, decim=M, ntaps=M, max_blocks=CB, bitlog=False, repair=True, max_lag=2)
    tap = {int(o): D.rtl_taps(int(131000000 + o), 131000000, M) for o in set(off.tolist())}
    dec.set_taps(np.stack([tap[int(o)] for o in off]))
    if table:
        dec.enable_flights(t0=1700000000.0, mdly=600, max_flights=65536)
    cap = max(8192, nch * 4)
    mbuf, obuf = (K.Msg * cap)(), (K.Oooi * cap)()
    n = C.c_int(0)
    stream = torch.cuda.current_stream().cuda_stream
    ncall = nblk // CB
    t_call, got = [], 0
    t_step = []
    for s in range(steps + 1):                                  # (the first step is for nothing)
        t0 = time.perf_counter()
        for k in range(ncall):
            part = iq[:, k * CB * 1024 * M * 2:(k + 1) * CB * 1024 * M * 2]
            dec.in_callback(part, nblocks=CB, pitch=row, stream=stream)
            while True:
                a = time.perf_counter()
                rc = L.acg_collect_msgs_oooi(dec.ctx, 2, mbuf, obuf, cap, C.byref(n))
                b = time.perf_counter()
                assert rc in (K.OK, K.EAGAIN), rc
                if s:
                    t_call.append(1e3 * (b - a))
                    got += n.value
                if rc == K.OK:
                    break
        dec.sync()
        if s:
            t_step.append(1e3 * (time.perf_counter() - t0))
    nfl = len(dec.flights()) if table else 0
    nrt = len(dec.drain_routes()) if table else 0
    dec.close()
    tc, ts = np.array(t_call), np.array(t_step)
    print("nch %5d %-9s table %-3s: %4d collects %7d msgs  collect ms mean %.3f median %.3f max %.3f | step ms mean %.2f min %.2f  rate %.3e ch-samples/s"
          "  (flights %d, routes %d)" % (nch, "hot" if hot else "spread", "on" if table else "off", tc.size, got, tc.mean(), np.median(tc), tc.max(),
                                        ts.mean(), ts.min(), nch * nout / (ts.mean() * 1e-3), nfl, nrt), flush=True)


if __name__ == "__main__":
    for w in [int(a) for a in sys.argv[1:]] or [1024]:
        nblk, steps = (32, 6) if w <= 2048 else (8, 12)
        for hot, table in ((False, False), (False, True), (False, False), (False, True), (True, False), (True, True)):
            run(w, nblk, steps, hot, table)
