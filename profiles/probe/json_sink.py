"""What the JSON sink (json.hip) costs at the headline shape: 1024 channels x 8 callbacks per call, ACG_F_REPAIR, lag 2, beside
the running down-converter and demodulator in one process, on the bench's traffic (benchlib/case.py: ACARS/MSK frames of 20-220
characters every 0.25-1 s per channel, AM depth 0.5, 20 dB SNR, decimation 200).  ONE context with the sink enabled; the calls
are collected alternately, K with acg_collect_msgs_oooi (the yardstick: records and decoded labels cross to the host) and K
with acg_collect_json (only the packed lines cross).

    python profiles/probe/json_sink.py [nch [K]]

Prints per arm: collects, messages / lines, ms per collect call (mean / median / max), ms per process + collect call, lines and
bytes per second of wall time; then the same two entry points on an IDLE device (everything synchronised first, the same number
of calls queued): their difference is the device and launch time the JSON passes add to a round trip when nothing hides it."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from acarsdec_amd import decoder as D, synth as S, _capi as K  # noqa: E402

M, CB, NTRACK, NBLK = 200, 8, 128, 32
CARRIER, DEPTH, SCALE, SNR_DB = 0.5, 0.5, 0.25, 20.0


def track(rng, nout):
    out = np.zeros(nout)
    pos = int(rng.integers(800, 3125))
    while True:
        fr = S.acars_frame(text=S.random_text(rng, 20, 220), mode=b"2", addr=b"." + bytes(rng.integers(0x41, 0x5B, size=6).astype(np.uint8).tolist()),
                           label=bytes(rng.integers(0x30, 0x3A, size=2).astype(np.uint8).tolist()), bid=bytes([int(rng.integers(0x30, 0x3A))]))
        a = S.msk_audio(S.frame_bits(fr), phase0=float(rng.uniform(0, 2 * np.pi)))
        if pos + a.size + 64 > nout:
            return out
        out[pos:pos + a.size] = a
        pos += a.size + int(rng.integers(3125, 12500))


def main(nch, kalt, steps=6):
    L = K.load()
    dev = torch.device("cuda:0")
    nout = NBLK * 1024
    row = nout * M * 2
    iq = torch.empty((nch, row), dtype=torch.uint8, device=dev)
    trk = np.stack([CARRIER * (1.0 + DEPTH * track(np.random.default_rng(1000 + i), nout)) for i in range(NTRACK)]).astype(np.float32)
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
    dec.enable_json((1700000000, 0), "STN1", "acarsdec", "3.7", freqs_hz=[int(131000000 + o) for o in off])
    cap = max(8192, nch * 4)
    mbuf, obuf = (K.Msg * cap)(), (K.Oooi * cap)()
    jbuf = C.create_string_buffer(cap * K.JSON_LINE_MAX)
    n, nb = C.c_int(0), C.c_size_t(0)
    stream = torch.cuda.current_stream().cuda_stream
    ncall = NBLK // CB

    def collect(arm, lag):
        """one collect through the arm's entry point: (ms, messages, bytes)"""
        got = nbytes = 0
        a = time.perf_counter()
        while True:
            if arm == "json":
                rc = L.acg_collect_json(dec.ctx, lag, jbuf, len(jbuf), C.byref(nb), C.byref(n))
                nbytes += nb.value
            else:
                rc = L.acg_collect_msgs_oooi(dec.ctx, lag, mbuf, obuf, cap, C.byref(n))
            assert rc in (K.OK, K.EAGAIN), rc
            got += n.value
            if rc == K.OK:
                return 1e3 * (time.perf_counter() - a), got, nbytes

    stat = {"oooi": dict(ms=[], call=[], msgs=0, bytes=0), "json": dict(ms=[], call=[], msgs=0, bytes=0)}
    seq = 0
    for s in range(steps + 1):                                  # (the first step is for nothing)
        for k in range(ncall):
            arm = "json" if (seq // kalt) % 2 else "oooi"
            seq += 1
            t0 = time.perf_counter()
            part = iq[:, k * CB * 1024 * M * 2:(k + 1) * CB * 1024 * M * 2]
            dec.in_callback(part, nblocks=CB, pitch=row, stream=stream)
            ms, got, nbytes = collect(arm, 2)
            if s:
                st = stat[arm]
                st["ms"].append(ms)
                st["call"].append(1e3 * (time.perf_counter() - t0))
                st["msgs"] += got
                st["bytes"] += nbytes
    dec.sync()
    for arm in ("oooi", "json"):
        st = stat[arm]
        ms, call = np.array(st["ms"]), np.array(st["call"])
        wall = call.sum() * 1e-3
        print("nch %5d %-4s: %4d collects %7d msgs  collect ms mean %.3f median %.3f max %.3f | process + collect ms mean %.3f median %.3f | "
              "%.0f msgs/s %.3e bytes/s" % (nch, arm, ms.size, st["msgs"], ms.mean(), np.median(ms), ms.max(), call.mean(), np.median(call),
                                          st["msgs"] / wall, st["bytes"] / wall), flush=True)
    # ---- idle device: the same queue content through either entry point, nothing to hide behind
    idle = {"oooi": [], "json": []}
    counts = {"oooi": 0, "json": 0}
    for rep in range(2 * 6 + 2):
        arm = "json" if rep % 2 else "oooi"
        dec.reset()
        for k in range(2):
            part = iq[:, k * CB * 1024 * M * 2:(k + 1) * CB * 1024 * M * 2]
            dec.in_callback(part, nblocks=CB, pitch=row, stream=stream)
        dec.sync()
        ms, got, _ = collect(arm, 0)
        if rep >= 2:
            idle[arm].append(ms)
            counts[arm] = got
    print("nch %5d idle device, 2 calls queued: acg_collect_msgs_oooi %.3f ms (%d msgs), acg_collect_json %.3f ms (%d lines): +%.3f ms" % (
        nch, np.median(idle["oooi"]), counts["oooi"], np.median(idle["json"]), counts["json"], np.median(idle["json"]) - np.median(idle["oooi"])), flush=True)
    dec.close()


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:]]
    main(args[0] if args else 1024, args[1] if len(args) > 1 else 4)
