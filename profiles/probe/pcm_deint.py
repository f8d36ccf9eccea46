"""What the de-interleave kernel (pcm.hip) costs in front of the demodulator, and what the bound soundfile.c costs per read.

    python profiles/probe/pcm_deint.py [pairs]

Kernel: one context per width (16 384 and 1024 channels, 8192 frames per call), both formats, ONE process.  The same noise goes
in as interleaved frames (acg_process_pcm_dev) and as planar floats (acg_process_dm_dev); the two calls alternate, `pairs` pairs
after 3 unrecorded ones, the device synchronised before each call.  Per call:
  events  HIP events around the call on the caller's stream.  The de-interleave kernel runs on that stream and the demodulator
          does not, so for the PCM arm this is the kernel itself; for the planar arm the stream waits for the demodulator, so
          it is the demodulator plus two cross-stream waits.
  wall    host clock from the call to the end of acg_sync: the whole call, either arm.
  msk     acg_get_timing's demodulator time per launch, either arm (the demodulator must not care where dm came from).
Beside them: (bytes read + bytes written) / the rate acg_probe_read_dev measures in this process (the pure reader bench.py
--full reports).

Legacy view: lib/acarsdec_gpu_file (soundfile.c bound: one call per 4096-frame read) beside lib/acarsdec_gpu (demodMSK(): one
per channel and read) on test.wav, ACARSDEC_AMD_STATS=1, three runs each, alternated."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from acarsdec_amd import decoder as D, _capi as K  # noqa: E402

NFRAMES = 8192


def stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def kernel_cost(nch, pairs):
    L = K.load()
    dec = D.Decoder(nch, decim=8, ntaps=8, max_blocks=NFRAMES // 1024, bitlog=False, timing=True)
    dec.set_timing(1)
    g = torch.Generator(device="cuda").manual_seed(nch)
    s16 = torch.randint(-3000, 3000, (NFRAMES, nch), dtype=torch.int16, device="cuda", generator=g)
    f32 = (s16.to(torch.float32) / 32768.0).contiguous()
    planar = f32.t().contiguous()
    gbps = C.c_double(0)
    assert L.acg_probe_read_dev(planar.data_ptr(), planar.numel() * 4, 10, C.byref(gbps)) == K.OK
    out = dict(nch=nch, nframes=NFRAMES, reader_GBs=gbps.value)
    ts = torch.cuda.Stream()                            # the caller's stream of both arms
    for name, fmt, frames in (("s16", K.PCM_S16, s16), ("f32", K.PCM_F32, f32)):
        arms = {"pcm": lambda: dec.process_pcm(frames, fmt, NFRAMES, stream=ts.cuda_stream),
                "planar": lambda: dec._chk(L.acg_process_dm_dev(dec.ctx, planar.data_ptr(), NFRAMES, NFRAMES, ts.cuda_stream))}
        rec = {a: dict(events=[], wall=[], msk=[]) for a in arms}
        for it in range(pairs + 3):
            for a, call in arms.items():
                torch.cuda.synchronize()
                dec.timing()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record(ts)
                call()
                e1.record(ts)
                dec.sync()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t = dec.timing()
                dec.drain_frames_raw()
                if it >= 3:
                    rec[a]["events"].append(e0.elapsed_time(e1))
                    rec[a]["wall"].append(1e3 * (t1 - t0))
                    rec[a]["msk"].append(t["msk_ms"] / max(1, t["msk_launches"]))
        elem = 2 if fmt == K.PCM_S16 else 4
        traffic = NFRAMES * nch * (elem + 4)
        out[name] = dict(bytes=traffic, streaming_ms=1e3 * traffic / (gbps.value * 1e9),
                         **{a: {k: stats(v) for k, v in r.items()} for a, r in rec.items()})
    dec.close()
    return out


def legacy_view():
    old, new = (os.path.join(ROOT, "acarsdec_amd", "lib", n) for n in ("acarsdec_gpu", "acarsdec_gpu_file"))
    if not (os.path.exists(old) and os.path.exists(new)):
        return None
    pcm = np.load(os.path.join(ROOT, "tests", "golden", "testwav_pcm16.npz"))["pcm"]
    out = {"acarsdec_gpu": [], "acarsdec_gpu_file": []}
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "t.wav")
        with wave.open(src, "wb") as wv:
            wv.setnchannels(pcm.shape[1])
            wv.setsampwidth(2)
            wv.setframerate(12500)
            wv.writeframes(np.ascontiguousarray(pcm, dtype="<i2").tobytes())
        for _ in range(3):
            for exe in (old, new):
                r = subprocess.run([exe, "-o", "1", "-f", src], env=dict(os.environ, ACARSDEC_AMD_STATS="1"), capture_output=True, timeout=300)
                m = re.search(r"compat: (\d+) calls, ([0-9.]+) s inside .*first call ([0-9.]+) ms; the others ([0-9.]+) ms per call; context made at initMsk\(\) time in ([0-9.]+) ms",
                              r.stderr.decode("latin-1"))
                calls, secs = int(m.group(1)), float(m.group(2))
                out[os.path.basename(exe)].append(dict(calls=calls, ms_per_call=float(m.group(4)), first_ms=float(m.group(3)),
                                                       ms_per_4096_frame_read=1e3 * secs / 14, context_ms=float(m.group(5))))
    return out


if __name__ == "__main__":
    pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    res = dict(kernel=[kernel_cost(n, pairs) for n in (16384, 1024)], legacy=legacy_view())
    print(json.dumps(res, indent=1))
