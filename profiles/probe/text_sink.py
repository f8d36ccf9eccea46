"""What the text sink's passes (text.hip) cost on the device, next to the JSON sink's (json.hip) over the SAME records in the same
run: acg_lab_time_sink_passes brackets each renderer's launches (keys, sort, measure, two scan launches, render) with HIP events
on an otherwise idle device, warm-up rounds first, the two arms alternated within every round.  Two record sets:

  fixture   the records of tests/golden/msgjson_pcm16.npz (3 channels, 68 messages) as acg_drain_msgs hands them out;
  1024ch    the records one drain hands out after two calls of 1024 channels of synthetic traffic (8 frames of 5-40 characters
            per track, varied amplitude).

    python profiles/probe/text_sink.py [reps]

Prints one line per record set and text format: records, median / min / max ms of the JSON passes and of the text passes."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from acarsdec_amd import decoder as D, synth as S, _capi as K  # noqa: E402

CHUNK = 4096
T0 = (1792301725, 269667)


def drain_all(x, nch):
    dec = D.Decoder(nch, decim=8, ntaps=8, max_blocks=CHUNK // 1024, repair=True, bitlog=False)
    out = []
    for s in range(0, x.shape[1], CHUNK):
        dec.demod_msk(x[:, s:s + CHUNK])
        out += dec.drain_msgs(max_msgs=8192)
    dec.close()
    return out


def wide(nch=1024, nsamp=2 * CHUNK):
    rng = np.random.default_rng(3)
    audio, frames = S.channel_audio(rng, 40000, nframes=8, gap=(600, 900), text_len=(5, 40))
    on = np.flatnonzero(np.abs(audio) > 0)
    cuts = np.flatnonzero(np.diff(on) > 300)
    pieces = [audio[on[a]:on[b] + 1].astype(np.float32) for a, b in zip(np.r_[0, cuts + 1], np.r_[cuts, on.size - 1])]
    y = np.zeros((nch, nsamp), dtype=np.float32)
    for c in range(nch):
        t = int(rng.integers(200, 1200))
        while True:
            a = pieces[rng.integers(0, len(pieces))]
            if t + a.size >= nsamp - 200:
                break
            y[c, t:t + a.size] = a * np.float32(rng.uniform(0.01, 0.9))
            t += a.size + int(rng.integers(500, 1200))
    return y


def main(reps):
    L = K.load()
    pcm = np.load(os.path.join(ROOT, "tests", "golden", "msgjson_pcm16.npz"))["pcm"]
    sets = [("fixture", 3, drain_all(pcm.astype(np.float32) / np.float32(32768.0), 3)), ("1024ch", 1024, drain_all(wide(), 1024))]
    jcfg = D.json_config(T0, "STN1", "acarsdec", "3.7")
    for name, nch, msgs in sets:
        n = len(msgs)
        buf = (K.Msg * n)(*msgs)
        for fmt, kw in (("oneline", dict(date=True)), ("std", dict(date=True, freq=True)), ("pp", {}), ("sv", {})):
            tcfg = D.text_config(fmt, T0, station_id="STN1", **kw)
            ms = np.zeros(2 * reps, dtype=np.float32)
            rc = L.acg_lab_time_sink_passes(buf, n, C.byref(jcfg), C.byref(tcfg), nch, 5, reps, ms.ctypes.data)
            assert rc == K.OK, rc
            j, t = ms[:reps], ms[reps:]
            print("%-8s %5d records %-8s JSON passes median %.4f ms (min %.4f max %.4f) | text passes median %.4f ms (min %.4f max %.4f)" % (
                name, n, fmt, np.median(j), j.min(), j.max(), np.median(t), t.min(), t.max()), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 30)
