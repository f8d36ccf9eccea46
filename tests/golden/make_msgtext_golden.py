"""Golden fixture for the text sink (printoneline() -o 1, printmsg() -o 2): the JSON fixture's recording (msgjson_pcm16.npz: NUL,
control characters, quotes, short downlinks, ETB, empty texts, decoded labels) played through the UNMODIFIED reference program
(oracle/_ref/acarsdec_cpu -o 1 / -o 2 [-A] [-e] [-b LIST] -f <wav>) once per filter variant of msgjson_golden.json, stdout kept
byte for byte (as hex).  Every run must yield as many records as the JSON fixture's variant has lines (asserted).

The sound-file front end prints neither the date nor printmsg()'s "F:" token.  For those one more leg: the first RTL_BLOCKS
blocks of the same recording (three channels, a fourth silent) up-converted onto four carriers of one 2.0 Msps stream the way
make_golden.py makes its own, played through oracle/_ref/acarsdec_cpu_rtl -o 2 -r 0 (rtl.c and a file-playing dongle).  The I/Q is
not kept: a test regenerates it from the committed recording (iq_sha256 says whether it got the same bytes).  The reference stamps
its wall clock, so the date's digits are replaced by a placeholder of the same shape.  Run in the build container only:

    python tests/golden/make_msgtext_golden.py

Output (derived data, no reference source):
  msgtext_golden.json   {"variants": {name: {"args", "o1": hex, "o2": hex, "records": n}},
                         "rtl": {"args", "freqs", "M", "Fc", "phases", "blocks", "tail_blocks", "iq_sha256", "o2_masked": hex, "records": n}}
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from acarsdec_amd import decoder as D, synth as S  # noqa: E402
import text_model as TM  # noqa: E402

RTL_FREQS = ["131.525", "131.725", "131.825", "131.550"]
RTL_PHASES = [0.1, 1.0, 2.0, 3.0]
RTL_M = 160
RTL_BLOCKS = 40
RTL_TAIL = 4


def rtl_iq(pcm, blocks=RTL_BLOCKS, tail=RTL_TAIL, freqs=RTL_FREQS, M=RTL_M, phases=RTL_PHASES):
    """(iq, Fc, Fr): the recording's first `blocks` blocks on the carriers, `tail` blocks of bare carrier behind them"""
    fr = [D.parse_freq_mhz(f) for f in freqs]
    fc, _ = D.choose_fc(fr, M)
    x = pcm[:, :blocks * 1024].astype(np.float32) / np.float32(32768.0)
    env = np.full((len(freqs), (blocks + tail) * 1024), 0.5)
    env[:x.shape[0], :x.shape[1]] = 0.5 + 0.5 * x.astype(np.float64)
    return S.iq_u8_from_envelopes(env, M, [f - fc for f in fr], phases=phases), fc, fr


def run_wav(pcm, args):
    exe = os.path.join(ROOT, "oracle", "_ref", "acarsdec_cpu")
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "msgtext.wav")
        with wave.open(p, "wb") as w:
            w.setnchannels(pcm.shape[0])
            w.setsampwidth(2)
            w.setframerate(12500)
            w.writeframes(np.ascontiguousarray(pcm.T).tobytes())
        r = subprocess.run([exe] + args + ["-f", p], capture_output=True)
    return r.stdout                                           # (the program ends with "exiting ..." and a non-zero status at the file's end)


if __name__ == "__main__":
    pcm = np.load(os.path.join(HERE, "msgjson_pcm16.npz"))["pcm"]
    with open(os.path.join(HERE, "msgjson_golden.json")) as f:
        gj = json.load(f)
    variants = {}
    for name, v in gj["variants"].items():
        o1, o2 = run_wav(pcm, ["-o", "1"] + v["args"]), run_wav(pcm, ["-o", "2"] + v["args"])
        n = len(v["lines"])
        assert len(TM.split_oneline(o1)) == n and len(TM.split_std(o2)) == n, (name, n, len(TM.split_oneline(o1)), len(TM.split_std(o2)))
        assert b"".join(TM.split_oneline(o1)) == o1 and b"".join(TM.split_std(o2)) == o2          # nothing but records
        variants[name] = dict(args=v["args"], o1=o1.hex(), o2=o2.hex(), records=n)
    iq, fc, fr = rtl_iq(pcm)
    with tempfile.NamedTemporaryFile(suffix=".iq", delete=False) as f:
        f.write(iq.tobytes())
        path = f.name
    args = ["-o", "2", "-r", "0"] + RTL_FREQS
    r = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "acarsdec_cpu_rtl")] + args, env=dict(os.environ, ACARSDEC_IQ_FILE=path), capture_output=True)
    os.unlink(path)
    masked = TM.mask_dates(r.stdout)
    recs = TM.split_std(masked)
    assert b"".join(recs) == masked and len(recs) >= 6 and all(TM.DATE_MASK in x and b"(F:131." in x for x in recs), len(recs)
    rtl = dict(args=args, freqs=RTL_FREQS, M=RTL_M, Fc=int(fc), phases=RTL_PHASES, blocks=RTL_BLOCKS, tail_blocks=RTL_TAIL,
               iq_sha256=hashlib.sha256(iq.tobytes()).hexdigest(), o2_masked=masked.hex(), records=len(recs))
    with open(os.path.join(HERE, "msgtext_golden.json"), "w") as f:
        json.dump(dict(variants=variants, rtl=rtl), f, indent=0)
    print("records per variant: %s; rtl leg: %d" % ({k: v["records"] for k, v in variants.items()}, len(recs)))
