"""Golden fixture for the JSON sink (buildjson(), acarsdec -o 4): a synthetic 3-channel 12.5 kHz recording of synth.message_zoo
traffic plus scripted transmissions that decide BYTES of a line -- a text holding '"', '\\', each of \\b \\f \\n \\r \\t, 0x01, 0x1f
and a NUL in its middle; a text that starts with NUL; a quote and a control character inside the address, the flight id, the
message number and the label; the mode '"' and the mode NUL; NAK and a '"' acknowledgement; a NUL block id; a label with DEL as its
second character; ETB; uplinks; downlinks shorter than 4 and shorter than 10 characters; labels DecodeLabel() decodes (texts from the
labels fixture's generator), one of them with a control character inside an airport field.  Text bodies avoid 0x03, 0x17 and 0x7f:
they end the block.

The recording is played through the UNMODIFIED reference program (oracle/_ref/acarsdec_cpu -o 4 -i STN1 [-A] [-e] [-b LIST]
-f <wav>) once per filter variant, and the lines it prints are kept exactly as printed, wall-clock time stamps included.  The
carrier phases of transmissions the reference loses are drawn again until it decodes every one (asserted: no case is silently
absent).  Run in the build container only:

    python tests/golden/make_msgjson_golden.py

Outputs (derived data, no reference source):
  msgjson_pcm16.npz     the recording as int16 [3, n]
  msgjson_golden.json   {"station", "label_list", "nch", "sent": the transmissions (chn, what, frame fields as hex),
                         "variants": {name: {"args": [...], "lines": the reference's stdout lines}}}
"""
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
sys.path.insert(0, HERE)
from acarsdec_amd import synth as S  # noqa: E402
import label_model as LM  # noqa: E402
import make_label_golden as LG  # noqa: E402

NCH = 3
STATION = "STN1"
LABEL_LIST = "Q1:44:26:H1:Qd:10:QA:\"\x04"
VARIANTS = {"none": [], "A": ["-A"], "e": ["-e"], "b": ["-b", LABEL_LIST], "Aeb": ["-A", "-e", "-b", LABEL_LIST]}
DOWN = b"M01AXY0123"                                       # message number (4) + flight id (6) of a downlink


def tx(what, text=b"", mode=b"2", addr=b".N12345", ack=b"\x15", label=b"H1", bid=b"3", etb=False):
    return dict(what=what, text=text, mode=mode, addr=addr, ack=ack, label=label, bid=bid, etb=etb)


def scripted(rng):
    out = [
        tx("every escape class in a text", DOWN + b'A"B\\C\bD\fE\nF\rG\tH\x01I\x1fJ\x00KLM'),
        tx("every escape class in an uplink text", b'\x1f\x01"\\\b\f\n\r\t tail \x00 hidden', bid=b"A"),
        tx("text starts with NUL", b"\x00HIDDEN", bid=b"B"),
        tx("downlink text starts with NUL", DOWN + b"\x00HIDDEN", bid=b"4"),
        tx("quote and control in addr, fid, msgno, label", b'M\x02"A' + b'X"\x1fY12' + b"BODY", addr=b'.N"1\x0145', label=b'"\x04', bid=b"5"),
        tx("backslash in addr and label", b"UP", addr=b"..\\AB\tC", label=b"\\\n", bid=b"C"),
        tx('mode is a quote', b"MODE", mode=b'"', bid=b"D"),
        tx("mode is NUL", b"MODE0", mode=b"\x00", bid=b"E"),
        tx("mode is a control character", DOWN + b"MODE1", mode=b"\x1b", bid=b"6"),
        tx("NAK", b"NAK", ack=b"\x15", bid=b"F"),
        tx("letter acknowledgement", b"ACK", ack=b"K", bid=b"G"),
        tx('acknowledgement is a quote', DOWN + b"ACKQ", ack=b'"', bid=b"7"),
        tx("acknowledgement is a control character", b"ACKC", ack=b"\x06", bid=b"H"),
        tx("block id is NUL", b"NOBID", bid=b"\x00"),
        tx("block id is a quote", b"QBID", bid=b'"'),
        tx("block id is a control character", b"CBID", bid=b"\x08"),
        tx("label ends in DEL", b"DEL LABEL", label=b"Q\x7f", bid=b"J"),
        tx("label ends in DEL, downlink", DOWN + b"DEL LABEL", label=b"Q\x7f", bid=b"8"),
        tx("one-character label", b"SHORT LABEL", label=b"5\x00", bid=b"K"),
        tx("ETB", b"FIRST PART", bid=b"L", etb=True),
        tx("ETB downlink", DOWN + b"FIRST PART", bid=b"9", etb=True),
        tx("empty uplink", b"", bid=b"M"),
        tx("empty downlink", b"", bid=b"0"),
        tx("empty ETB block", b"", bid=b"N", etb=True),
        tx("downlink shorter than 4", b"M0", bid=b"1"),
        tx("downlink of exactly 4", b"M012", bid=b"2"),
        tx("downlink shorter than 10", b"M01AXY0", bid=b"3"),
        tx("downlink of exactly 10", DOWN, bid=b"4"),
        tx("control character inside an airport field", DOWN + b"KJ\x05K0815", label=b"QA", bid=b"5"),
        tx("quote inside an airport field", DOWN + b'LF"GEG\\L0930', label=b"QP", bid=b"6"),
        tx("NUL inside an airport field", DOWN + b"AB\x00DXXXXEHAMZZZZKBOS", label=b"QL", bid=b"7"),
        tx("long text", DOWN + S.random_text(rng, 205, 205), bid=b"8"),
        tx("long text of control characters", bytes([1 + i % 2 + 3 * (i % 7 == 0) for i in range(215)]), bid=b"P"),
    ]
    # labels DecodeLabel() decodes, as downlinks and one uplink: the texts the labels fixture is built from
    want = ("Q1", "44", "10", "QT", "17", "8D", "QN")
    seen = set()
    for lbl, text, what in LG.table_cases(rng) + LG.label26_cases(rng):
        if what in ("ok", "ok:prefix") and lbl in want + ("26",) and (lbl, what) not in seen:
            seen.add((lbl, what))
            i = len(seen)
            out.append(tx("label %s decodes (%s)" % (lbl, what), DOWN + text, label=lbl.encode(), bid=bytes([0x30 + i % 10])))
    out.append(tx("label Q1 decodes, uplink", b"KJFK0800081209450950XXXXEGLL", label=b"Q1", bid=b"Q"))
    out.append(tx("label 12 fails its check", DOWN + b"KJFKXEGLLREST", label=b"12", bid=b"1"))
    return out


def transmissions(rng, nzoo=24):
    zoo = []
    for fr in S.message_zoo(rng, nzoo):
        zoo.append(dict(what="zoo", frame=fr))
    sc = [dict(what=t["what"], frame=S.acars_frame(text=t["text"], mode=t["mode"], addr=t["addr"], ack=t["ack"], label=t["label"], bid=t["bid"],
                                                   etb=t["etb"])) for t in scripted(rng)]
    allt = zoo + sc
    order = rng.permutation(len(allt))
    return [allt[i] for i in order]


def frame_key(frame):
    """(label, block id, text) as the reference's JSON shows them, from the transmission's bytes (parity stripped)"""
    b = bytes(x & 0x7F for x in frame[5:-3])                # mode .. ETX / ETB
    label = LM.label_str(bytes([b[9], 0x64 if b[10] == 0x7F else b[10]]))
    bid = b[11:12]
    body = b[13:-1] if b[12] == 0x02 else b""
    if b"0" <= bid <= b"9":
        body = body[10:]
    c = lambda v: v.split(b"\0")[0].decode("latin1")
    return (c(label), c(bid), c(body))


def json_key(j):
    return (j["label"], j.get("block_id", ""), j.get("text", ""))


def lay_out(txs, chans, phases, gaps, lead=2500):
    audio = [S.msk_audio(S.frame_bits(t["frame"]), phase0=float(p)) for t, p in zip(txs, phases)]
    at = [lead] * NCH
    starts = []
    for a, c, g in zip(audio, chans, gaps):
        starts.append(at[c])
        at[c] += a.size + int(g)
    n = max(at) + 4000
    n += (-n) % 4096
    x = np.zeros((NCH, n))
    for a, c, s in zip(audio, chans, starts):
        x[c, s:s + a.size] = a
    return np.rint(np.clip(0.5 * x, -1, 1) * 4000).astype(np.int16)


def reference_lines(pcm, args):
    exe = os.path.join(ROOT, "oracle", "_ref", "acarsdec_cpu")
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "msgjson.wav")
        with wave.open(p, "wb") as w:
            w.setnchannels(NCH)
            w.setsampwidth(2)
            w.setframerate(12500)
            w.writeframes(np.ascontiguousarray(pcm.T).tobytes())
        r = subprocess.run([exe, "-o", "4", "-i", STATION] + args + ["-f", p], capture_output=True)
    return [ln for ln in r.stdout.split(b"\n") if ln.startswith(b"{")]


def make_recording(seed=20261018, rounds=16):
    rng = np.random.default_rng(seed)
    txs = transmissions(rng)
    chans = [i % NCH for i in range(len(txs))]
    phases = rng.uniform(0, 2 * np.pi, len(txs))
    gaps = rng.integers(900, 1500, len(txs))
    for _ in range(rounds):
        pcm = lay_out(txs, chans, phases, gaps)
        got = [json.loads(ln.decode("latin1")) for ln in reference_lines(pcm, [])]
        missing = []
        for c in range(NCH):
            mine = [json_key(j) for j in got if j["channel"] == c]
            k = 0
            for i, t in enumerate(txs):
                if chans[i] != c:
                    continue
                if k < len(mine) and mine[k] == frame_key(t["frame"]):
                    k += 1
                else:
                    missing.append(i)
        if not missing:
            return txs, chans, pcm
        phases[missing] = rng.uniform(0, 2 * np.pi, len(missing))
    raise RuntimeError("transmissions %s never decoded" % missing)


if __name__ == "__main__":
    txs, chans, pcm = make_recording()
    variants = {}
    for name, args in VARIANTS.items():
        lines = reference_lines(pcm, args)
        variants[name] = dict(args=args, lines=[ln.decode("ascii") for ln in lines])
    n = {k: len(v["lines"]) for k, v in variants.items()}
    assert n["none"] == len(txs), (n, len(txs))             # every transmission is there
    assert n["none"] > n["A"] > n["Aeb"] > 0 and n["none"] > n["e"] and n["none"] > n["b"] > n["Aeb"], n
    np.savez_compressed(os.path.join(HERE, "msgjson_pcm16.npz"), pcm=pcm)
    sent = [dict(chn=c, what=t["what"], frame=t["frame"].hex()) for t, c in zip(txs, chans)]
    with open(os.path.join(HERE, "msgjson_golden.json"), "w") as f:
        json.dump(dict(station=STATION, label_list=LABEL_LIST, nch=NCH, sent=sent, variants=variants), f, indent=0)
    print("wrote %d transmissions, %d samples per channel; lines per variant: %s" % (len(txs), pcm.shape[1], n))
