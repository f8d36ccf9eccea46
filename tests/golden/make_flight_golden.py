"""Golden fixture for the flight table (addFlight() / routejson(), acarsdec -o 3 and -o 5): a synthetic 3-channel 12.5 kHz
recording of about 120 transmissions from 25 aircraft, spread over the channels, in which departure and destination arrive in
different messages, later messages overwrite fields, decodes fail, flight ids are empty (a downlink text shorter than 4
characters) or change, downlinks consist of an ETX only, uplinks lie in between, a message whose text starts with NUL completes
a route (so -e defers the emission), and labels lie inside and outside the -b list.  Field values are plain alphanumerics.

ORDER.  Completions are more than 4096 samples apart (asserted from the oracle's end_sample values), so at most one block
completes in any 4096-frame chunk the reference reads from the file: its buffer-wise, channel-major order and the real-time
order (end_sample, chn) are the same order, and the comparison with the reference program is exact.

The recording is played through the UNMODIFIED reference program (oracle/_ref/acarsdec_cpu -o 3 | -o 5 [-A] [-e] [-b LIST]
-f <wav>) once per filter variant and output mode.  In file mode the reference stamps the wall clock, so times (and expiry) do
not come from it.  Run in the build container only:

    python tests/golden/make_flight_golden.py

Outputs (derived data, no reference source):
  flights_pcm16.npz     the recording as int16 [3, n]
  flights_golden.json   {"label_list", "sent": the transmissions (addr, label, bid, text as hex, chn, end_sample, soh_sample),
                         "rows": the distinct monitor rows [addr, fid, nbm, mask, DEP, ARR, ETA], "variants": {name: {"args",
                         "frames": per printed monitor frame the indices of its rows, "routes": the route lines without
                         timestamp and station_id}}}
"""
import json
import os
import subprocess
import sys
import tempfile
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from acarsdec_amd import synth as S  # noqa: E402
import flight_model as FM  # noqa: E402
import label_model as LM  # noqa: E402
import oracle as O  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
NCH = 3
LABEL_LIST = "QA:QN:QP:12:H1:QE"                            # QM, 2Z, 5Z stay outside
VARIANTS = {"none": [], "A": ["-A"], "e": ["-e"], "b": ["-b", LABEL_LIST], "Aeb": ["-A", "-e", "-b", LABEL_LIST]}
AIRPORTS = [b"KJFK", b"EGLL", b"LFPG", b"EDDF", b"KBOS", b"LEMD", b"EHAM", b"LIRF"]


def transmissions(rng, n=112, naircraft=25):
    """(addr, label, bid, text) in time order: random traffic, then the scripted cases worked in"""
    ap = lambda: AIRPORTS[int(rng.integers(0, len(AIRPORTS)))]
    hhmm = lambda: b"%04d" % int(rng.integers(0, 2400))
    fids = {a: b"XY%04d" % (100 + a) for a in range(naircraft)}
    out = []
    for i in range(n):
        a = int(rng.integers(0, naircraft))
        addr = b".N%05d" % (700 + a)
        r = rng.random()
        if r < 0.12:                                                    # uplinks in between
            out.append((addr, b"H1", b"A", b"UPLINK %d" % i))
            continue
        if r < 0.16:                                                    # a downlink that is an ETX only
            out.append((addr, b"QA", b"3", b""))
            continue
        if r < 0.21:                                                    # text shorter than 4 characters: no flight id, no text
            out.append((addr, b"H1", b"4", b"M0%d" % (i % 10)))
            continue
        if rng.random() < 0.08:                                         # the flight id changes
            fids[a] = b"ZW%04d" % int(rng.integers(0, 1000))
        lab = [b"QA", b"QN", b"QP", b"QM", b"12", b"2Z", b"H1", b"QE"][int(rng.integers(0, 8))]
        body = {b"QA": lambda: ap() + hhmm(),                           # sa, gout
                b"QN": lambda: b"XXXX" + ap() + hhmm(),                 # da, eta
                b"QP": lambda: ap() + ap() + hhmm(),                    # sa, da, gout
                b"QM": lambda: ap() + b"ABCD" + ap(),                   # da, sa (outside the -b list)
                b"12": lambda: ap() + (b"," if rng.random() < 0.6 else b"X") + ap() + b"REST",     # sa, da -- or a failed decode
                b"2Z": lambda: ap(),                                    # da (outside the -b list)
                b"H1": lambda: b"FREE TEXT %d" % i,
                b"QE": lambda: ap() + hhmm() + ap()}[lab]()             # sa, gout, da
        out.append((addr, lab, bytes([0x30 + i % 10]), b"M%02dA" % (i % 100) + fids[a] + body))
    # the scripted case: N00999 learns sa, then a message whose text starts with NUL brings da (under -e it updates the entry but
    # emits nothing), then a plain message (under -e the route comes out here)
    k = n // 3
    out[k:k] = [(b".N00999", b"QA", b"1", b"M90AXY0999" + b"LIRF" + b"0815")]
    out[k + 7:k + 7] = [(b".N00999", b"QN", b"2", b"M91AXY0999" + b"\x00XXXEHAM0955")]
    out[k + 15:k + 15] = [(b".N00999", b"H1", b"3", b"M92AXY0999" + b"LATER")]
    return out


def reference(pcm, mode, args):
    exe = os.path.join(ROOT, "oracle", "_ref", "acarsdec_cpu")
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "flights.wav")
        with wave.open(p, "wb") as w:
            w.setnchannels(NCH)
            w.setsampwidth(2)
            w.setframerate(12500)
            w.writeframes(np.ascontiguousarray(pcm.T).tobytes())
        r = subprocess.run([exe, "-o", str(mode)] + args + ["-f", p], capture_output=True)
    return r.stdout.decode("latin1")


def monitor_frames(text):
    """every frame printmonitor() printed (output.c:458-484) as rows [addr, fid, nbm, mask, DEP, ARR, ETA]"""
    frames = []
    for part in text.split("\x1b[H\x1b[2J")[1:]:
        if "Acarsdec monitor" not in part:                  # (the screen is also cleared once at start-up)
            continue
        rows = []
        for line in part.split("\n")[2:]:
            if len(line) < 69:
                continue
            rows.append([line[1:9].strip(), line[10:17].strip(), int(line[18:21]), line[22:22 + NCH], line[51:57].strip(),
                         line[57:63].strip(), line[63:69].strip()])
        frames.append(rows)
    return frames


def route_lines(text):
    out = []
    for line in text.splitlines():
        if line.startswith("{"):
            j = json.loads(line)
            out.append(dict(flight=j["flight"], depa=j["depa"], dsta=j["dsta"]))
    return out


def json_keys(text):
    out = []
    for line in text.splitlines():
        if line.startswith("{"):
            j = json.loads(line)
            out.append((j["channel"], j["label"], j.get("tail"), j.get("block_id"), j.get("text", "")))
    return out


def sent_key(t, chn):
    addr, lab, bid, text = t
    body = text[10:] if (b"0" <= bid <= b"9" and text) else text
    return (chn, lab.decode(), addr.replace(b".", b"").decode(), bid.decode(), body.split(b"\0")[0].decode("latin1"))


def lay_out(tx, chans, phases, lead=3000, apart=4700):
    """the recording: transmission i on channel chans[i], each COMPLETING at least `apart` samples after the one before"""
    audio = [S.msk_audio(S.frame_bits(S.acars_frame(text=t[3], addr=t[0], label=t[1], bid=t[2])), phase0=float(p)) for t, p in zip(tx, phases)]
    starts, prev_end, last_end = [], lead, [0] * NCH
    for a, c in zip(audio, chans):
        s = max(prev_end + apart - a.size, last_end[c] + 900)
        starts.append(s)
        prev_end = max(prev_end + apart, s + a.size)
        last_end[c] = s + a.size
    n = prev_end + 5000
    n += (-n) % 4096
    x = np.zeros((NCH, n))
    for a, c, s in zip(audio, chans, starts):
        x[c, s:s + a.size] = a
    return np.rint(np.clip(0.5 * x, -1, 1) * 4000).astype(np.int16)


def make_recording(seed=20261017, rounds=12):
    rng = np.random.default_rng(seed)
    tx = transmissions(rng)
    chans = [int(c) for c in rng.integers(0, NCH, len(tx))]
    phases = rng.uniform(0, 2 * np.pi, len(tx))
    for _ in range(rounds):
        pcm = lay_out(tx, chans, phases)
        got = json_keys(reference(pcm, 4, []))
        missing, k = [], 0
        for i, t in enumerate(tx):
            if k < len(got) and got[k] == sent_key(t, chans[i]):
                k += 1
            else:
                missing.append(i)
        if not missing:
            return tx, chans, pcm
        phases[missing] = rng.uniform(0, 2 * np.pi, len(missing))
    raise RuntimeError("transmissions %s never decoded" % missing)


def oracle_blocks(pcm):
    """(end_sample, soh_sample, chn) of every block, from the oracle's restatement of the demodulator, in time order"""
    out = []
    for c in range(NCH):
        ch = O.Channel(c, max_frames=1024)
        x = pcm[c].astype(np.float32) / 32768.0
        for s in range(0, x.size, 4096):
            ch.demod(x[s:s + 4096])
        out += [(int(f.end_sample), int(f.soh_sample), c) for f in ch.frames]
    return sorted(out)


def model(sent, args):
    """the list walk over the sent transmissions: (frames, routes) as the reference prints them"""
    kw = dict(downlink_only="-A" in args, skip_empty="-e" in args, labels=LM.parse_label_filter(LABEL_LIST) if "-b" in args else ())
    walk, frames = FM.ListWalk(600), []
    for s in sent:
        m = FM.record_of(bytes.fromhex(s["addr"]), bytes.fromhex(s["label"]), s["bid"].encode(), bytes.fromhex(s["text"]), s["chn"],
                         s["end_sample"], s["soh_sample"])
        ev = FM.event_of(m, (0, 0), **kw)
        if ev is not None:
            walk.add(ev)
        if LM.keep(m.down, m.label, m.txt, m.txt_len, **kw):
            frames.append([FM.monitor_row(f, NCH) for f in walk.entries()])
    routes = [dict(flight=r["fid"].split(b"\0")[0].decode(), depa=r["sa"].decode(), dsta=r["da"].decode()) for r in walk.routes]
    return frames, routes


if __name__ == "__main__":
    tx, chans, pcm = make_recording()
    blocks = oracle_blocks(pcm)
    assert len(blocks) == len(tx) and [b[2] for b in blocks] == chans, (len(blocks), len(tx))
    gaps = np.diff([b[0] for b in blocks])
    assert gaps.min() > 4096, gaps.min()                    # the ordering condition
    assert len({b[0] // 4096 for b in blocks}) == len(blocks)
    sent = [dict(addr=t[0].hex(), label=t[1].hex(), bid=t[2].decode(), text=t[3].hex(), chn=c, end_sample=b[0], soh_sample=b[1])
            for t, c, b in zip(tx, chans, blocks)]
    rows, index, variants = [], {}, {}
    for name, args in VARIANTS.items():
        frames = monitor_frames(reference(pcm, 3, args))
        routes = route_lines(reference(pcm, 5, args))
        mf, mr = model(sent, args)
        assert frames == mf, (name, next(i for i in range(min(len(frames), len(mf))) if frames[i] != mf[i]) if frames and mf else None, len(frames), len(mf))
        assert routes == mr, (name, routes, mr)
        enc = []
        for fr in frames:
            ids = []
            for r in fr:
                key = json.dumps(r)
                if key not in index:
                    index[key] = len(rows)
                    rows.append(r)
                ids.append(index[key])
            enc.append(ids)
        variants[name] = dict(args=args, frames=enc, routes=routes)
    # the cases the fixture is for
    none, e = variants["none"], variants["e"]
    assert len(none["routes"]) >= 10 and none["routes"] != e["routes"]
    assert any(r[1] == "" for r in rows) and any(r[4] and not r[5] for r in rows) and any(r[5] and not r[4] for r in rows)
    assert dict(flight="XY0999", depa="LIRF", dsta="EHAM") in none["routes"] and dict(flight="XY0999", depa="LIRF", dsta="EHAM") in e["routes"]
    assert [r["flight"] for r in none["routes"]].index("XY0999") < [r["flight"] for r in e["routes"]].index("XY0999") or len(e["routes"]) < len(none["routes"])
    np.savez_compressed(os.path.join(HERE, "flights_pcm16.npz"), pcm=pcm)
    with open(os.path.join(HERE, "flights_golden.json"), "w") as f:
        json.dump(dict(label_list=LABEL_LIST, nch=NCH, sent=sent, rows=rows, variants=variants), f, indent=0)
    print("wrote %d transmissions from %d aircraft, %d samples per channel; frames / routes per variant: %s" % (
        len(sent), len({s["addr"] for s in sent}), pcm.shape[1], {k: (len(v["frames"]), len(v["routes"])) for k, v in variants.items()}))
