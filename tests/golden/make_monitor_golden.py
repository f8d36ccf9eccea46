"""Golden fixture for the flight table's TEXT: the bytes the unmodified reference program (oracle/_ref/acarsdec_cpu, as build()
makes it) writes for the committed flight recording (flights_pcm16.npz, see make_flight_golden.py) with -o 3 (the monitor
screen, printmonitor()) and -o 5 (the route line, routejson() + cJSON), in the five filter variants of make_flight_golden.py,
plus one -o 5 run with -i and a station id that needs an escape.  The five -o 5 runs pass -i "" (the key is absent, output.c:444):
without -i the reference names the station after the host it runs on.

The file front end stamps the wall clock, so every "hh:mm:ss.mmm" token and the route's "timestamp" number are masked (the tests
mask the model's and the device's bytes the same way; the masked part is pinned apart, against gmtime).  Run in the build
container only:

    python tests/golden/make_monitor_golden.py

Output (derived data, no reference source): monitor_golden.json
  {"nch", "station", "header": the two header lines of a frame, masked, behind cls(), "rows": the distinct masked rows,
   "variants": {name: {"args", "frames": per printed frame the indices of its rows, "routes": the masked route lines}},
   "station_routes": the masked lines of the -i run (variant "none")}
Bytes are stored as latin-1 strings."""
import json
import os
import subprocess
import sys
import tempfile
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import monitor_model as MM  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
LABEL_LIST = "QA:QN:QP:12:H1:QE"
VARIANTS = {"none": [], "A": ["-A"], "e": ["-e"], "b": ["-b", LABEL_LIST], "Aeb": ["-A", "-e", "-b", LABEL_LIST]}
STATION = 'st"1\\'


def reference(pcm, mode, args):
    exe = os.path.join(ROOT, "oracle", "_ref", "acarsdec_cpu")
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "flights.wav")
        with wave.open(p, "wb") as w:
            w.setnchannels(pcm.shape[0])
            w.setsampwidth(2)
            w.setframerate(12500)
            w.writeframes(np.ascontiguousarray(pcm.T).tobytes())
        r = subprocess.run([exe, "-o", str(mode)] + args + ["-f", p], capture_output=True)      # (the file front end ends with a non-zero status at the end of its file)
    return r.stdout


def route_lines(blob):
    return [MM.mask_route(ln + b"\n") for ln in blob.split(b"\n") if ln.startswith(b"{")]


if __name__ == "__main__":
    pcm = np.load(os.path.join(HERE, "flights_pcm16.npz"))["pcm"]
    with open(os.path.join(HERE, "flights_golden.json")) as f:
        fg = json.load(f)
    header, rows, index, variants = None, [], {}, {}
    for name, args in VARIANTS.items():
        assert args == fg["variants"][name]["args"]
        enc = []
        for fr in MM.split_frames(reference(pcm, 3, args)):
            fr = MM.mask_times(fr)
            head, body = fr[:MM.HDR_LEN], fr[MM.HDR_LEN:]
            assert header in (None, head) and head.startswith(MM.CLS), head
            header = head
            lines = body.split(b"\n")
            assert lines[-1] == b"", lines[-1]
            ids = []
            for ln in lines[:-1]:
                ids.append(index.setdefault(ln, len(rows)))
                if ids[-1] == len(rows):
                    rows.append(ln.decode("latin1"))
            enc.append(ids)
        routes = route_lines(reference(pcm, 5, args + ["-i", ""]))      # (without -i the station is the host's name)
        assert len(enc) == len(fg["variants"][name]["frames"]) and len(routes) == len(fg["variants"][name]["routes"]), name
        variants[name] = dict(args=args, frames=enc, routes=[r.decode("latin1") for r in routes])
    station_routes = route_lines(reference(pcm, 5, ["-i", STATION]))
    assert len(station_routes) == len(variants["none"]["routes"]) and all(b'"station_id":"st\\"1\\\\"' in r for r in station_routes)
    out = dict(nch=int(pcm.shape[0]), station=STATION, header=header[MM.CLS_LEN:].decode("latin1"), rows=rows, variants=variants,
               station_routes=[r.decode("latin1") for r in station_routes])
    path = os.path.join(HERE, "monitor_golden.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote %s: %d bytes, %d distinct rows, frames / routes per variant: %s" % (
        path, os.path.getsize(path), len(rows), {k: (len(v["frames"]), len(v["routes"])) for k, v in variants.items()}))
