"""The flight table without a GPU: the device's lazy expiry rule against the reference's list walk (tests/flight_model.py) on
random traffic, the new entry points of the C ABI, and the instruction stream of the flight kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import flight_model as FM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPS_PER_BYTE = 12500 * 8 / 2400.0                     # 12.5 kHz samples per transmitted byte (2400 bit/s)


def random_traffic(rng, n, naircraft, nch, max_gap_s):
    """n events in (end_sample, chn) order.  A block of L <= 241 bytes ends L bytes after its SOH: tv (taken at the SOH) lies up
    to 0.81 s before end_sample, so tv runs backwards between neighbours -- the case the lazy rule has to survive."""
    airports = [b"KJFK", b"EGLL", b"LFPG", b"EDDF", b"\0\0\0\0"]
    gaps = np.where(rng.random(n) < 0.02, rng.uniform(0, max_gap_s, n), rng.exponential(0.05, n))
    end = 20000 + np.cumsum(np.rint(gaps * 12500).astype(np.int64) + 1)
    out = []
    for i in range(n):
        length = int(rng.integers(13, 242))
        chn = int(rng.integers(0, nch))
        soh = int(end[i]) - int(round((length + 2) * SPS_PER_BYTE))
        f = [b"\0" * 4] * 7
        for k in range(7):
            if rng.random() < 0.25:
                f[k] = airports[int(rng.integers(0, 4))] if k < 2 else b"%04d" % int(rng.integers(0, 2400))
        fid = b"" if rng.random() < 0.15 else b"XY%04d" % int(rng.integers(0, 30))
        sec, usec = FM.tv(1700000000, 999000, soh)
        out.append(FM.Event(b"N%05d" % int(rng.integers(0, naircraft)), fid, chn, soh, int(end[i]), sec, usec, tuple(f), rng.random() < 0.7))
    return out


def both(events, mdly):
    walk, lazy = FM.ListWalk(mdly), FM.LazyTable(mdly)
    for k, ev in enumerate(events):
        ra, rb = walk.add(ev), lazy.add(ev)
        assert ra == rb, (k, ra, rb)
        a, b = [FM.entry_key(f) for f in walk.entries()], [FM.entry_key(f) for f in lazy.entries()]
        assert a == b, (k, mdly)
    assert walk.routes == lazy.routes
    return walk


def test_lazy_rule_equals_the_list_walk_on_random_traffic():
    """'live iff tl_sec + mdly >= G, restart when the running maximum before the message exceeds it' gives the same rows after
    every message and the same routes as deleting from the list after every message: 200 000 messages in (end_sample, chn)
    order, blocks up to 241 bytes (tv up to 0.81 s behind end_sample), mdly 1 .. 5, gaps up to 20 s."""
    rng = np.random.default_rng(20261017)
    total = recreated = routes = 0
    for mdly in (1, 2, 3, 4, 5):
        ev = random_traffic(rng, 40000, 60, 16, 20.0)
        assert any(b.sec < a.sec for a, b in zip(ev, ev[1:])), "no message with an earlier second behind a later one"
        w = both(ev, mdly)
        total += len(ev)
        recreated += w.recreated
        routes += len(w.routes)
    # (entries expired and were made anew, thousands of times; routes came out)
    assert total >= 200000 and recreated > 1000 and routes > 100


def test_lazy_rule_at_a_second_boundary():
    """By hand: message B ends after message A but was stamped in the second BEFORE A's (a long block), with mdly = 1.  The list
    walk, at A, deletes what is older than A.sec - 1; at B (one second back) nothing more.  An aircraft last heard at A.sec - 2
    is gone when B arrives, one heard at A.sec - 1 stays -- and B's own aircraft, heard at A.sec - 2, restarts."""
    t0 = 1000
    def ev(addr, end, length, **kw):
        soh = end - int(round(length * SPS_PER_BYTE))
        sec, usec = FM.tv(t0, 0, soh)
        return FM.Event(addr, kw.get("fid", b"AB0001"), kw.get("chn", 0), soh, end, sec, usec,
                        tuple(kw.get("f", [b"\0" * 4] * 7)), True)
    s = 12500
    sa_da = [b"EGLL", b"KJFK"] + [b"\0" * 4] * 5
    seq = [ev(b"OLD", 8 * s + 600, 13, f=sa_da),          # sec 8: sa and da known, route emitted
           ev(b"KEEP", 9 * s + 600, 13),                   # sec 9
           ev(b"A", 10 * s + 700, 13),                     # sec 10: deletes OLD (8 < 10 - 1), keeps KEEP
           ev(b"OLD", 10 * s + 900, 40, chn=1, f=sa_da)]   # ends later, stamped in sec 9: OLD starts anew, emits its route again
    assert [e.sec - t0 for e in seq] == [8, 9, 10, 9]
    w = both(seq, 1)
    assert [f["addr"].rstrip(b"\0") for f in w.entries()] == [b"OLD", b"A", b"KEEP"]
    assert w.entries()[0]["nbm"] == 1 and w.entries()[0]["first_chn"] == 1 and len(w.routes) == 2
    # and with mdly = 2 nothing expires: one entry for OLD with both messages, one route
    w = both(seq, 2)
    assert w.entries()[0]["nbm"] == 2 and w.entries()[0]["chm"] == 3 and len(w.routes) == 1


def test_route_waits_for_a_message_that_passes_e():
    """a message that completes (fid, sa, da) but fails -e updates the entry and emits nothing; the next one that passes does"""
    mk = lambda end, f, e_ok, fid=b"AB0001": FM.Event(b"N1", fid, 0, end - 600, end, *FM.tv(0, 0, end - 600), tuple(f), e_ok)
    z = b"\0" * 4
    w = both([mk(20000, [z, b"EGLL"] + [z] * 5, True), mk(40000, [b"KJFK"] + [z] * 6, False), mk(60000, [z] * 7, True, fid=b""),
              mk(80000, [z] * 7, True)], 600)
    assert len(w.routes) == 1 and w.routes[0]["soh_sample"] == 80000 - 600 and w.routes[0]["sa"] == b"EGLL" and w.routes[0]["da"] == b"KJFK"


def test_model_equals_the_reference_monitor_and_routes():
    """The list walk over the fixture's transmissions, per filter variant: after every message the reference printed a monitor
    frame for, the model's rows equal that frame (the unmodified reference program's -o 3 output); the model's routes equal
    its -o 5 lines, in order.  The fixture holds the cases the table is about, and its ordering condition."""
    import json
    import label_model as LM
    with open(os.path.join(ROOT, "tests", "golden", "flights_golden.json")) as f:
        g = json.load(f)
    sent, nch = g["sent"], g["nch"]
    ends = sorted(s["end_sample"] for s in sent)
    assert 100 <= len(sent) <= 150 and 20 <= len({s["addr"] for s in sent}) <= 30 and {s["chn"] for s in sent} == set(range(nch))
    assert min(b - a for a, b in zip(ends, ends[1:])) > 4096          # at most one block completes per 4096-frame chunk of the file
    assert ends == [s["end_sample"] for s in sent]
    for v, gv in g["variants"].items():
        args = gv["args"]
        kw = dict(downlink_only="-A" in args, skip_empty="-e" in args, labels=LM.parse_label_filter(g["label_list"]) if "-b" in args else ())
        walk, k = FM.ListWalk(600), 0
        for s in sent:
            m = FM.record_of(bytes.fromhex(s["addr"]), bytes.fromhex(s["label"]), s["bid"].encode(), bytes.fromhex(s["text"]), s["chn"],
                             s["end_sample"], s["soh_sample"])
            ev = FM.event_of(m, (1700000000, 0), **kw)
            if ev is not None:
                walk.add(ev)
            if LM.keep(m.down, m.label, m.txt, m.txt_len, **kw):
                assert [FM.monitor_row(f, nch) for f in walk.entries()] == [g["rows"][i] for i in gv["frames"][k]], (v, k)
                k += 1
        assert k == len(gv["frames"]), (v, k)
        routes = [dict(flight=r["fid"].split(b"\0")[0].decode(), depa=r["sa"].decode(), dsta=r["da"].decode()) for r in walk.routes]
        assert routes == gv["routes"] and len(routes) >= 10, v
    # the cases: an empty flight id, DEP without ARR and ARR without DEP (they arrive in different messages), a changed flight
    # id, a field overwritten, and the route that -e defers (N00999: its ARR comes in a text that starts with NUL)
    rows = g["rows"]
    assert any(r[1] == "" for r in rows) and any(r[4] and not r[5] for r in rows) and any(r[5] and not r[4] for r in rows)
    assert any(a[0] == b[0] and a[1] and b[1] and a[1] != b[1] for a in rows for b in rows)
    assert any(a[0] == b[0] and a[4] and b[4] and a[4] != b[4] for a in rows for b in rows)
    pos = lambda v: [r["flight"] for r in g["variants"][v]["routes"]].index("XY0999")
    none, e = g["variants"]["none"], g["variants"]["e"]
    assert none["routes"][pos("none")] == e["routes"][pos("e")] == dict(flight="XY0999", depa="LIRF", dsta="EHAM")
    assert none["routes"] != e["routes"] and sorted(map(str, none["routes"])) == sorted(map(str, e["routes"]))


def test_abi_exports_the_flight_entry_points():
    """the four new symbols are exported and declared; without a context every call is ACG_EINVAL, a bad configuration is
    ACG_EINVAL before any device is looked for, and the self test needs a device (ACG_ENODEV: there is no CPU fallback)"""
    from acarsdec_amd import _capi as K
    L = K.load()
    for name in ("acg_flights_enable", "acg_flight_snapshot", "acg_drain_routes", "acg_selftest_flights"):
        assert hasattr(L, name), name
    good = K.FlightConfig(1700000000, 0, 600, 1024)
    assert L.acg_flights_enable(None, C.byref(good)) == K.EINVAL
    assert L.acg_flights_enable(None, None) == K.EINVAL
    n, d = C.c_int(0), C.c_int(0)
    assert L.acg_flight_snapshot(None, None, 0, C.byref(n), C.byref(d)) == K.EINVAL
    assert L.acg_drain_routes(None, None, 0, C.byref(n)) == K.EINVAL
    nr = C.c_int(0)
    for bad in (K.FlightConfig(0, 0, 0, 16), K.FlightConfig(0, 0, 600, 0), K.FlightConfig(0, 1000000, 600, 16), K.FlightConfig(0, -1, 600, 16)):
        assert L.acg_selftest_flights(None, None, 0, C.byref(bad), None, None, 0, None, None, 0, C.byref(nr), C.byref(d)) == K.EINVAL
    assert L.acg_selftest_flights(None, None, 0, None, None, None, 0, None, None, 0, C.byref(nr), C.byref(d)) == K.EINVAL
    rc = L.acg_selftest_flights(None, None, 0, C.byref(good), None, None, 0, None, None, 0, C.byref(nr), C.byref(d))
    assert rc == (K.OK if L.acg_device_count() > 0 else K.ENODEV)
    assert C.sizeof(K.Flight) == 120 and C.sizeof(K.Route) == 56 and K.Flight.chm.offset == 32 and K.Flight.da.offset == 80
    assert K.Route.fid.offset == 24 and K.Route.addr.offset == 41


def test_monitor_rows_and_route_json_render_like_the_reference():
    """monitor_rows() is printmonitor()'s row without the clock column, route_json() is routejson()'s object"""
    from acarsdec_amd import _capi as K
    from acarsdec_amd import decoder as D
    f = K.Flight(addr=b"N12345", fid=b"AB0123", nbm=7, chm=0b101, sa=b"EGLL", da=b"", eta=b"1234")
    assert D.monitor_rows([f], 3) == [" N12345   AB0123    7 x.x" + " " * 13 + " " + " EGLL " + " " * 6 + " 1234 "]
    r = K.Route(sec=1700000000, usec=500000, fid=b"AB0123", sa=b"EGLL", da=b"KJFK")
    assert list(D.route_json(r, "st1").items()) == [("timestamp", 1700000000.5), ("station_id", "st1"), ("flight", "AB0123"),
                                                   ("depa", "EGLL"), ("dsta", "KJFK")]
    assert "station_id" not in D.route_json(r)


def test_flight_kernels_use_no_scratch():
    """flight.hip's own kernels and the event extraction in label.hip, compiled with the product's flags: no scratch access,
    no private segment (the wave keeps its entry in registers)."""
    from acarsdec_amd import _build as B
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "acarsdec_amd", "csrc")
    flags = {name: fl for name, fl, _ in B.UNITS}
    want = {"flight.hip": ("flight_sort_kernel", "flight_order_kernel", "flight_heads_kernel", "flight_walk_kernel", "flight_finish_kernel",
                           "flight_snapkeys_kernel", "flight_snapshot_kernel"),
            "label.hip": ("flight_extract_kernel",)}
    for unit, names in want.items():
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include")] +
                           flags[unit] + ["-S", "-o", "-", os.path.join(csrc, unit)], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        kernels, cur = {}, None
        for line in r.stdout.splitlines():
            m = re.match(r"^_Z\d+(flight_\w+?_kernel)\w*:", line)
            if m:
                cur = m.group(1)
                kernels[cur] = []
            elif line.startswith(".Lfunc_end"):
                cur = None
            elif cur:
                kernels[cur].append(line)
        assert sorted(kernels) == sorted(names), sorted(kernels)
        for name, body in kernels.items():
            assert not any("scratch_" in l for l in body), name
        priv = re.findall(r"\.amdhsa_kernel _Z\d+(flight_\w+?_kernel)\w*\n(?:.*\n)*?\s*\.amdhsa_private_segment_fixed_size (\d+)", r.stdout)
        assert sorted(priv) == sorted((n, "0") for n in names), priv
