"""The flight table's text without a GPU: the Python model of the reference's monitor screen and route line
(tests/monitor_model.py) against the bytes the reference program printed for the flight fixture
(tests/golden/monitor_golden.json, made by tests/golden/make_monitor_golden.py), the masked time token against the C library's
gmtime, the kernels' own integer arithmetic (csrc/flight_text_num.h, compiled for the host) against glibc, the ABI of the new
entry points, the code object's budget, and the seam coverage of the designed inputs the GPU self test runs."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import time

import pytest

from conftest import GOLDEN, ROOT
import flight_model as FM
import label_model as LM
import monitor_model as MM

VARIANTS = ("none", "A", "e", "b", "Aeb")
T0 = MM.T0


@pytest.fixture(scope="module")
def fix():
    with open(os.path.join(GOLDEN, "flights_golden.json")) as f:
        fg = json.load(f)
    with open(os.path.join(GOLDEN, "monitor_golden.json")) as f:
        mg = json.load(f)
    return fg, mg


def reference_frames(mg, v):
    """the reference's masked frames of variant v, put together again from the fixture's parts"""
    rows, head = mg["rows"], MM.CLS + mg["header"].encode("latin1")
    return [head + b"".join(rows[i].encode("latin1") + b"\n" for i in ids) for ids in mg["variants"][v]["frames"]]


def walk_the_fixture(fg, args, on_frame):
    """the list walk over the fixture's transmissions under the filters of `args`; on_frame(entries, tv) for every message the
    reference prints a frame for.  Returns the walk."""
    kw = dict(downlink_only="-A" in args, skip_empty="-e" in args, labels=LM.parse_label_filter(fg["label_list"]) if "-b" in args else ())
    walk = FM.ListWalk(600)
    for s in fg["sent"]:
        m = FM.record_of(bytes.fromhex(s["addr"]), bytes.fromhex(s["label"]), s["bid"].encode(), bytes.fromhex(s["text"]), s["chn"],
                         s["end_sample"], s["soh_sample"])
        ev = FM.event_of(m, T0, **kw)
        if ev is not None:
            walk.add(ev)
        if LM.keep(m.down, m.label, m.txt, m.txt_len, **kw):
            on_frame(walk.entries(), FM.tv(T0[0], T0[1], s["soh_sample"]))
    return walk


def test_model_reproduces_every_frame_and_route_line_of_the_reference(fix):
    """Every frame of every variant, whole, and every route line, the -i run included, equal the reference's masked bytes.  The
    number of frames compared is flights_golden.json's frame count: nothing is left out."""
    fg, mg = fix
    assert mg["nch"] == fg["nch"] == 3 and mg["header"].encode("latin1") == MM.mask_times(MM.header(T0))[MM.CLS_LEN:]
    compared = {}
    for v in VARIANTS:
        args = mg["variants"][v]["args"]
        assert args == fg["variants"][v]["args"]
        want, mine = reference_frames(mg, v), []
        walk = walk_the_fixture(fg, args, lambda entries, tv: mine.append(MM.mask_times(MM.frame(entries, mg["nch"], tv))))
        assert len(mine) == len(want) == len(fg["variants"][v]["frames"]), (v, len(mine), len(want))
        for k, (a, b) in enumerate(zip(mine, want)):
            assert a == b, (v, k, a, b)
        routes = [MM.mask_route(MM.route_line(r)) for r in walk.routes]
        assert routes == [r.encode("latin1") for r in mg["variants"][v]["routes"]] and len(routes) == len(fg["variants"][v]["routes"]) >= 10, v
        compared[v] = (len(mine), len(routes))
        if v == "none":
            st = [MM.mask_route(MM.route_line(r, mg["station"].encode("latin1"))) for r in walk.routes]
            assert st == [r.encode("latin1") for r in mg["station_routes"]] and all(b'"station_id":"st\\"1\\\\"' in r for r in st)
    print("frames / route lines compared:", compared)
    assert compared["none"][0] == 115 and sum(c[0] for c in compared.values()) == sum(len(fg["variants"][v]["frames"]) for v in VARIANTS)
    # the rows carry what decides bytes: an empty flight id, empty and filled DEP / ARR / ETA, every mask pattern of three channels
    rows = [r.encode("latin1") for r in mg["rows"]]
    assert all(len(r) == 69 for r in rows) and any(r[10:17] == b" " * 7 for r in rows)
    assert any(r[51:57] == b" " * 6 for r in rows) and any(r[51:57] != b" " * 6 and r[57:63] == b" " * 6 for r in rows)
    assert {r[22:25] for r in rows} >= {b"x..", b".x.", b"..x", b"xxx"} and all(r[25:38] == b" " * 13 for r in rows)


def test_time_token_and_timestamp_equal_the_c_library():
    """the masked parts, pinned apart: printtime() against time.gmtime at usec 0 / 999 / 999999, a day's last and first second,
    tv_sec >= 2^31 and >= 2^32; the header's tv from a soh_sample past 2^31, 2^32 and 2^40; the route's number round-trips"""
    secs = [s for s, _ in MM.TIMES] + [1700006399, 1700006400, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 33 + 86399]
    assert 1700006400 % 86400 == 0
    for s in secs:
        for u in (0, 999, 1000, 999999):
            t = time.gmtime(s)
            assert MM.time_text(s, u) == b"%02d:%02d:%02d.%03d" % (t.tm_hour, t.tm_min, t.tm_sec, u // 1000), (s, u)
    assert MM.time_text(1700006399, 999999) == b"23:59:59.999" and MM.time_text(1700006400, 0) == b"00:00:00.000"
    assert MM.time_text(2 ** 32, 999) == b"06:28:16.000" and MM.time_text(2 ** 31, 999999) == b"03:14:08.999"
    for soh in MM.HDR_SOH[1:]:
        sec, usec = MM.header_tv([], T0, soh)
        assert sec * 1000000 + usec == T0[0] * 1000000 + T0[1] + soh * 80 and 0 <= usec < 1000000
    assert MM.header_tv([], T0, -1) == T0 and MM.header_tv([dict(tl=(5, 6))], T0, -1) == (5, 6)
    for r in MM.designed_routes(300, 0):
        tok = MM.route_line(r).split(b",")[0][len(b'{"timestamp":'):]
        assert float(tok) == r["sec"] + r["usec"] / 1e6


def test_rows_and_lines_by_hand():
    """the format strings restated once by hand, and the header's bounds token by token"""
    z = b"\0" * 4
    f = dict(addr=b"N12345\0\0", fid=b"AB0123\0", nbm=7, chm=0b101, ts=(1700006399, 999999), tl=(0, 0), fields=[z, b"EGLL", b"12\0\0"] + [z] * 4)
    assert MM.row(f, 3) == b" N12345   AB0123    7 x.x" + b" " * 13 + b" 23:59:59.999 EGLL " + b" " * 6 + b"   12 \n"
    assert len(MM.row(f, 3)) == 70 and len(MM.row(dict(f, nbm=1000), 0)) == 71 and len(MM.row(dict(f, nbm=2 ** 31 - 1), 16)) == 77
    assert len(MM.row(dict(f, nbm=-2 ** 31, addr=b"1234567\0", fid=b"1234567"), 16)) == 78 == MM.ROW_MAX
    assert MM.row(dict(f, chm=0xFFFF0000), 16)[22:38] == b"." * 16 and MM.row(dict(f, chm=2 ** 64 - 1), 16)[22:38] == b"x" * 16
    assert len(MM.header((0, 0))) == MM.HDR_LEN == 7 + 30 + 12 + 61 and MM.header((0, 0))[:MM.CLS_LEN] == MM.CLS
    r = dict(sec=1700000000, usec=500000, fid=b'A"\x01\0\0\0\0', sa=b"EGLL", da=b"K\\\0\0")
    assert MM.route_line(r, b"s\n") == b'{"timestamp":1700000000.5,"station_id":"s\\n","flight":"A\\"\\u0001","depa":"EGLL","dsta":"K\\\\"}\n'
    worst = dict(sec=1700000000, usec=123457, fid=b"\x01" * 7, sa=b"\x02" * 4, da=b"\x03" * 4)
    assert len(MM.route_line(worst, b"\x1f" * 32)) == 363 - 1 == MM.LINE_MAX - 1          # (this number has 17 characters, the bound counts 18)
    assert len(MM.route_line(dict(worst, fid=b"\x01" * 6 + b"\0"), b"\x1f" * 32)) == 357 - 1


def test_designed_inputs_reach_every_seam():
    """Over the designed inputs of the GPU self test a row starts at every residue mod 16 and ends at every residue mod 16 (rows
    of 70 bytes alone reach eight), and so do the route lines; the cases the issue names are all there."""
    cases = MM.designed_cases()
    starts, ends, lens, lstarts, lends = set(), set(), set(), set(), set()
    for c in cases:
        spans = MM.row_spans(c["entries"], c["nbch"])
        starts |= {a % 16 for a, _ in spans}
        ends |= {b % 16 for _, b in spans}
        lens |= {b - a for a, b in spans}
        at = 0
        for r in c["routes"]:
            n = len(MM.route_line(r, c["station"]))
            lstarts.add(at % 16)
            lends.add((at + n) % 16)
            at += n
    assert starts == ends == lstarts == lends == set(range(16)) and {70, 71, 77} <= lens
    only70 = {(MM.HDR_LEN + 70 * i) % 16 for i in range(64)}
    assert len(only70) == 8
    assert tuple(len(c["entries"]) for c in cases) == MM.ROW_COUNTS == (0, 1, 2, 63, 64, 65, 256, 257, 1025)
    assert {len(c["routes"]) for c in cases} == {0, 1, 64, 65, 257} and {c["nbch"] for c in cases} == {0, 1, 3, 16}
    assert {c["hdr_soh"] for c in cases} == set(MM.HDR_SOH) and {c["station"] for c in cases} == set(MM.STATIONS)
    ent = [f for c in cases for f in c["entries"]]
    assert {f["nbm"] for f in ent} >= {1, 999, 1000, 2 ** 31 - 1} and any(not f["fid"][0] for f in ent) and any(f["addr"][6] for f in ent)
    for k in (0, 1, 2):
        assert any(not f["fields"][k][0] for f in ent) and any(f["fields"][k][0] and not f["fields"][k][3] for f in ent), k
    assert {2 ** 64 - 1, 0, 0xFFFFFFFFFFFF0000} <= {f["chm"] for f in ent} and {f["ts"] for f in ent} == set(MM.TIMES)
    blob = b"".join(r["fid"] + r["sa"] + r["da"] for c in cases for r in c["routes"])
    assert all(ch in blob for ch in b'"\\\n\x01\x80\xff')
    assert len(MM.STATIONS[1]) == 32 and all(b < 32 for b in MM.STATIONS[1])


def test_the_kernels_time_and_count_printers_equal_glibc(tmp_path):
    """csrc/flight_text_num.h is what flight_text.hip compiles for the device; tests/flight_text_num_check.cpp compiles the same
    functions for the host and holds "%3d" (1, 9, 99, 999, 1000, 2^31 - 1, ...) and the time token against snprintf / gmtime_r"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path / "flight_text_num_check")
    r = subprocess.run([cxx, "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "acarsdec_amd", "csrc"), os.path.join(ROOT, "tests", "flight_text_num_check.cpp"),
                        "-o", exe, "-lm"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe, "200000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:]


def test_abi_exports_the_flight_text_entry_points():
    """the new symbols are exported and declared, the header's bounds are the model's, and argument errors come before any device
    is looked for; the self test needs a device (ACG_ENODEV: there is no CPU fallback)"""
    from acarsdec_amd import _capi as K, _build
    L = K.load()
    declared = _build.declared_symbols()
    for name in ("acg_flight_text_enable", "acg_flight_monitor_text", "acg_drain_routes_json", "acg_selftest_flight_text"):
        assert hasattr(L, name) and name in declared, name
    hdr = open(os.path.join(ROOT, "include", "acarsdec_amd.h")).read()
    val = lambda name: int(re.search(r"#define %s\s+(\d+)" % name, hdr).group(1))
    assert (val("ACG_MONITOR_CLS_LEN"), val("ACG_MONITOR_HDR_LEN"), val("ACG_MONITOR_ROW_MAX"), val("ACG_ROUTE_LINE_MAX")) == \
           (K.MONITOR_CLS_LEN, K.MONITOR_HDR_LEN, K.MONITOR_ROW_MAX, K.ROUTE_LINE_MAX) == (MM.CLS_LEN, MM.HDR_LEN, MM.ROW_MAX, MM.LINE_MAX)
    assert C.sizeof(K.FlightTextConfig) == 40 and K.FlightTextConfig.station_id.offset == 4
    nb, n = C.c_size_t(0), C.c_int(0)
    buf = C.create_string_buffer(1024)
    good = K.FlightTextConfig(3, b"st1")
    assert L.acg_flight_text_enable(None, C.byref(good)) == K.EINVAL
    assert L.acg_flight_monitor_text(None, -1, buf, len(buf), C.byref(nb), C.byref(n), None) == K.EINVAL
    assert L.acg_drain_routes_json(None, buf, len(buf), C.byref(nb), C.byref(n)) == K.EINVAL
    fcfg = K.FlightConfig(T0[0], T0[1], 600, 16)
    call = lambda tc, fc=fcfg, nrows=0: L.acg_selftest_flight_text(None, nrows, None, 0, C.byref(fc), C.byref(tc) if tc is not None else None, -1, buf, len(buf),
                                                                   C.byref(nb), C.byref(n), buf, len(buf), C.byref(nb), C.byref(n))
    unterminated = K.FlightTextConfig(3, b"")
    C.memset(C.byref(unterminated, K.FlightTextConfig.station_id.offset), ord("S"), 33)
    for bad in (K.FlightTextConfig(-1, b""), K.FlightTextConfig(17, b""), unterminated, None):
        assert call(bad) == K.EINVAL
    assert call(good, K.FlightConfig(0, 0, 0, 16)) == K.EINVAL and call(good, nrows=-1) == K.EINVAL and call(good, nrows=1) == K.EINVAL
    assert call(good) == (K.OK if L.acg_device_count() > 0 else K.ENODEV)


# DESIGN.md 4 states these: VGPRs and LDS bytes per kernel of flight_text.hip as the product builds it
BUDGET = {"mon_measure": (14, 256), "mon_render": (119, 544), "route_keys": (8, 0), "route_measure": (29, 128), "route_render": (108, 928),
          "sum": (6, 264), "offsets": (21, 24)}


def test_flight_text_kernels_use_no_scratch_and_keep_their_budget():
    """flight_text.hip compiled with the product's flags (text.hip's): a private segment of 0 bytes for every kernel, no scratch
    instruction, and the register and LDS counts DESIGN.md states"""
    from acarsdec_amd import _build as B
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    assert hipcc, "hipcc"
    csrc = os.path.join(ROOT, "acarsdec_amd", "csrc")
    flags = {name: (f, prod) for name, f, prod in B.UNITS}
    assert flags["flight_text.hip"] == (flags["text.hip"][0], True)
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include")] +
                       flags["flight_text.hip"][0] + ["-S", "-o", "-", os.path.join(csrc, "flight_text.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = [n.split("flight_text_")[1].split("_kernel")[0] for n in re.findall(r"^\s*\.amdhsa_kernel (\S+)", r.stdout, flags=re.M)]
    scratch = [int(v) for v in re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", r.stdout)]
    vgpr = [int(v) for v in re.findall(r"\.amdhsa_next_free_vgpr (\d+)", r.stdout)]
    lds = [int(v) for v in re.findall(r"\.amdhsa_group_segment_fixed_size (\d+)", r.stdout)]
    print("flight_text.hip kernels:", list(zip(names, vgpr, lds, scratch)))
    assert sorted(names) == sorted(BUDGET) and len(scratch) == len(BUDGET) and not any(scratch), (names, scratch)
    assert "scratch_" not in r.stdout
    assert {n: (v, l) for n, v, l in zip(names, vgpr, lds)} == BUDGET
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for n, (v, l) in BUDGET.items():
        assert re.search(r"flight_text_%s_kernel\s*\|\s*%d\s*\|\s*%d\s*\|" % (n, v, l), design), n
