"""The JSON sink without a GPU: the Python model of the reference's line (tests/json_model.py) against the lines the reference
program printed for the JSON fixture (tests/golden/msgjson_golden.json, made by tests/golden/make_msgjson_golden.py), the two
number printers against the C library's, the kernel's own integer arithmetic (csrc/json_num.h, compiled for the host) against
glibc, and the ABI of the new entry points."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import json_model as JM
import label_model as LM

VARIANTS = ("none", "A", "e", "b", "Aeb")


@pytest.fixture(scope="module")
def fix():
    pcm = np.load(os.path.join(GOLDEN, "msgjson_pcm16.npz"))["pcm"]
    with open(os.path.join(GOLDEN, "msgjson_golden.json")) as f:
        return pcm, json.load(f)


@pytest.fixture(scope="module")
def oracle_msgs(fix):
    """per channel: the split records of the fixture from the oracle's restatement of demodulator, framing, repair and split"""
    from oracle import oracle as O
    pcm, g = fix
    out = []
    for c in range(g["nch"]):
        ch = O.Channel(c, max_frames=256)
        x = pcm[c].astype(np.float32) / np.float32(32768.0)
        for s in range(0, x.size, 4096):
            ch.demod(x[s:s + 4096])
        msgs = []
        for f in ch.frames:
            b = O.blk_process(f)
            if b is not None:
                msgs.append(O.msg_split(b))
        out.append(msgs)
    return out


def filter_kw(g, variant):
    args = g["variants"][variant]["args"]
    return dict(downlink_only="-A" in args, skip_empty="-e" in args, labels=LM.parse_label_filter(g["label_list"]) if "-b" in args else ())


def ref_lines(g, variant, chn):
    """the reference's lines of one channel, bytes with their newline"""
    out = []
    for ln in g["variants"][variant]["lines"]:
        b = ln.encode("ascii") + b"\n"
        if json.loads(ln)["channel"] == chn:
            out.append(b)
    return out


def app_of(g):
    j = json.loads(g["variants"]["none"]["lines"][0])
    return j["app"]["name"].encode(), j["app"]["ver"].encode()


def test_fixture_holds_every_scripted_case(fix):
    """no case is silently absent: every transmission is among the unfiltered lines, and the cases that decide bytes are there"""
    _, g = fix
    lines = g["variants"]["none"]["lines"]
    assert len(lines) == len(g["sent"]) and len({s["what"] for s in g["sent"]}) > 40
    js = [json.loads(ln) for ln in lines]
    blob = "\n".join(lines)
    for esc in ('\\"', "\\\\", "\\b", "\\f", "\\n", "\\r", "\\t", "\\u0001", "\\u001f", '"mode":"\\""', '"mode":""', '"ack":false', '"ack":"\\""',
                '"end":true', '"label":"Qd"', '"label":"5"', '"depa":"KJ\\u0005K"', '"wlin":', '"gtin":', '"wloff":', '"gtout":', '"eta":'):
        assert esc in blob, esc
    assert any("block_id" not in j for j in js) and any("text" not in j for j in js) and any(j.get("msgno") == "M0" for j in js)
    assert any(j.get("flight") == 'X"\x1fY12' and j.get("msgno") == 'M\x02"A' and j["tail"] == 'N"1\x0145' for j in js)
    assert all(j["station_id"] == g["station"] and j["freq"] == 0 for j in js)


def test_model_reproduces_every_reference_line_byte_for_byte(fix, oracle_msgs):
    """Every variant, every channel: the model's line of each record the filters keep equals the line the reference printed, once
    the time stamp's number (the reference's wall clock) is cut out of both."""
    _, g = fix
    app = app_of(g)
    for v in VARIANTS:
        kw = filter_kw(g, v)
        total = 0
        for c in range(g["nch"]):
            want = [JM.cut_timestamp(ln)[0] for ln in ref_lines(g, v, c)]
            mine = [JM.cut_timestamp(JM.line(m, c, b"0", station=g["station"].encode(), app=app))[0] for m in oracle_msgs[c] if JM.keep(m, **kw)]
            assert mine == want, (v, c, next((a, b) for a, b in zip(mine + [None], want + [None]) if a != b))
            total += len(mine)
        assert total == len(g["variants"][v]["lines"])
    assert max(len(ln) for ln in g["variants"]["none"]["lines"]) + 1 <= JM.LINE_MAX


def test_number_printer_reprints_every_reference_timestamp(fix):
    _, g = fix
    n = 0
    for v in VARIANTS:
        for ln in g["variants"][v]["lines"]:
            tok = JM.cut_timestamp(ln.encode("ascii") + b"\n")[1].decode()
            assert JM.print_number(float(tok)) == tok
            n += 1
    assert n > 150


def test_integer_number_printer_equals_the_c_library_recipe():
    """the kernel's algorithm (integer arithmetic on the double's fraction) against '%1.15g' / '%1.17g' with the parse-back test"""
    rng = np.random.default_rng(20261018)
    edge = [10 ** 9, 2 ** 30 - 1, 2 ** 30, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1]
    cases = [(s, u) for s in edge for u in (0, 1, 80, 499999, 500000, 500001, 999920, 999999)]
    cases += [(s, 80 * int(k)) for s in edge for k in rng.integers(0, 12500, 2000)]
    sec = rng.integers(10 ** 9, 2 ** 32, 200000)
    usec = np.where(rng.integers(0, 2, sec.size) == 0, 80 * rng.integers(0, 12500, sec.size), rng.integers(0, 10 ** 6, sec.size))
    usec[::97] = 0
    cases += list(zip(sec.tolist(), usec.tolist()))
    seventeen = 0
    for s, u in cases:
        want = JM.print_number(JM.tv_double(s, u))
        assert JM.print_number_int(s, u) == want, (s, u)
        seventeen += len(want) > 16
    assert 0 < seventeen < len(cases)                        # both precisions occur


def test_level_printer_equals_the_c_library():
    rng = np.random.default_rng(7)
    vals = [0.05, -0.05, 0.25, -0.25, 0.35, -0.35, -0.04, 0.0, -0.0, np.inf, -np.inf, np.nan, 9.95, 99.95, -999.95, 3240.1, -3240.1, 123456.7]
    vals += (rng.integers(-100000, 100001, 50000) / 20.0).tolist()                  # tenths and their midpoints
    vals += rng.uniform(-3300, 3300, 100000).tolist()
    vals += rng.integers(0, 2 ** 32, 50000, dtype=np.uint64).astype(np.uint32).view(np.float32).tolist()    # any bit pattern
    for x in vals:
        f = np.float32(x)
        if np.isfinite(f) and abs(f) >= 9e17:
            continue
        assert JM.level_text(f) == JM.level_libc(f), repr(f)
    assert JM.level_text(np.float32(-0.04)) == "-0.0" and JM.level_text(np.float32(0.25)) == "0.2" and JM.level_text(np.float32(0.35)) == "0.3"
    assert JM.level_text(np.copysign(np.float32(np.nan), np.float32(-1))) == "-nan"


def test_the_kernels_number_printers_equal_glibc(tmp_path):
    """csrc/json_num.h is what json.hip compiles for the device; tests/json_num_check.cpp compiles the same functions for the
    host and holds them against snprintf / sscanf on edge cases and 200 000 random values each."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path / "json_num_check")
    r = subprocess.run([cxx, "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "acarsdec_amd", "csrc"), os.path.join(ROOT, "tests", "json_num_check.cpp"),
                        "-o", exe, "-lm"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe, "200000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:]


def test_freq_token_and_escaping():
    assert JM.freq_token(131725000) == b"131.725" and JM.freq_token(0) == b"0.000" and JM.freq_token(1090000000) == b"1090.00"
    assert JM.escape(b'a"b\\c\x01\x1f\n\0zz') == b'a\\"b\\\\c\\u0001\\u001f\\n'
    assert JM.quoted(b"\0") == b'""'


def test_abi_exports_the_json_entry_points():
    """the new symbols are exported and declared; argument errors come before any device is looked for, and the self test needs
    a device (ACG_ENODEV: there is no CPU fallback)"""
    from acarsdec_amd import _capi as K, _build
    L = K.load()
    names = ("acg_json_enable", "acg_drain_json", "acg_collect_json", "acg_selftest_msg_json", "acg_lab_json_level_guard")
    declared = _build.declared_symbols()
    for name in names:
        assert hasattr(L, name) and name in declared, name
    good = K.JsonConfig(1700000000, 0, b"STN1", b"acarsdec", b"3.7")
    nb, nl = C.c_size_t(0), C.c_int(0)
    buf = C.create_string_buffer(K.JSON_LINE_MAX)
    assert K.JSON_LINE_MAX % 64 == 0 and K.JSON_LINE_MAX == JM.LINE_MAX
    assert L.acg_json_enable(None, C.byref(good), None) == K.EINVAL
    assert L.acg_drain_json(None, buf, len(buf), C.byref(nb), C.byref(nl)) == K.EINVAL
    assert L.acg_collect_json(None, 0, buf, len(buf), C.byref(nb), C.byref(nl)) == K.EINVAL
    recs = (K.Msg * 1)()
    for bad in (K.JsonConfig(999999999, 0, b"", b"a", b"1"), K.JsonConfig(4000000000, 0, b"", b"a", b"1"), K.JsonConfig(1700000000, 1000000, b"", b"a", b"1"),
                K.JsonConfig(1700000000, -1, b"", b"a", b"1")):
        assert L.acg_selftest_msg_json(recs, 1, None, C.byref(bad), None, 1, buf, len(buf), C.byref(nb), C.byref(nl)) == K.EINVAL
    assert L.acg_selftest_msg_json(recs, 1, None, None, None, 1, buf, len(buf), C.byref(nb), C.byref(nl)) == K.EINVAL
    assert L.acg_selftest_msg_json(recs, 1, None, C.byref(good), None, 0, buf, len(buf), C.byref(nb), C.byref(nl)) == K.EINVAL
    recs[0].chn = 3                                           # outside nch
    assert L.acg_selftest_msg_json(recs, 1, None, C.byref(good), None, 3, buf, len(buf), C.byref(nb), C.byref(nl)) == K.EINVAL
    recs[0].chn = 0
    rc = L.acg_selftest_msg_json(recs, 1, None, C.byref(good), None, 1, buf, len(buf), C.byref(nb), C.byref(nl))
    assert rc == (K.OK if L.acg_device_count() > 0 else K.ENODEV)


def test_json_kernels_use_no_scratch_and_stay_inside_their_budget():
    """json.hip as the product builds it: no scratch in any kernel (no indexed private arrays: fields are read out of LDS, digits
    are computed), the render kernel's registers and LDS where DESIGN.md 4 states them (two waves, a record and a row each)"""
    import re
    from acarsdec_amd import _build as B
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    assert hipcc, "hipcc"
    csrc = os.path.join(ROOT, "acarsdec_amd", "csrc")
    flags = next(f for name, f, _ in B.UNITS if name == "json.hip")
    assert "-O3" in flags and "-ffp-contract=off" in flags
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include")] +
                       flags + ["-S", "-o", "-", os.path.join(csrc, "json.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", r.stdout, flags=re.M)
    # (the unit's own two: keys and scan are outs.hip's, tests/test_outputs_host.py)
    assert sorted(n.split("json_")[1].split("_kernel")[0] for n in names) == ["measure", "render"], names
    scratch = [int(v) for v in re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", r.stdout)]
    assert len(scratch) == 2 and not any(scratch), scratch
    assert "scratch_" not in r.stdout
    lds = [int(v) for v in re.findall(r"\.amdhsa_group_segment_fixed_size (\d+)", r.stdout)]
    assert max(lds) <= 2 * (384 + 2496 + 16), lds
    vgpr = [int(v) for v in re.findall(r"\.amdhsa_next_free_vgpr (\d+)", r.stdout)]
    assert max(vgpr) <= 128, vgpr
