"""The text sink without a GPU: the Python model of the reference's text formats (tests/text_model.py) against the bytes the
reference program printed for the text fixture (tests/golden/msgtext_golden.json, made by tests/golden/make_msgtext_golden.py),
the date against the C library's gmtime, the kernel's own integer arithmetic (csrc/text_num.h, compiled for the host) against
glibc, the ABI of the new entry points, and the code object's budget."""
import ctypes as C
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import label_model as LM
import text_model as TM

sys.path.insert(0, GOLDEN)
import make_msgtext_golden as MG  # noqa: E402

VARIANTS = ("none", "A", "e", "b", "Aeb")


@pytest.fixture(scope="module")
def fix():
    pcm = np.load(os.path.join(GOLDEN, "msgjson_pcm16.npz"))["pcm"]
    with open(os.path.join(GOLDEN, "msgjson_golden.json")) as f:
        gj = json.load(f)
    with open(os.path.join(GOLDEN, "msgtext_golden.json")) as f:
        gt = json.load(f)
    return pcm, gj, gt


def split_frames(frames):
    from oracle import oracle as O
    out = []
    for f in frames:
        b = O.blk_process(f)
        if b is not None:
            out.append(O.msg_split(b))
    return out


@pytest.fixture(scope="module")
def oracle_msgs(fix):
    """per channel: the split records of the fixture from the oracle's restatement of demodulator, framing, repair and split"""
    from oracle import oracle as O
    pcm, gj, _ = fix
    out = []
    for c in range(gj["nch"]):
        ch = O.Channel(c, max_frames=256)
        x = pcm[c].astype(np.float32) / np.float32(32768.0)
        for s in range(0, x.size, 4096):
            ch.demod(x[s:s + 4096])
        out.append(split_frames(ch.frames))
    return out


def filter_kw(gj, variant):
    args = gj["variants"][variant]["args"]
    return dict(downlink_only="-A" in args, skip_empty="-e" in args, labels=LM.parse_label_filter(gj["label_list"]) if "-b" in args else ())


def first_difference(mine, want):
    return next(((i, a, b) for i, (a, b) in enumerate(zip(mine + [None], want + [None])) if a != b), None)


def test_fixture_holds_the_cases_that_decide_bytes(fix):
    """as many records per variant as the JSON fixture has lines, nothing but records in the reference's stdout, and the cases
    that decide bytes are there: a NUL mode ("%1c"), Nak, a record without block id, ETB, an empty text, decoded labels, a
    one-character label padded by "%2s", a short message number padded by "%4s" """
    _, gj, gt = fix
    for v in VARIANTS:
        o1, o2 = bytes.fromhex(gt["variants"][v]["o1"]), bytes.fromhex(gt["variants"][v]["o2"])
        n = len(gj["variants"][v]["lines"])
        assert gt["variants"][v]["records"] == n and gt["variants"][v]["args"] == gj["variants"][v]["args"]
        assert len(TM.split_oneline(o1)) == n and len(TM.split_std(o2)) == n and b"".join(TM.split_std(o2)) == o2
    o1, o2 = bytes.fromhex(gt["variants"]["none"]["o1"]), bytes.fromhex(gt["variants"]["none"]["o2"])
    for piece in (b"Mode : \0 Label", b"Nak\n", b"Ack : K\n", b"\nETB\n", b"#" * 26 + b"\n", b"Destination Airport : ", b"Departure Airport : ",
                  b"Estimation Time of Arrival : ", b"Gate out Time : ", b"Gate in Time : ", b"Wheels off Tme : ", b"Wheels on Time : ",
                  b"Label :  5 ", b"No:   M0", b"Label : Qd "):
        assert piece in o2, piece
    assert any(b"Id : " not in r for r in TM.split_std(o2)) and b" \0 " in o1 and b"F:" not in o2.split(b"L:")[0]
    assert not re.search(TM.DATE_RE, o1) and not re.search(TM.DATE_RE, o2)          # the file front end prints no date


def test_model_reproduces_the_reference_bytes_of_o1_and_o2(fix, oracle_msgs):
    """Every variant, every channel, both formats: the model's record of each message the filters keep equals the bytes the
    reference printed.  The number of records compared is the fixture's count: nothing is left out."""
    _, gj, gt = fix
    compared = {}
    for v in VARIANTS:
        kw = filter_kw(gj, v)
        for fmt, key, split in ((TM.ONELINE, "o1", TM.split_oneline), (TM.STD, "o2", TM.split_std)):
            ref = split(bytes.fromhex(gt["variants"][v][key]))
            total = 0
            for c in range(gj["nch"]):
                want = [r for r in ref if TM.chn_of(r) == c]
                mine = [TM.record(m, c, fmt) for m in oracle_msgs[c] if TM.keep(m, **kw)]
                assert mine == want, (v, key, c, first_difference(mine, want))
                total += len(mine)
            assert total == len(ref) == gt["variants"][v]["records"] == len(gj["variants"][v]["lines"])
            compared[(v, key)] = total
            assert max(len(r) for r in ref) <= TM.REC_MAX
    print("records compared:", compared)
    assert compared[("none", "o1")] == compared[("none", "o2")] == len(gj["sent"]) == 68


@pytest.fixture(scope="module")
def rtl_leg(fix):
    """the rtl leg's I/Q regenerated from the committed recording, and the oracle's messages of its four channels"""
    from oracle import oracle as O
    from acarsdec_amd import decoder as D
    pcm, _, gt = fix
    g = gt["rtl"]
    iq, fc, fr = MG.rtl_iq(pcm, g["blocks"], g["tail_blocks"], g["freqs"], g["M"], g["phases"])
    assert fc == g["Fc"] and hashlib.sha256(iq.tobytes()).hexdigest() == g["iq_sha256"], "the synthetic I/Q differs from the fixture's"
    msgs = []
    for c in range(len(fr)):
        ch = O.Channel(c, max_frames=256)
        ch.demod(O.fir_u8(iq, g["M"], D.rtl_taps(fr[c], fc, g["M"])))
        msgs.append(split_frames(ch.frames))
    return fr, msgs


def test_model_with_date_and_freq_equals_the_rtl_leg(fix, rtl_leg):
    """printmsg() behind rtl.c prints "F:%3.3f " and the date: the model with F_DATE | F_FREQ against the reference's bytes, the
    date's digits masked on both sides (the reference stamps its wall clock)"""
    _, _, gt = fix
    fr, msgs = rtl_leg
    ref = TM.split_std(bytes.fromhex(gt["rtl"]["o2_masked"]))
    total = 0
    for c in range(len(fr)):
        want = [r for r in ref if TM.chn_of(r) == c]
        mine = [TM.mask_dates(TM.record(m, c, TM.STD, TM.F_DATE | TM.F_FREQ, fr_hz=fr[c])) for m in msgs[c]]
        assert mine == want, (c, first_difference(mine, want))
        total += len(mine)
    assert total == len(ref) == gt["rtl"]["records"] >= 6
    assert len({r[:14] for r in ref}) >= 3                      # three channels, three "F:" tokens


def test_oneline_with_date_equals_the_existing_rtl_program_fixture(golden, testwav):
    """testwav_golden.json's program_rtl leg is `-o 1 -r 0` with "<date> " cut out: the model's one-line format with F_DATE, cut
    the same way, on the oracle's messages of the same synthetic I/Q"""
    from oracle import oracle as O
    from acarsdec_amd import decoder as D, synth as S
    g, pr = golden["rtl"], golden["program_rtl"]
    fr = [int(round(float(f) * 1e6)) for f in g["freqs"]]
    env = S.pad_blocks(0.5 + 0.5 * testwav.T.astype(np.float64), 1024, 0.5)
    env = np.concatenate([env, np.full((4, 1024 * pr["tail_blocks"]), 0.5)], axis=1)
    iq = S.iq_u8_from_envelopes(env, g["M"], [f - g["Fc"] for f in fr], phases=g["phases"])
    assert hashlib.sha256(iq.tobytes()).hexdigest() == pr["iq_sha256"]
    want = TM.split_oneline(pr["stdout_no_timestamps"].encode("latin-1"))
    assert len(want) == 7
    total = 0
    for c in range(4):
        ch = O.Channel(c, max_frames=64)
        ch.demod(O.fir_u8(iq, g["M"], D.rtl_taps(fr[c], g["Fc"], g["M"])))
        lines = [TM.record(m, c, TM.ONELINE, TM.F_DATE) for m in split_frames(ch.frames)]
        assert all(re.search(TM.DATE_RE + rb" ", ln) for ln in lines)
        mine = [re.sub(TM.DATE_RE + rb" ", b"", ln) for ln in lines]
        assert mine == [w for w in want if TM.chn_of(w) == c], c
        total += len(mine)
    assert total == 7


def gmtime_text(sec, usec):
    t = time.gmtime(sec)
    return b"%02d/%02d/%04d %02d:%02d:%02d.%03d" % (t.tm_mday, t.tm_mon, t.tm_year, t.tm_hour, t.tm_min, t.tm_sec, usec // 1000)


NAMED_SECONDS = TM.NAMED_SECONDS


def test_model_date_equals_gmtime():
    rng = np.random.default_rng(2100)
    assert gmtime_text(4107542399, 0).startswith(b"28/02/2100 23:59:59") and gmtime_text(4107542400, 0).startswith(b"01/03/2100 00:00:00")
    assert gmtime_text(4233686400, 0).startswith(b"29/02/2104") and gmtime_text(2 ** 31, 0).startswith(b"19/01/2038 03:14:08")
    secs = list(NAMED_SECONDS) + rng.integers(10 ** 9, 4_800_000_000, 4000).tolist()
    for s in secs:
        for u in (0, 999, 1000, 999999, int(rng.integers(0, 10 ** 6))):
            assert TM.date_text(s, u) == gmtime_text(s, u), (s, u)
    assert TM.date_text(4107542400, 999999) == b"01/03/2100 00:00:00.999"


def test_level_and_int_printers_equal_the_c_library():
    rng = np.random.default_rng(7)
    vals = [0.05, -0.05, 0.25, -0.25, 0.35, -0.35, -0.04, 0.0, -0.0, np.inf, -np.inf, np.nan, 9.95, -9.95, 99.95, -999.95, 3240.1, -7.9]
    vals += (rng.integers(-100000, 100001, 20000) / 20.0).tolist() + rng.uniform(-3300, 3300, 20000).tolist()
    for x in vals:
        f = np.float32(x)
        assert TM.level_text(f) == TM.level_libc(f), repr(f)
    assert TM.level_text(np.float32(-0.04)) == b" -0.0" and TM.level_text(np.float32(0.25)) == b" +0.2" and TM.level_text(np.float32(-12.34)) == b"-12.3"
    assert TM.level_text(np.float32(np.inf)) == b" +inf" and TM.level_text(np.copysign(np.float32(np.nan), np.float32(-1))) == b" -nan"
    assert b"%03d" % TM.trunc_int(-7.9) == b"-07" and b"%03d" % TM.trunc_int(7.9) == b"007" and TM.trunc_int(np.nan) == TM.trunc_int(np.inf) == -2 ** 31
    assert TM.freq_token(131725000) == b"F:131.725 " and TM.freq_token(0) == b"F:0.000 " and TM.freq_token(131550000) == b"F:131.550 "


class Rec:
    """a record for the model's own cases"""
    def __init__(self, **kw):
        d = dict(chn=0, err=0, lvl=-12.34, txt_len=0, soh_sample=0, mode=b"2", addr=b".N12345", ack=b"!", label=b"H1", bid=b"3", no=b"M01A",
                 fid=b"XY0123", be=b"\x03", txt=b"")
        d.update(kw)
        d["txt_len"] = kw.get("txt_len", len(d["txt"]))
        self.__dict__.update(d)


def test_pp_and_sv_restate_one_snprintf_each():
    """PP and SV have no reference capture, because they leave through a socket and no test here opens one.  Their model is a
    literal restatement of one snprintf each (netout.c:112-114 and 130-135); these are that snprintf's bytes worked out by hand."""
    m = Rec(txt=b"LINE1\r\nLINE2\0HIDDEN", lvl=-7.9, err=2)
    assert TM.pp(m) == b"AC2 .N12345 ! H1 3 M01A XY0123 LINE1  LINE2"
    assert TM.sv(m, 4, 4107542400, b"STN1") == b"    STN1 5 01/03/2100 00:00:00 2 -07 2 .N12345 ! H1 3 M01A XY0123 LINE1\r\nLINE2"
    up = Rec(mode=b"\0", addr=b"N1", ack=b"K", label=b"5", bid=b"\0", no=b"", fid=b"", txt=b"", lvl=np.inf)
    assert TM.pp(up) == b"AC\0      N1 K  5 .             "
    assert TM.sv(up, 0, 10 ** 9, b"A-VERY-LONG-STATION") == b"A-VERY-LONG-STATION 1 09/09/2001 01:46:40 0 -2147483648 \0      N1 K  5 .             "
    # the longest record of any format is printmsg()'s: the header's derivation, token by token
    o = {f: b"ABCD" for f, _ in TM.OOOI_LINES}
    big = Rec(chn=2 ** 31 - 2, err=-2 ** 31, lvl=-8.9e17, txt=b"T" * 242, be=b"\x17", ack=b"K")
    n = len(TM.std(big, big.chn, TM.date_text(10 ** 9, 0), b"F:-2147.484 ", (1, o)))
    assert n == 653 - 1 and (653 + 63) // 64 * 64 == TM.REC_MAX            # (chn + 1 = 2147483647 has ten characters, the bound counts eleven)


def test_the_kernels_date_and_level_printers_equal_glibc(tmp_path):
    """csrc/text_num.h is what text.hip compiles for the device; tests/text_num_check.cpp compiles the same functions for the
    host and holds them against gmtime_r + snprintf over the named seconds, a dense sweep through 2122 and random seconds, and
    against "%+5.1f" / "%03d" over ties, signed zeros, non-finite values and random floats."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path / "text_num_check")
    r = subprocess.run([cxx, "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "acarsdec_amd", "csrc"), os.path.join(ROOT, "tests", "text_num_check.cpp"),
                        "-o", exe, "-lm"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe, "200000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:]


def test_abi_exports_the_text_entry_points():
    """the new symbols are exported and declared; argument errors come before any device is looked for, and the self test needs
    a device (ACG_ENODEV: there is no CPU fallback)"""
    from acarsdec_amd import _capi as K, _build, decoder as D
    L = K.load()
    declared = _build.declared_symbols()
    for name in ("acg_text_enable", "acg_drain_text", "acg_collect_text", "acg_selftest_msg_text", "acg_lab_text_level_guard"):
        assert hasattr(L, name) and name in declared, name
    hdr = open(os.path.join(ROOT, "include", "acarsdec_amd.h")).read()
    assert int(re.search(r"#define ACG_TEXT_REC_MAX\s+(\d+)", hdr).group(1)) == K.TEXT_REC_MAX == TM.REC_MAX and K.TEXT_REC_MAX % 64 == 0
    assert (K.TEXT_ONELINE, K.TEXT_STD, K.TEXT_PP, K.TEXT_SV, K.TEXT_F_DATE, K.TEXT_F_FREQ) == (TM.ONELINE, TM.STD, TM.PP, TM.SV, TM.F_DATE, TM.F_FREQ)
    good = D.text_config("std", (1700000000, 0), date=True, freq=True)
    nb, nr = C.c_size_t(0), C.c_int(0)
    buf, offs = C.create_string_buffer(K.TEXT_REC_MAX), (C.c_uint * 2)()
    assert L.acg_text_enable(None, C.byref(good), None) == K.EINVAL
    assert L.acg_drain_text(None, buf, len(buf), C.byref(nb), offs, 1, C.byref(nr)) == K.EINVAL
    assert L.acg_collect_text(None, 0, buf, len(buf), C.byref(nb), offs, 1, C.byref(nr)) == K.EINVAL
    recs = (K.Msg * 1)()
    call = lambda cfg, nch=1: L.acg_selftest_msg_text(recs, 1, None, C.byref(cfg) if cfg is not None else None, None, nch, buf, len(buf),
                                                      C.byref(nb), offs, C.byref(nr))
    bad = [K.TextConfig(0, 0, 1700000000, 0, b""), K.TextConfig(5, 0, 1700000000, 0, b""),                   # unknown formats
           K.TextConfig(K.TEXT_ONELINE, K.TEXT_F_FREQ, 1700000000, 0, b""), K.TextConfig(K.TEXT_PP, K.TEXT_F_DATE, 1700000000, 0, b""),
           K.TextConfig(K.TEXT_SV, K.TEXT_F_DATE, 1700000000, 0, b""), K.TextConfig(K.TEXT_STD, 4, 1700000000, 0, b""),   # flags the format does not take
           K.TextConfig(K.TEXT_STD, 0, 999999999, 0, b""), K.TextConfig(K.TEXT_STD, 0, 4000000000, 0, b""),
           K.TextConfig(K.TEXT_STD, 0, 1700000000, 1000000, b""), K.TextConfig(K.TEXT_STD, 0, 1700000000, -1, b"")]
    unterminated = K.TextConfig(K.TEXT_SV, 0, 1700000000, 0, b"")
    C.memset(C.byref(unterminated, K.TextConfig.station_id.offset), ord("S"), 33)
    for cfg in bad + [unterminated, None]:
        assert call(cfg) == K.EINVAL
    assert call(good, nch=0) == K.EINVAL
    recs[0].chn = 3                                           # outside nch
    assert call(good, nch=3) == K.EINVAL
    recs[0].chn = 0
    assert call(good) == (K.OK if L.acg_device_count() > 0 else K.ENODEV)


def test_text_kernels_use_no_scratch():
    """text.hip as the product builds it: a private segment (scratch) of 0 bytes for every kernel; the register counts and the
    LDS are recorded (printed) and held inside the budget of two waves per workgroup, a record and a row each"""
    from acarsdec_amd import _build as B
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    assert hipcc, "hipcc"
    csrc = os.path.join(ROOT, "acarsdec_amd", "csrc")
    flags = next(f for name, f, _ in B.UNITS if name == "text.hip")
    assert "-O3" in flags and "-ffp-contract=off" in flags
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include")] +
                       flags + ["-S", "-o", "-", os.path.join(csrc, "text.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", r.stdout, flags=re.M)
    # (the unit's own two: keys and scan are outs.hip's, tests/test_outputs_host.py)
    assert sorted(n.split("text_")[1].split("_kernel")[0] for n in names) == ["measure", "render"], names
    scratch = [int(v) for v in re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", r.stdout)]
    vgpr = [int(v) for v in re.findall(r"\.amdhsa_next_free_vgpr (\d+)", r.stdout)]
    lds = [int(v) for v in re.findall(r"\.amdhsa_group_segment_fixed_size (\d+)", r.stdout)]
    print("text.hip kernels:", list(zip(names, vgpr, lds, scratch)))
    assert len(scratch) == 2 and not any(scratch), scratch
    assert "scratch_" not in r.stdout
    assert max(lds) <= 2 * (384 + TM.REC_MAX + 16), lds
    assert max(vgpr) <= 128, vgpr
