"""The outputs (acg_outputs_enable / acg_drain_outputs), the parts that need no GPU: acg_outputs_config_check on every rule (host
arithmetic), the code object of csrc/outs.hip as the product builds it (no scratch, the register and LDS figures DESIGN.md
states), and the per-leg merge of three ranks' legs by ONE key list (shard.merge_keyed as it is)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np

from conftest import ROOT
from acarsdec_amd import _capi as K, decoder as D, shard
import json_model as JM
import text_model as TM

T0 = (1792301725, 269667)


def check(cfg):
    return K.load().acg_outputs_config_check(C.byref(cfg))


def test_config_check_holds_every_rule_without_a_device():
    L = K.load()
    assert L.acg_outputs_config_check(None) == K.EINVAL
    good = [["msgs"], ["json"], ["oneline", "sv"], ["msgs", "json", "oneline", "std"], ["oneline", "std", "pp", "sv"],
            [("oneline", dict(date=True)), ("std", dict(date=True, freq=True)), "json"], [("std", dict(freq=True))]]
    for legs in good:
        assert check(D.outputs_config(legs, T0, "STN1", "acarsdec", "3.7")) == K.OK, legs
    # the number of legs
    cfg = D.outputs_config(["json"], T0)
    for n in (0, -1, K.OUT_LEGS_MAX + 1):
        cfg.nlegs = n
        assert check(cfg) == K.EINVAL, n
    # an unknown kind
    for kind in (0, 5, 0x11, 0x30, -1):
        assert check(D.outputs_config([(kind, 0)], T0)) == K.EINVAL, kind
        assert check(D.outputs_config(["json", (kind, 0)], T0)) == K.EINVAL, kind
    # a flag the kind does not take
    for leg in ((K.OUT_MSGS, 1), (K.OUT_JSON, K.TEXT_F_DATE), (K.TEXT_ONELINE, K.TEXT_F_FREQ), (K.TEXT_PP, K.TEXT_F_DATE), (K.TEXT_SV, K.TEXT_F_FREQ),
                (K.TEXT_STD, 4), (K.TEXT_STD, 8)):
        assert check(D.outputs_config([leg], T0)) == K.EINVAL, leg
    # duplicate kinds, flags or not
    for legs in (["msgs", "msgs"], ["json", "std", "json"], ["std", ("std", dict(date=True))], ["pp", "sv", "oneline", "pp"]):
        assert check(D.outputs_config(legs, T0)) == K.EINVAL, legs
    # the epoch: the sinks' own bounds, for every kind of leg
    for legs in (["msgs"], ["json"], ["sv"]):
        for t0 in ((999999999, 0), (4000000000, 0), (1700000000, 1000000), (1700000000, -1)):
            cfg = D.outputs_config(legs, T0)
            cfg.t0_sec, cfg.t0_usec = t0
            assert check(cfg) == K.EINVAL, (legs, t0)
        for t0 in ((10 ** 9, 0), (3999999999, 999999)):
            cfg = D.outputs_config(legs, T0)
            cfg.t0_sec, cfg.t0_usec = t0
            assert check(cfg) == K.OK, (legs, t0)
    # an unterminated string
    for field, size in (("station_id", 33), ("app_name", 17), ("app_ver", 17)):
        cfg = D.outputs_config(["msgs", "json"], T0)
        C.memset(C.addressof(cfg) + getattr(K.OutputsConfig, field).offset, 0x41, size)
        assert check(cfg) == K.EINVAL, field
        C.memset(C.addressof(cfg) + getattr(K.OutputsConfig, field).offset + size - 1, 0, 1)
        assert check(cfg) == K.OK, field
    # the ABI the ctypes view relies on
    assert C.sizeof(K.OutLeg) == 8 and C.sizeof(K.OutBuf) == 40 and K.OutputsConfig.t0_sec.offset == 40 and C.sizeof(K.OutputsConfig) == 120


# DESIGN.md 4 states these: VGPRs and LDS bytes per kernel of outs.hip as the product builds it
BUDGET = {"keys": (8, 0), "sum": (6, 264), "offsets": (21, 24), "gather": (12, 0)}


def test_outs_kernels_use_no_scratch_and_keep_their_budget():
    """outs.hip compiled with the product's flags (text.hip's): a private segment of 0 bytes for every kernel, no scratch
    instruction, VGPRs at or below and LDS equal to the figures DESIGN.md states"""
    from acarsdec_amd import _build as B
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    assert hipcc, "hipcc"
    csrc = os.path.join(ROOT, "acarsdec_amd", "csrc")
    flags = {name: (f, prod) for name, f, prod in B.UNITS}
    # text.hip's code generation; the unit's four small kernels travel as a compressed bundle (two pages of the library, not five)
    assert flags["outs.hip"] == (flags["text.hip"][0] + ["--offload-compress"], True)
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include")] +
                       flags["outs.hip"][0] + ["-S", "-o", "-", os.path.join(csrc, "outs.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = [re.search(r"outs_(\w+?)_kernel", n).group(1) for n in re.findall(r"^\s*\.amdhsa_kernel (\S+)", r.stdout, flags=re.M)]
    scratch = [int(v) for v in re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", r.stdout)]
    vgpr = [int(v) for v in re.findall(r"\.amdhsa_next_free_vgpr (\d+)", r.stdout)]
    lds = [int(v) for v in re.findall(r"\.amdhsa_group_segment_fixed_size (\d+)", r.stdout)]
    print("outs.hip kernels:", list(zip(names, vgpr, lds, scratch)))
    assert sorted(names) == sorted(BUDGET) and len(scratch) == len(BUDGET) and not any(scratch), (names, scratch)
    assert "scratch_" not in r.stdout
    for n, v, l in zip(names, vgpr, lds):
        assert v <= BUDGET[n][0] and l == BUDGET[n][1], (n, v, l)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for n, (v, l) in BUDGET.items():
        assert re.search(r"outs_%s_kernel\s*\|\s*%d\s*\|\s*%d\s*\|" % (n, v, l), design), n


def test_three_ranks_legs_merge_per_leg_by_one_key_list():
    """Messages on six channels, `c mod 3` over three ranks.  Every rank's legs (the acg_msg bytes, json_model's line, text_model's
    -o 2 record and -n packet of its messages in key order) and its ONE key list; shard.merge_keyed applied per leg with that list
    gives, for every leg, the single stream over all channels -- the same permutation, so record i stays the same message."""
    rng = np.random.default_rng(77)
    nch, n = 6, 200
    msgs = []
    for i, eb in enumerate(rng.permutation(4 * n)[:n]):
        m = K.Msg()
        m.chn, m.end_bit, m.err, m.lvl = int(rng.integers(0, nch)), int(eb), int(rng.integers(0, 3)), float(np.float32(rng.uniform(-40, 5)))
        m.end_sample = int(eb) * 5 + 3000
        m.soh_sample = m.end_sample - int(rng.integers(100, 2500))
        m.mode, m.ack, m.bid, m.addr, m.label, m.no, m.fid = b"2", b"!", b"%d" % (i % 10), b".N%05d" % i, b"H1", b"D%03d" % (i % 1000), b"XY%04d" % (i % 10000)
        txt = bytes(rng.integers(0x20, 0x7F, int(rng.integers(0, 243)), dtype=np.uint8))
        m.txt, m.txt_len, m.bs, m.be, m.down = (C.c_ubyte * 242)(*txt), len(txt), b"\x02", b"\x03", b"\x01"
        msgs.append(m)
    key = lambda m: (m.chn << K.SINK_KEY_END_BITS) | m.end_bit

    def legs_of(ms):
        ms = sorted(ms, key=key)
        ts = lambda m: JM.print_number(JM.tv_double(*JM.tv(T0, m.soh_sample))).encode()
        return ([key(m) for m in ms],
                [[bytes(m) for m in ms],
                 [JM.line(m, m.chn, ts(m), station=b"STN1", app=(b"acarsdec", b"3.7")) for m in ms],
                 [TM.record(m, m.chn, TM.STD, TM.F_DATE, t0=T0) for m in ms],
                 [TM.record(m, m.chn, TM.SV, 0, t0=T0, station=b"STN1") for m in ms]])

    wkeys, want = legs_of(msgs)
    assert len(set(wkeys)) == n
    ranks = [legs_of([m for m in msgs if m.chn % 3 == r]) for r in range(3)]
    assert all(len(k) > 10 for k, _ in ranks)
    for l in range(4):
        assert shard.merge_keyed([(k, legs[l]) for k, legs in ranks]) == want[l], l
    assert shard.merge_keyed([(k, k) for k, _ in ranks]) == wkeys
    assert len({len(r) for r in want[1]}) > 10 and len({len(r) for r in want[2]}) > 10      # (the legs' records really differ in length)
