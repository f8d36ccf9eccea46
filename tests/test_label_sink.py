"""The batch sink's filters and label decoding without a GPU: the Python model (tests/label_model.py) against the JSON the
unmodified reference program printed for the label fixture, the fixture's coverage of DecodeLabel()'s dispatch, the C ABI's -b
parser against build_label_filter's token rules, and the argument checks of the new entry points."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from acarsdec_amd import _capi as K, decoder as D
import label_model as M


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "labels_golden.json")) as f:
        return json.load(f)


def sent_label(s):
    return bytes.fromhex(s["label"]).replace(b"\x7f", b"d")


def model_json_view(s):
    """what the model says the reference prints for a transmission: label, text, OOOI keys"""
    txt = bytes.fromhex(s["text"])
    dec, fields = M.decode(sent_label(s), txt, len(txt))
    view = dict(label=M.label_str(sent_label(s)).decode("latin1"), text=txt.split(b"\0")[0].decode("latin1"))
    view.update(M.json_keys(dec, fields))
    return view


def ref_json_view(j):
    view = dict(label=j["label"], text=j.get("text", ""))
    view.update({k: j[k] for k in M.JSON_KEYS.values() if k in j})
    return view


@pytest.mark.parametrize("variant", ["none", "A", "e", "b", "Aeb"])
def test_model_matches_reference_json(fixture, variant):
    """the model's filters keep exactly the messages the reference printed, and its decoder gives their OOOI keys"""
    v = fixture["variants"][variant]
    args = v["args"]
    labels = M.parse_label_filter(fixture["label_list"]) if "-b" in args else ()
    kept = []
    for s in fixture["sent"]:
        txt = bytes.fromhex(s["text"])
        if M.keep(s["down"], sent_label(s), txt, len(txt), downlink_only="-A" in args, skip_empty="-e" in args, labels=labels):
            kept.append(s)
    assert len(kept) == len(v["json"])
    for s, j in zip(kept, v["json"]):
        assert model_json_view(s) == ref_json_view(j), (s, j)
        assert (j.get("block_id", "") in "0123456789") == s["down"]
    if variant == "none":
        assert sum(1 for j in v["json"] if "dsta" in j or "depa" in j or "eta" in j) >= 40      # the keys really are there


def test_fixture_covers_every_dispatch_entry_and_check(fixture):
    cases = {}
    for s in fixture["sent"]:
        cases.setdefault(M.label_str(sent_label(s)).decode("latin1"), []).append((s["what"], s["down"]))
    for lbl, spec in M.TABLE.items():
        got = cases.get(lbl, [])
        assert ("ok", False) in got and ("ok", True) in got, lbl
        if spec == "26":
            want = {"ok:noeta", "fail:ver", "fail:newline", "fail:sch", "fail:slash", "fail:eta"}
        else:
            want = {"fail:guard%d" % g for g in range(len(spec[0]))} | ({"ok:prefix", "fail:prefix"} if spec[2] else set()) | \
                   ({"ok:alt"} if any(len(a) > 1 for _, a in spec[0]) else set())
        assert want <= {w for w, _ in got}, (lbl, want - {w for w, _ in got})
    whats = {s["what"] for s in fixture["sent"]}
    for w in ("del label", "one-char label", "empty text", "text starts with NUL", "embedded NUL"):
        assert w in whats
    # every failure case really fails in the model, every success decodes
    for s in fixture["sent"]:
        txt = bytes.fromhex(s["text"])
        if s["what"].startswith("ok"):
            assert M.decode(sent_label(s), txt, len(txt))[0] == 1, s
        elif s["what"].startswith("fail"):
            assert M.decode(sent_label(s), txt, len(txt))[0] == 0, s


def parse(arg):
    f = K.MsgFilter()
    f.flags = 3
    rc = K.load().acg_parse_label_filter(arg, C.byref(f))
    return rc, [f.labels[i].value for i in range(f.nlabels)], f.flags


@pytest.mark.parametrize("arg", [None, b"", b":", b"::H1:", b"H1", b"H1:Q1:5", b"Q1::44:", b"TOOLONG:H1", b"abc:de:f", b":a::b:"])
def test_parse_label_filter_follows_strtok(arg):
    rc, toks, flags = parse(arg)
    assert rc == K.OK and flags == 3                    # (the flags are the caller's)
    assert toks == [t[:3] for t in M.parse_label_filter(arg)]


def test_parse_label_filter_capacity():
    assert parse(b":".join([b"A%d" % (i % 10) for i in range(64)]))[0] == K.OK
    assert parse(b":".join([b"A"] * 65) + b":")[0] == K.EINVAL
    assert parse(b":".join([b"A"] * 64) + b"::::")[0] == K.OK
    assert K.load().acg_parse_label_filter(b"H1", None) == K.EINVAL
    f = D.make_msg_filter(True, False, "H1::Q1")
    assert f.flags == K.MSGF_DOWNLINK_ONLY and f.nlabels == 2 and f.labels[1].value == b"Q1"


def test_new_entry_points_refuse_bad_arguments():
    L = K.load()
    f = K.MsgFilter()
    n = C.c_int(0)
    buf, oo = (K.Msg * 2)(), (K.Oooi * 2)()
    assert L.acg_set_msg_filter(None, C.byref(f)) == K.EINVAL
    assert L.acg_drain_msgs_oooi(None, buf, oo, 2, C.byref(n)) == K.EINVAL
    assert L.acg_collect_msgs_oooi(None, 1, buf, oo, 2, C.byref(n)) == K.EINVAL
    keep = np.zeros(2, dtype=np.uint8)
    assert L.acg_selftest_msg_labels(buf, -1, None, keep.ctypes.data, oo) == K.EINVAL
    assert L.acg_selftest_msg_labels(buf, 0, None, keep.ctypes.data, oo) == K.OK
    for bad in ("flags", "count", "empty", "unterminated"):
        g = K.MsgFilter()
        g.nlabels = 1
        g.labels[0].value = b"H1"
        if bad == "flags":
            g.flags = 4
        elif bad == "count":
            g.nlabels = 65
        elif bad == "empty":
            g.labels[0].value = b""
        else:
            C.memmove(C.addressof(g.labels[0]), b"ABCD", 4)
        assert L.acg_selftest_msg_labels(buf, 1, C.byref(g), keep.ctypes.data, oo) == K.EINVAL, bad
    assert C.sizeof(K.Oooi) == 40 and K.Oooi.decoded.offset == 35 and C.sizeof(K.MsgFilter) == 8 + 64 * 4


def test_oooi_json_helper():
    o = K.Oooi()
    o.sa, o.da, o.eta = b"KJFK", b"EG", b""
    assert D.oooi_json(None, o) == {}                   # not decoded: nothing, whatever the fields hold
    o.decoded = b"\x01"
    assert D.oooi_json(None, o) == {"depa": "KJFK", "dsta": "EG"}
