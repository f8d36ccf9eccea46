"""The outputs (acg_outputs_enable, acg_drain_outputs / acg_collect_outputs; csrc/outs.hip): a take of blocks consumed ONCE and
handed out as up to four legs rendered from the same kept records in the same order.  The legs against the reference program's
bytes for the fixture; their alignment (record i of every leg the same message, one key list); each leg against its own entry
point in a twin context; designed records through the lab entry against the sinks' own lab entries; ACG_EAGAIN by every bound;
collect with a lag; the side effects of a take happening once; state and argument errors; three sharded contexts merged per leg.
GPU box only."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN
import json_model as JM
import text_model as TM
from outputs_records import NCH_LAB, T0_LAB, TEXT_LENS_WANTED, equal_key_pairs, lab_records

pytestmark = pytest.mark.gpu

VARIANTS = ("none", "A", "e", "b", "Aeb")
T0 = (1792301725, 269667)
CHUNK = 4096
FR = [131725000, 131525000, 129125000]


@pytest.fixture(scope="module")
def D():
    from acarsdec_amd import decoder
    from acarsdec_amd import _capi as K
    assert K.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return decoder


@pytest.fixture(scope="module")
def fix():
    pcm = np.load(os.path.join(GOLDEN, "msgjson_pcm16.npz"))["pcm"]
    with open(os.path.join(GOLDEN, "msgjson_golden.json")) as f:
        gj = json.load(f)
    with open(os.path.join(GOLDEN, "msgtext_golden.json")) as f:
        gt = json.load(f)
    x = pcm.astype(np.float32) / np.float32(32768.0)
    assert x.shape[0] == gj["nch"] == 3 and x.shape[1] % CHUNK == 0
    j = json.loads(gj["variants"]["none"]["lines"][0])
    return x, gj, gt, (j["app"]["name"], j["app"]["ver"])


def new_decoder(D, nch=3, legs=None, station="STN1", app=("acarsdec", "3.7"), freqs_hz=None, **kw):
    dec = D.Decoder(nch, decim=8, ntaps=8, max_blocks=CHUNK // 1024, repair=True, bitlog=False, **kw)
    if legs is not None:
        dec.enable_outputs(legs, T0, station, app[0], app[1], freqs_hz=freqs_hz)
    return dec


def play(dec, x, per_call=None):
    out = []
    for s in range(0, x.shape[1], CHUNK):
        dec.demod_msk(x[:, s:s + CHUNK])
        if per_call:
            out.append(per_call())
    return out


def filter_kw(gj, variant):
    args = gj["variants"][variant]["args"]
    return dict(downlink_only="-A" in args, skip_empty="-e" in args, labels=gj["label_list"] if "-b" in args else None)


def json_chn(ln):
    return int(re.search(rb',"channel":(-?\d+),"freq":', ln).group(1))


def key_of(chn, end_bit):
    return (int(chn) << 44) | int(end_bit)


def joined(calls, nlegs):
    """the per-call leg lists of a run as one list per leg"""
    return [sum((c[l] for c in calls), []) for l in range(nlegs)]


def packed(ms):
    return [bytes(m) + bytes(o) for m, o in ms]


# ---- 1, 2: the reference's bytes from all legs at once, and their alignment ------------------------------------------------
@pytest.mark.parametrize("v", VARIANTS)
def test_all_legs_equal_the_reference_and_index_alike(D, fix, v):
    """Legs {MSGS, JSON, ONELINE, STD} under every filter variant, drained after every call of 4096 samples.  Per channel and in
    order the JSON leg equals the reference program's lines (the time stamp's number cut out, as the JSON sink's test does), the
    ONELINE leg its -o 1 stdout, the STD leg its -o 2 stdout; the counts are the golden's.  Every call hands every leg the same
    number of records, record i names the same channel in all four, and the call's ONE key list is chn << 44 | end_bit of
    msgs[i], strictly ascending."""
    x, gj, gt, app = fix
    dec = new_decoder(D, legs=["msgs", "json", "oneline", "std"], station=gj["station"], app=app)
    dec.set_msg_filter(**filter_kw(gj, v))
    calls = []
    for s in range(0, x.shape[1], CHUNK):
        dec.demod_msk(x[:, s:s + CHUNK])
        more, n, legs = dec.drain_outputs_once()
        keys = dec.sink_keys("outputs")
        assert not more and [len(l) for l in legs] == [n] * 4 and len(keys) == n
        msgs, lines, o1, o2 = legs
        for i in range(n):
            m = msgs[i][0]
            assert json_chn(lines[i]) == m.chn == TM.chn_of(o1[i]) == TM.chn_of(o2[i]), (v, s, i)
            assert int(keys[i]) == key_of(m.chn, m.end_bit), (v, s, i)
        assert all(int(a) < int(b) for a, b in zip(keys, keys[1:]))
        calls.append(legs)
    assert dec.drain_msgs() == []                                # every block was consumed, once
    dec.close()
    msgs, lines, o1, o2 = joined(calls, 4)
    ref = [ln.encode("ascii") + b"\n" for ln in gj["variants"][v]["lines"]]
    ref1 = TM.split_oneline(bytes.fromhex(gt["variants"][v]["o1"]))
    ref2 = TM.split_std(bytes.fromhex(gt["variants"][v]["o2"]))
    assert len(lines) == len(ref) and len(o1) == len(ref1) == len(o2) == len(ref2) == gt["variants"][v]["records"] == len(msgs)
    for c in range(gj["nch"]):
        mine = [JM.cut_timestamp(ln) for ln in lines if json_chn(ln) == c]
        assert [a for a, _ in mine] == [JM.cut_timestamp(ln)[0] for ln in ref if json_chn(ln) == c], (v, c)
        assert [t for _, t in mine] == [JM.print_number(JM.tv_double(*JM.tv(T0, m.soh_sample))).encode() for m, _ in msgs if m.chn == c], (v, c)
        assert [r for r in o1 if TM.chn_of(r) == c] == [r for r in ref1 if TM.chn_of(r) == c], (v, c)
        assert [r for r in o2 if TM.chn_of(r) == c] == [r for r in ref2 if TM.chn_of(r) == c], (v, c)


# ---- 3: each leg equals its own entry point --------------------------------------------------------------------------------
def twin_for(D, leg):
    """a decoder that enables only the sink of `leg`, and the call that drains it as a list of records"""
    dec = new_decoder(D)
    if leg == "msgs":
        return dec, lambda: packed(dec.drain_msgs(oooi=True))
    if leg == "json":
        dec.enable_json(T0, "STATION-9", "acarsdec", "3.7", freqs_hz=FR)
        return dec, lambda: [ln + b"\n" for ln in dec.drain_json().split(b"\n")[:-1]]
    name, flags = leg if isinstance(leg, tuple) else (leg, {})
    dec.enable_text(name, T0, date=bool(flags.get("date")), freq=bool(flags.get("freq")), station_id="STATION-9", freqs_hz=FR)
    return dec, dec.drain_text


@pytest.mark.parametrize("legs", [["msgs", "json", "pp", "sv"], [("oneline", dict(date=True)), ("std", dict(date=True, freq=True))]])
def test_each_leg_equals_its_own_entry_point(D, fix, legs):
    """station and frequencies set; after EVERY call each leg's records (the packed buffer cut at its offset table: offs[0] = 0 and
    offs[n] = nbytes are asserted by the wrapper) are byte-identical to those of a twin decoder that enables only that sink and
    drains after the same calls; the MSGS leg equals drain_msgs(oooi=True), acg_msg and acg_oooi byte for byte"""
    x = fix[0]
    dec = new_decoder(D, legs=legs, station="STATION-9", freqs_hz=FR)
    twins = [twin_for(D, leg) for leg in legs]
    total = 0
    for s in range(0, x.shape[1], CHUNK):
        for d in [dec] + [t for t, _ in twins]:
            d.demod_msk(x[:, s:s + CHUNK])
        got = dec.drain_outputs()
        for l, (leg, (_, drain)) in enumerate(zip(legs, twins)):
            mine = packed(got[l]) if leg == "msgs" else got[l]
            assert mine == drain(), (leg, s)
        total += len(got[0])
    for d in [dec] + [t for t, _ in twins]:
        d.close()
    assert total > 10


# ---- 4: designed records through the lab entry -----------------------------------------------------------------------------
SIZES = (1, 2, 3, 255, 256, 257, 1025)


def selftest_outputs(K, L, D, buf, n, flt, cfg, fr):
    """acg_selftest_outputs with roomy buffers: (nrecs, per leg (bytes, offsets) or [(msg bytes, oooi bytes)])"""
    bufs = (K.OutBuf * cfg.nlegs)()
    keep = []
    for l in range(cfg.nlegs):
        kind = cfg.leg[l].kind
        if kind == K.OUT_MSGS:
            out, extra = (K.Msg * n)(), (K.Oooi * n)()
            bufs[l].cap, bufs[l].oooi = n * C.sizeof(K.Msg), C.addressof(extra)
        else:
            cap = n * (K.JSON_LINE_MAX if kind == K.OUT_JSON else K.TEXT_REC_MAX)
            out, extra = np.full(cap + 64, 0xA5, dtype=np.uint8), np.full(n + 2, 0xA5A5A5A5, dtype=np.uint32)
            bufs[l].cap, bufs[l].offs = cap, extra.ctypes.data
        bufs[l].out = C.addressof(out) if kind == K.OUT_MSGS else out.ctypes.data
        keep.append((out, extra))
    nr = C.c_int(0)
    rc = L.acg_selftest_outputs(buf, n, C.byref(flt) if flt is not None else None, C.byref(cfg), fr.ctypes.data, NCH_LAB, bufs, C.byref(nr))
    assert rc == K.OK, rc
    legs = []
    for l in range(cfg.nlegs):
        out, extra = keep[l]
        if cfg.leg[l].kind == K.OUT_MSGS:
            assert bufs[l].nbytes == nr.value * C.sizeof(K.Msg)
            legs.append([(bytes(out[i]), bytes(extra[i])) for i in range(nr.value)])
        else:
            nb = bufs[l].nbytes
            assert (out[nb:] == 0xA5).all() and extra[nr.value + 1] == 0xA5A5A5A5, "bytes behind the result were written"
            legs.append((out[:nb].tobytes(), extra[:nr.value + 1].tolist()))
    return nr.value, legs


def test_designed_records_equal_the_sinks_own_lab_entries(D):
    """n in 1, 2, 3 (PK_WAVES = 2), 255, 256, 257 (the scan's 256-rank workgroups) and 1025 (the sort's 1024-key tile), with and
    without a filter that drops some, records marked dropped among them: every JSON and text leg of acg_selftest_outputs is
    byte-identical, buffer and table, to acg_selftest_msg_json / _text over the same input (the JSON leg's table against its
    lines' lengths: the JSON lab entry hands out none); the MSGS leg is the kept inputs in key order, equal keys in input order,
    with the acg_oooi acg_selftest_msg_labels decodes.  Asserted over the set: kept records under ONE (chn, end_bit) key that are
    neighbours in rank, inside a 256-rank workgroup and across two; every text length of 0, 1, 58 .. 65, 241, 242 among the kept
    records.  The legs differ in length per record, so each meets its seams at other alignments: over the set every offset mod 16
    occurs in each rendered kind, in every configuration that renders it.  The one-leg configurations are what a sink of its own
    runs: a JSON leg alone, a text leg alone, and the MSGS leg alone (no rendered leg: no scan is launched)."""
    from acarsdec_amd import _capi as K
    L = K.load(lab=True)                                         # (the outputs' lab entries live in the lab library only)
    fr = np.random.default_rng(5).integers(118000000, 137000000, NCH_LAB).astype(np.int32)
    configs = [["msgs", "json", ("oneline", dict(date=True)), ("std", dict(date=True, freq=True))], ["pp", "sv", "json", "msgs"],
               ["json"], ["sv"], ["msgs"]]     # one leg: what a sink of its own runs; ["msgs"] renders nothing (nrender == 0)
    seams, lens, inside, across = {}, set(), 0, 0
    for n in SIZES:
        recs = lab_records(np.random.default_rng(4000 + n), n, K)
        buf = (K.Msg * n).from_buffer_copy(recs.tobytes())
        msgs = [K.Msg.from_buffer_copy(r.tobytes()) for r in recs]
        for fkw in (None, dict(downlink_only=True, skip_empty=True)):
            flt = D.make_msg_filter(**fkw) if fkw else None
            fp = C.byref(flt) if flt is not None else None
            kept_flag, oooi = (C.c_ubyte * n)(), (K.Oooi * n)()
            assert L.acg_selftest_msg_labels(buf, n, fp, kept_flag, oooi) == K.OK
            order = sorted((i for i in range(n) if kept_flag[i] and msgs[i].reserved2 in (b"\x00", 0)), key=lambda i: (msgs[i].chn, msgs[i].end_bit))
            want_msgs = [(recs[i].tobytes(), bytes(oooi[i])) for i in order]
            if n >= 255:
                assert 0 < len(order) < n
            pairs = equal_key_pairs([msgs[i] for i in order])
            inside, across = inside + pairs[0], across + pairs[1]
            lens |= {max(0, min(msgs[i].txt_len, 242)) for i in order}
            for legs in configs:
                cfg = D.outputs_config(legs, T0_LAB, b"S\"1", b"acarsdec", b"3.7")
                nrecs, got = selftest_outputs(K, L, D, buf, n, flt, cfg, fr)
                assert nrecs == len(order), (n, fkw, legs)
                for leg, mine in zip(legs, got):
                    if leg == "msgs":
                        assert mine == want_msgs, (n, fkw)
                        continue
                    nb, nr = C.c_size_t(0), C.c_int(0)
                    if leg == "json":
                        jc = D.json_config(T0_LAB, b"S\"1", b"acarsdec", b"3.7")
                        out = np.zeros(n * K.JSON_LINE_MAX, dtype=np.uint8)
                        assert L.acg_selftest_msg_json(buf, n, fp, C.byref(jc), fr.ctypes.data, NCH_LAB, out.ctypes.data, out.size, C.byref(nb), C.byref(nr)) == K.OK
                        blob = out[:nb.value].tobytes()
                        offs = np.cumsum([0] + [len(ln) + 1 for ln in blob.split(b"\n")[:-1]]).tolist()
                    else:
                        name, flags = leg if isinstance(leg, tuple) else (leg, {})
                        tc = D.text_config(name, T0_LAB, date=bool(flags.get("date")), freq=bool(flags.get("freq")), station_id=b"S\"1")
                        out, table = np.zeros(n * K.TEXT_REC_MAX, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint32)
                        assert L.acg_selftest_msg_text(buf, n, fp, C.byref(tc), fr.ctypes.data, NCH_LAB, out.ctypes.data, out.size, C.byref(nb),
                                                       table.ctypes.data, C.byref(nr)) == K.OK
                        blob, offs = out[:nb.value].tobytes(), table[:nr.value + 1].tolist()
                    assert nr.value == nrecs and mine[1] == offs and mine[0] == blob, (n, fkw, leg)
                    seams.setdefault((configs.index(legs), str(leg)), set()).update(o % 16 for o in offs)
    assert inside > 100 and across >= 2 and set(TEXT_LENS_WANTED) <= lens, (inside, across, sorted(lens))
    rendered = [(c, str(leg)) for c, legs in enumerate(configs) for leg in legs if leg != "msgs"]
    assert len({k for _, k in rendered}) == 5 and sorted(seams) == sorted(rendered)     # five kinds; every rendered leg of every configuration
    assert all(s == set(range(16)) for s in seams.values()), {k: sorted(v) for k, v in seams.items()}


def test_lab_entry_says_again_with_every_legs_size_and_writes_nothing(D):
    """one leg a byte too small: ACG_EAGAIN, every leg's nbytes says what it needs, no byte and no table entry is written"""
    from acarsdec_amd import _capi as K
    L = K.load(lab=True)
    n = 40
    fr = np.zeros(NCH_LAB, dtype=np.int32)
    recs = lab_records(np.random.default_rng(40), n, K)
    buf = (K.Msg * n).from_buffer_copy(recs.tobytes())
    cfg = D.outputs_config(["json", "sv"], T0_LAB)
    nrecs, (js, sv) = selftest_outputs(K, L, D, buf, n, None, cfg, fr)
    bufs = (K.OutBuf * 2)()
    outs = [np.full(len(js[0]), 0xA5, dtype=np.uint8), np.full(len(sv[0]), 0xA5, dtype=np.uint8)]
    tabs = [np.full(n + 1, 0xA5A5A5A5, dtype=np.uint32) for _ in range(2)]
    for l in range(2):
        bufs[l].out, bufs[l].cap, bufs[l].offs = outs[l].ctypes.data, outs[l].size - (1 if l == 1 else 0), tabs[l].ctypes.data
    nr = C.c_int(0)
    assert L.acg_selftest_outputs(buf, n, None, C.byref(cfg), fr.ctypes.data, NCH_LAB, bufs, C.byref(nr)) == K.EAGAIN
    assert (bufs[0].nbytes, bufs[1].nbytes) == (len(js[0]), len(sv[0])) and nr.value == 0
    assert all((o == 0xA5).all() for o in outs) and all((t[1:] == 0xA5A5A5A5).all() for t in tabs)


# ---- 5: ACG_EAGAIN by each binding bound -----------------------------------------------------------------------------------
def side_effects(dec):
    table, lost = dec.stats()
    return [bytes(f) for f in dec.flights()], [bytes(r) for r in dec.drain_routes()], table.tobytes(), lost


@pytest.fixture(scope="module")
def big_run(D, fix):
    """six calls queued, then one drain through roomy buffers: the legs, the keys, the flight table and the statistics"""
    x = fix[0]
    dec = new_decoder(D, legs=["msgs", "json", "std"])
    dec.enable_flights(t0=T0, mdly=600, max_flights=64)
    dec.enable_stats()
    assert dec.max_lag + 1 >= 6                                  # (the block queue holds the calls of acg_max_lag() + 1)
    play(dec, x[:, :6 * CHUNK])
    legs = dec.drain_outputs()
    out = legs, side_effects(dec)
    dec.close()
    assert len(legs[0]) > 10
    return out


@pytest.mark.parametrize("caps,max_recs,limit", [((4096, 5, 4096), 4096, 5), ((4096, 4096, 5), 4096, 5), ((3, 4096, 4096), 4096, 3), ((4096, 4096, 4096), 3, 3)])
def test_every_bound_says_again_and_loses_nothing(D, fix, big_run, caps, max_recs, limit):
    """the JSON leg's buffer for 5 lines, the text leg's for 5 records, the MSGS leg's for 3, max_recs = 3, everything else large:
    ACG_EAGAIN until the queue is empty, every call hands every leg the same count (at most the bound), the concatenation over the
    calls is the big-buffer run's per channel and in order, and the flight table and the statistics end as the big-buffer run's"""
    x = fix[0]
    whole, effects = big_run
    dec = new_decoder(D, legs=["msgs", "json", "std"])
    dec.enable_flights(t0=T0, mdly=600, max_flights=64)
    dec.enable_stats()
    play(dec, x[:, :6 * CHUNK])
    calls, codes = [], []
    for _ in range(len(whole[0]) + 2):
        more, n, legs = dec.drain_outputs_once(max_recs=max_recs, caps=caps)
        assert [len(l) for l in legs] == [n] * 3 and n <= limit
        assert [m.chn for m, _ in legs[0]] == [json_chn(ln) for ln in legs[1]] == [TM.chn_of(r) for r in legs[2]]
        calls.append(legs)
        codes.append(more)
        if not more:
            break
    assert codes[-1] is False and all(codes[:-1]) and len(codes) >= 3
    assert dec.drain_outputs_once(max_recs=max_recs, caps=caps) == (False, 0, [[], [], []])
    got = joined(calls, 3)
    chn = [lambda p: p[0].chn, json_chn, TM.chn_of]
    for l in range(3):
        for c in range(3):                                       # per channel the order is completion order in both
            a, b = [r for r in got[l] if chn[l](r) == c], [r for r in whole[l] if chn[l](r) == c]
            if l == 0:
                a, b = packed(a), packed(b)
            assert a == b, (l, c)
    assert side_effects(dec) == effects
    dec.close()


# ---- 6: collect with a lag ---------------------------------------------------------------------------------------------------
def test_collect_with_lag_equals_drain(D, fix):
    x, gj = fix[0], fix[1]
    legs = ["json", "msgs", "sv"]
    lagging, draining = new_decoder(D, legs=legs, max_lag=1), new_decoder(D, legs=legs)
    got = joined(play(lagging, x, lambda: lagging.collect_outputs(lag=1)) + [lagging.collect_outputs(lag=0)], 3)
    want = joined(play(draining, x, draining.drain_outputs), 3)
    lagging.close()
    draining.close()
    assert len(want[0]) == len(gj["sent"])
    for c in range(3):
        assert [ln for ln in got[0] if json_chn(ln) == c] == [ln for ln in want[0] if json_chn(ln) == c]
        assert packed(p for p in got[1] if p[0].chn == c) == packed(p for p in want[1] if p[0].chn == c)
    assert sorted(got[2]) == sorted(want[2])
    # SV names its channel in no fixed place: its records ride on the JSON leg's order, record i the same message
    assert [got[2][i] for i in range(len(got[2])) if json_chn(got[0][i]) == 1] == [want[2][i] for i in range(len(want[2])) if json_chn(want[0][i]) == 1]


# ---- 7: the side effects of a take happen once -------------------------------------------------------------------------------
def test_four_legs_update_the_flight_table_and_the_statistics_once(D, fix):
    """flight table (mdly 600, 64 slots) and statistics on, four legs: the snapshot (nbm per aircraft included: a message counted
    once per leg would show there), the routes and the statistics equal those of a decoder that plays the fixture through drain_msgs"""
    x = fix[0]
    outs, plain = new_decoder(D, legs=["msgs", "json", "oneline", "pp"]), new_decoder(D)
    for dec in (outs, plain):
        dec.enable_flights(t0=T0, mdly=600, max_flights=64)
        dec.enable_stats()
    play(outs, x, outs.drain_outputs)
    play(plain, x, plain.drain_msgs)
    a, b = side_effects(outs), side_effects(plain)
    nbm = [f.nbm for f in outs.flights()]
    outs.close()
    plain.close()
    assert len(a[0]) > 0 and max(nbm) > 1 and a == b


# ---- 8: state and arguments --------------------------------------------------------------------------------------------------
def raw_call(dec, K, kinds, caps, max_recs, lag=None, drop=None):
    """one C call with buffers of caps[l] bytes; drop: (leg, field) left NULL"""
    bufs = (K.OutBuf * len(kinds))()
    keep = []
    for l, kind in enumerate(kinds):
        out, tab, oo = C.create_string_buffer(max(1, caps[l])), (C.c_uint * (max(max_recs, 0) + 2))(), (K.Oooi * (caps[l] // C.sizeof(K.Msg) + 1))()
        keep.append((out, tab, oo))
        bufs[l].out, bufs[l].cap = C.addressof(out), caps[l]
        if kind == K.OUT_MSGS:
            bufs[l].oooi = C.addressof(oo)
        else:
            bufs[l].offs = C.addressof(tab)
        if drop and drop[0] == l:
            setattr(bufs[l], drop[1], None)
    nr = C.c_int(0)
    if lag is None:
        return dec.L.acg_drain_outputs(dec.ctx, bufs, max_recs, C.byref(nr)), nr.value
    return dec.L.acg_collect_outputs(dec.ctx, lag, bufs, max_recs, C.byref(nr)), nr.value


def test_state_and_argument_errors(D, fix):
    from acarsdec_amd import _capi as K
    x = fix[0]
    kinds = [K.OUT_MSGS, K.OUT_JSON, K.TEXT_STD]
    roomy = [4 * C.sizeof(K.Msg), 4 * K.JSON_LINE_MAX, 4 * K.TEXT_REC_MAX]
    cfg = D.outputs_config(["msgs", "json", "std"], T0, "STN1", "acarsdec", "3.7")
    plain = D.Decoder(3, decim=8, ntaps=8, max_blocks=4, repair=False, bitlog=False)
    assert plain.L.acg_outputs_enable(plain.ctx, C.byref(cfg), None) == K.ESTATE            # no ACG_F_REPAIR
    assert raw_call(plain, K, kinds, roomy, 4)[0] == K.ESTATE and raw_call(plain, K, kinds, roomy, 4, lag=0)[0] == K.ESTATE
    plain.close()
    dec = new_decoder(D)
    dec.demod_msk(x[:, :CHUNK])
    assert raw_call(dec, K, kinds, roomy, 4)[0] == K.ESTATE                                  # before acg_outputs_enable
    keys = np.zeros(4, dtype=np.uint64)
    nk = C.c_int(0)
    assert dec.L.acg_sink_keys(dec.ctx, K.SINK_OUTPUTS, keys.ctypes.data, 4, C.byref(nk)) == K.ESTATE
    bad = D.outputs_config(["msgs", "msgs"], T0)
    assert dec.L.acg_outputs_enable(dec.ctx, C.byref(bad), None) == K.EINVAL
    assert raw_call(dec, K, kinds, roomy, 4)[0] == K.ESTATE                                  # a refused configuration enables nothing
    dec.enable_outputs(["msgs", "json", "std"], T0, "STN1", "acarsdec", "3.7")
    for l, rec in enumerate((C.sizeof(K.Msg), K.JSON_LINE_MAX, K.TEXT_REC_MAX)):             # a leg's cap below its recmax
        caps = list(roomy)
        caps[l] = rec - 1
        assert raw_call(dec, K, kinds, caps, 4)[0] == K.EINVAL and raw_call(dec, K, kinds, caps, 4, lag=0)[0] == K.EINVAL
    assert raw_call(dec, K, kinds, roomy, 0)[0] == K.EINVAL                                  # max_recs < 1
    assert raw_call(dec, K, kinds, roomy, 4, lag=-1)[0] == K.EINVAL
    for drop in ((0, "out"), (0, "oooi"), (1, "offs"), (2, "out")):                          # a missing buffer or table
        assert raw_call(dec, K, kinds, roomy, 4, drop=drop)[0] == K.EINVAL
    assert dec.L.acg_drain_outputs(dec.ctx, None, 4, C.byref(nk)) == K.EINVAL
    first = dec.drain_outputs()                                                              # nothing was consumed by the refused calls
    dec.disable_outputs()
    dec.demod_msk(x[:, CHUNK:2 * CHUNK])
    assert raw_call(dec, K, kinds, roomy, 4)[0] == K.ESTATE                                  # disabled: off again, nothing consumed
    dec.enable_outputs(["msgs", "json", "std"], T0, "STN1", "acarsdec", "3.7")               # ... and on again
    second = dec.drain_outputs()
    dec.reset()                                                                              # acg_reset keeps the configuration
    dec.demod_msk(x[:, :CHUNK])
    again = dec.drain_outputs()
    dec.close()
    twin = new_decoder(D, legs=["msgs", "json", "std"])
    twin.demod_msk(x[:, :CHUNK])
    a = twin.drain_outputs()
    twin.demod_msk(x[:, CHUNK:2 * CHUNK])
    b = twin.drain_outputs()
    twin.close()
    flat = lambda legs: [packed(legs[0]), legs[1], legs[2]]
    assert flat(first) == flat(a) and flat(second) == flat(b) and flat(again) == flat(a) and len(a[0]) + len(b[0]) > 0


def test_individual_sinks_are_untouched_by_enabled_outputs(D, fix):
    """with the outputs enabled (and never drained), drain_msgs / drain_json / drain_text of individually enabled sinks hand out,
    in rotation, the bytes they hand out in a context without the outputs; then the outputs take their turn in the same context"""
    x, gj = fix[0], fix[1]
    with_outs, without = new_decoder(D, legs=["json", "std", "msgs", "sv"]), new_decoder(D)
    for dec in (with_outs, without):
        dec.enable_json(T0, "STN1", "acarsdec", "3.7")
        dec.enable_text("std", T0, date=True)
    ncall = x.shape[1] // CHUNK
    a, b, tail = [], [], 0
    for i in range(ncall):
        for dec in (with_outs, without):
            dec.demod_msk(x[:, i * CHUNK:(i + 1) * CHUNK])
        if i >= ncall - 3:                                       # the last calls go to the outputs: each entry point consumes what it hands out
            tail += len(with_outs.drain_outputs()[0])
            b.append(len(without.drain_msgs()))
            continue
        call = (lambda d: packed(d.drain_msgs(oooi=True)), lambda d: d.drain_json(), lambda d: d.drain_text())[i % 3]
        a.append(call(with_outs))
        b.append(call(without))
    with_outs.close()
    without.close()
    assert a == b[:len(a)] and sum(len(v) for v in a) > 0 and tail == sum(b[len(a):])


# ---- 9: sharded -----------------------------------------------------------------------------------------------------------------
def test_three_sharded_contexts_merge_per_leg_by_the_one_key_list(D, fix):
    """the fixture by three 1-channel contexts under set_channel_numbers, legs {MSGS, JSON, STD}: per round, shard.merge_keyed of
    each leg by the outputs keys equals the single context's leg; the merged keys are the single context's"""
    from acarsdec_amd import shard
    x = fix[0]
    legs = ["msgs", "json", "std"]
    single = new_decoder(D, legs=legs)
    parts = []
    for r in range(3):
        d = new_decoder(D, nch=1, legs=legs)
        d.set_channel_numbers(shard.channel_numbers(1, r, 3))
        parts.append(d)
    total = 0
    for s in range(0, x.shape[1], CHUNK):
        single.demod_msk(x[:, s:s + CHUNK])
        want = single.drain_outputs()
        wkeys = single.sink_keys("outputs")
        got, keys = [], []
        for r, d in enumerate(parts):
            d.demod_msk(x[shard.owned_channels(3, r, 3), s:s + CHUNK])
            got.append(d.drain_outputs())
            keys.append(d.sink_keys("outputs"))
        for l in range(3):
            merged = shard.merge_keyed([(keys[r], got[r][l]) for r in range(3)])
            assert (packed(merged) if l == 0 else merged) == (packed(want[l]) if l == 0 else want[l]), (s, l)
        assert shard.merge_keyed([(k, [int(v) for v in k]) for k in keys]) == [int(v) for v in wkeys]
        total += len(wkeys)
    for d in [single] + parts:
        d.close()
    assert total > 10
