"""Time stamps, order and counters after days of uptime.  2^31 samples at 12.5 kHz are 47.7 hours, 2^32 samples 95.4 hours, 2^31
bits 10.4 days; every other GPU test starts at sample 0 and sees a few seconds.  Here the lab hook acg_lab_set_stream_counters
puts a fresh context's 64-bit sample and bit counters (and the 32-bit SOH stamp) where a long run has them:

  a. every demodulator kernel against the oracle preset alike, blocks, stamps and framing state exact after every call;
  b. a channel moved between contexts in the middle of a block, with the wrap of the stamp's 32 bits on either side of the move;
  c. the JSON sink and the flight table on the committed fixtures, the counters shifted by whole seconds and t0 moved back by as
     many: the same bytes as from 0, hence the reference program's;
  d. the sinks' lab entries on records with large counters against the Python models (the time sort and the JSON order sort
     with upper key digits that are not zero and differ inside a batch).

All comparisons are exact.  tests/test_uptime_inputs.py holds the conditions on the traffic.  GPU box only."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
import flight_model as FM
import json_model as JM
import label_model as LM
import test_gpu_flights as TF
import test_gpu_json_sink as TJ
import uptime_traffic as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def D():
    from acarsdec_amd import decoder
    from acarsdec_amd import _capi as K
    assert K.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return decoder


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def S():
    from acarsdec_amd import synth
    return synth


# ---- the hook's contract ------------------------------------------------------------------------------------------------------
def test_stream_counter_hook_contract(D):
    """ACG_EINVAL for a channel range outside the context or a negative value, ACG_ESTATE once a call has been issued since the
    reset; it changes the three counters of the channels named and nothing else"""
    from acarsdec_amd import _capi as K
    dec = D.Decoder(4, decim=8, ntaps=8, max_blocks=1, bitlog=False)
    hook = dec.L.acg_lab_set_stream_counters
    assert hook(None, 0, 1, 5, 5) == K.EINVAL
    for ch0, n in ((-1, 1), (0, 0), (0, 5), (4, 1), (3, 2)):
        assert hook(dec.ctx, ch0, n, 5, 5) == K.EINVAL, (ch0, n)
    assert hook(dec.ctx, 0, 4, -1, 5) == K.EINVAL and hook(dec.ctx, 0, 4, 5, -1) == K.EINVAL
    before = [dec.state(c) for c in range(4)]
    dec.set_stream_counters((1 << 32) - 100, (1 << 32) - 7, ch0=1, n=2)
    after = [dec.state(c) for c in range(4)]
    for a, b in zip(before, after):
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    x = np.full((4, 1024), 0.5, dtype=np.float32)
    dec.demod_msk(x)
    assert hook(dec.ctx, 0, 4, 5, 5) == K.ESTATE
    dec.reset()
    assert hook(dec.ctx, 0, 4, 5, 5) == K.OK                         # right after acg_reset it is allowed again
    dec.close()


# ---- a. demodulator and framing against the oracle, counters preset ---------------------------------------------------------
# (name, ACG_MSK_LPC, ACG_MSK_NOLEAN, bit log, cuts)
KERNELS = [
    ("lean8", 8, 0, False, U.EVEN_CUTS),                 # msk_lean_kernel, 8 lanes per channel (the default)
    ("lean8-bitlog", 8, 0, True, U.EVEN_CUTS),
    ("lean4", 4, 0, False, U.EVEN_CUTS),
    ("lean4-bitlog", 4, 0, True, U.EVEN_CUTS),
    ("demod8", 8, 1, True, U.EVEN_CUTS),                 # msk_demod_kernel
    ("demod2", 2, 0, True, U.EVEN_CUTS),
    ("demod1", 1, 0, True, U.EVEN_CUTS),
    ("demod8-ragged", 8, 0, True, U.RAGGED_CUTS),        # its scalar-refill shape: call lengths that are no multiples of 32
]


@pytest.mark.parametrize("bi", range(len(U.SAMPLE_BASES)), ids=["s%d" % i for i in range(len(U.SAMPLE_BASES))])
@pytest.mark.parametrize("kernel", KERNELS, ids=[k[0] for k in KERNELS])
def test_blocks_and_stamps_equal_the_oracle_at_large_counters(D, tune, kernel, bi):
    """After every call: the drained blocks (text, level, end_bit, end_sample, soh_sample) equal the oracle's with the same
    preset; every channel's framing state is the oracle's, and for the channels inside a block acg_chan_state.soh_back is the
    oracle's distance back to the SOH.  With the block repair on, every delivered message carries its block's three stamps."""
    from acarsdec_amd import _capi as K
    name, lpc, nolean, bitlog, cuts = kernel
    sb = U.SAMPLE_BASES[bi][0]
    bb = U.BIT_BASES[(bi + KERNELS.index(kernel)) % len(U.BIT_BASES)][0]          # paired freely: every pair of kinds occurs
    tune("ACG_MSK_LPC", lpc)
    if nolean:
        tune("ACG_MSK_NOLEAN", "1")
    x = U.traffic()
    want = U.oracle_run(cuts, sb, bb)
    assert sum(len(v) for fr, _, _ in want for v in fr.values()) >= 3 * U.NCH
    maxb = max((b - a + 1023) // 1024 for a, b in zip(cuts[:-1], cuts[1:]))
    for repair in (False, True):
        dec = D.Decoder(U.NCH, decim=8, ntaps=8, max_blocks=maxb, repair=repair, bitlog=bitlog)
        dec.set_stream_counters(sb, bb)
        st = (K.ChanState * U.NCH)()
        nmsg = 0
        for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            frames, states, backs = want[k]
            dec.demod_msk(x[:, a:b])
            if repair:
                # the delivered messages are a subset (blocks the block thread drops are omitted), in order per channel
                got = {}
                for m in dec.drain_msgs():
                    got.setdefault(int(m.chn), []).append((int(m.end_bit), int(m.end_sample), int(m.soh_sample)))
                for c, lst in got.items():
                    assert set(lst) <= {f[6:9] for f in frames.get(c, [])} and lst == sorted(lst), (name, sb, bb, k, c)
                    nmsg += len(lst)
            else:
                got = {}
                for f in dec.drain_frames():
                    got.setdefault(int(f.chn), []).append(U.frame_key(f))
                assert got == frames, (name, sb, bb, k)
            dec._chk(dec.L.acg_get_state_n(dec.ctx, 0, U.NCH, st))
            assert {c: int(st[c].Acarsstate) for c in range(U.NCH)} == states, (name, sb, bb, k)
            assert {c: int(st[c].soh_back) for c in range(U.NCH) if states[c] in (3, 4, 5)} == backs, (name, sb, bb, k)
        dec.close()
        assert not repair or nmsg >= 2 * U.NCH


# ---- b. a channel moved mid-block across the wrap -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_block(O, S):
    """test_channel_moved_mid_block_keeps_its_soh_stamp's signal: one block, and a call boundary strictly inside it"""
    rng = np.random.default_rng(606)
    n = 12 * 1024
    a, _ = S.channel_audio(rng, n, nframes=1, gap=(1500, 1600), text_len=(100, 110))
    x = S.envelope(a, noise=0.003, rng=rng).astype(np.float32)
    ch = O.Channel(0)
    ch.demod(x)
    assert len(ch.frames) == 1
    f = ch.frames[0]
    cut = (int(f.soh_sample) + int(f.end_sample)) // 2 // 1024 * 1024
    assert int(f.soh_sample) + 100 < cut < int(f.end_sample)
    return x, f, cut


SKEW = 3 * 1024


@pytest.mark.parametrize("case", ["soh-below-cut-above", "wrap-after-set-state", "source-past-wrap"])
def test_channel_moved_mid_block_across_the_wrap(D, O, one_block, case):
    """acg_get_state -> acg_set_state carries the SOH stamp as a distance and re-bases it on the destination's counter, both
    modulo 2^32: the source has the wrap between the SOH and the cut; the destination has it between acg_set_state and the closing
    bit; the source runs past 2^32 and the destination stands at 3072.  The block is the oracle's, its end - SOH distance the
    oracle's, its end_sample the destination's own index."""
    from acarsdec_amd import _capi as K
    x, f, cut = one_block
    n = x.size
    soh, end = int(f.soh_sample), int(f.end_sample)
    if case == "soh-below-cut-above":
        src, dst = (1 << 32) - (soh + 100), 0
        assert src + soh < (1 << 32) < src + cut
    elif case == "wrap-after-set-state":
        src, dst = 0, (1 << 32) - SKEW - (end - cut) // 2
        assert dst + SKEW < (1 << 32) < dst + SKEW + (end - cut)
    else:
        src, dst = (1 << 32) + 777777, 0
    d1 = D.Decoder(1, decim=8, ntaps=8, nstreams=1, max_blocks=12)
    if src:
        d1.set_stream_counters(src, (1 << 32) - 2000)
    d1.demod_msk(x[:cut].reshape(1, -1))
    s = K.ChanState()
    d1._chk(d1.L.acg_get_state(d1.ctx, 0, C.byref(s)))
    txt = (C.c_ubyte * 250)()
    d1._chk(d1.L.acg_get_block_text(d1.ctx, 0, txt))
    assert s.Acarsstate in (3, 4, 5) and s.soh_back == cut - soh and 0 < s.blk_len < int(f.len)
    assert d1.drain_frames() == []
    d2 = D.Decoder(2, decim=8, ntaps=8, nstreams=2, max_blocks=12)
    if dst:
        d2.set_stream_counters(dst, 1 << 36)
    d2.demod_msk(np.full((2, SKEW), 0.5, dtype=np.float32))                  # the destination has consumed 3072 samples of its own
    d2._chk(d2.L.acg_set_state(d2.ctx, 1, C.byref(s)))
    d2._chk(d2.L.acg_set_block_text(d2.ctx, 1, txt))
    back = K.ChanState()
    d2._chk(d2.L.acg_get_state(d2.ctx, 1, C.byref(back)))
    assert back.soh_back == s.soh_back                                      # re-based on this slot's counter, the distance kept
    rest = np.full((2, n - cut), 0.5, dtype=np.float32)
    rest[1] = x[cut:]
    d2.demod_msk(rest)
    got = [g for g in d2.drain_frames() if int(g.chn) == 1]
    assert len(got) == 1 and D.frame_tuple(got[0])[1:] == O.frame_tuple(f)[1:]
    assert np.float32(got[0].lvl).tobytes() == np.float32(f.lvl).tobytes()
    assert int(got[0].end_sample) - int(got[0].soh_sample) == end - soh
    assert int(got[0].end_sample) == dst + SKEW + (end - cut)
    d1.close()
    d2.close()


# ---- c. the sinks under a shift, against the committed fixtures --------------------------------------------------------------
def shifted_t0(t0, base):
    assert base % 12500 == 0
    sec = t0[0] - base // 12500
    assert 10 ** 9 <= sec < 10 ** 10                                         # the shifted seconds keep ten digits
    return (sec, t0[1])


fix = TJ.fix                                                                 # (the JSON fixture, as tests/test_gpu_json_sink.py loads it)


def json_run(D, fix, variant, base, bit_base, what):
    """the JSON fixture through a context whose counters start at (base, bit_base) and whose sinks are handed t0 - base / 12500 s.
    what = "json": (per call the drained bytes, the final flight snapshot, the routes); "msgs": per call drain_msgs(oooi=True)"""
    x, g, app = fix
    dec = TJ.new_decoder(D, json_on=False)
    if base or bit_base:
        dec.set_stream_counters(base, bit_base)
    dec.set_msg_filter(**TJ.filter_kw(g, variant))
    if what == "msgs":
        out = TJ.play(dec, x, lambda: dec.drain_msgs(oooi=True))
    else:
        dec.enable_json(shifted_t0(TJ.T0, base), g["station"], app[0], app[1])
        dec.enable_flights(t0=shifted_t0(TJ.T0, base), mdly=600, max_flights=64)
        out = (TJ.play(dec, x, dec.drain_json), dec.flights(), dec.drain_routes())
    dec.close()
    return out


@pytest.fixture(scope="module")
def json_from_zero(D, fix):
    return {(v, what): json_run(D, fix, v, 0, 0, what) for v in TJ.VARIANTS for what in ("json", "msgs")}


def unshift_msg(K, m, base, bit_base):
    m = K.Msg.from_buffer_copy(m)
    m.end_sample -= base
    m.soh_sample -= base
    m.end_bit -= bit_base
    return bytes(m)


def unshift_flight(K, f, base):
    f = K.Flight.from_buffer_copy(f)
    f.ts_sample -= base
    f.tl_sample -= base
    return bytes(f)


def unshift_route(K, r, base):
    r = K.Route.from_buffer_copy(r)
    r.soh_sample -= base
    return bytes(r)


@pytest.mark.parametrize("bi", range(len(U.SINK_BASES)), ids=[str(b) for b in U.SINK_BASES])
def test_json_fixture_is_the_same_bytes_under_a_shift(D, fix, json_from_zero, bi):
    """Every filter variant of the JSON fixture with the counters preset to B (a multiple of 12500) and t0 moved back by
    B / 12500 s: every tv is unchanged, so the text is byte for byte that of a run from 0, call by call -- and so the reference
    program's lines (time stamps cut out of those: it stamps its wall clock).  The records behind it are equal field for field
    except end_sample, soh_sample (+B) and end_bit (+ the bit base), in the same order within every call; the flight table the
    same entry point feeds has ts_sample / tl_sample and its routes soh_sample shifted by B, every other byte equal."""
    from acarsdec_amd import _capi as K
    x, g, app = fix
    base, bit_base = U.SINK_BASES[bi], U.SINK_BIT_BASES[bi % 2]
    for v in TJ.VARIANTS:
        blobs, flights, routes = json_run(D, fix, v, base, bit_base, "json")
        blobs0, flights0, routes0 = json_from_zero[(v, "json")]
        assert blobs == blobs0, (v, next(i for i, (a, b) in enumerate(zip(blobs, blobs0)) if a != b))
        lines = TJ.split_lines(b"".join(blobs))
        ref = [ln.encode("ascii") + b"\n" for ln in g["variants"][v]["lines"]]
        assert len(lines) == len(ref) > 0, v
        for c in range(g["nch"]):
            assert [JM.cut_timestamp(ln)[0] for ln in lines if TJ.chn_of(ln) == c] == [JM.cut_timestamp(ln)[0] for ln in ref if TJ.chn_of(ln) == c], (v, c)
        assert len(flights0) > 0 and [unshift_flight(K, f, base) for f in flights] == [bytes(f) for f in flights0], v
        assert [unshift_route(K, r, base) for r in routes] == [bytes(r) for r in routes0], v
        assert all(f.ts_sample >= base and f.tl_sample >= base for f in flights) and all(r.soh_sample >= base for r in routes)
        msgs, msgs0 = json_run(D, fix, v, base, bit_base, "msgs"), json_from_zero[(v, "msgs")]
        assert len(msgs) == len(msgs0)
        for k, (part, part0) in enumerate(zip(msgs, msgs0)):
            assert [unshift_msg(K, m, base, bit_base) + bytes(o) for m, o in part] == [bytes(m) + bytes(o) for m, o in part0], (v, k)
            assert all(m.end_sample >= m.soh_sample >= base and m.end_bit >= bit_base for m, _ in part)
        if v == "none":
            # the time stamps are the model's print of t0 + soh_sample / 12500 s on the shifted values
            t0 = shifted_t0(TJ.T0, base)
            for c in range(g["nch"]):
                assert [JM.cut_timestamp(ln)[1] for ln in lines if TJ.chn_of(ln) == c] == \
                    [JM.print_number(JM.tv_double(*JM.tv(t0, m.soh_sample))).encode() for part in msgs for m, _ in part if m.chn == c], c
            ends = [m.end_sample for part in msgs for m, _ in part]
            for p in (1 << 31, 1 << 32):
                if base < p < base + x.shape[1]:                             # the counters started below the power of two and passed it
                    assert max(ends) >= p, (base, p)


def flights_fixture():
    pcm = np.load(os.path.join(GOLDEN, "flights_pcm16.npz"))["pcm"]
    with open(os.path.join(GOLDEN, "flights_golden.json")) as f:
        g = json.load(f)
    nch, chunk = 3, 4096
    assert pcm.shape[0] == nch
    x = pcm.astype(np.float32) / 32768.0
    return np.concatenate([x, np.zeros((nch, (-x.shape[1]) % chunk), dtype=np.float32)], axis=1), g


def flights_run(D, x, g, variant, base, bit_base):
    """test_fixture_end_to_end_equals_the_reference_monitor_and_routes' run with the counters preset: per delivered message the
    snapshot, then the routes"""
    nch, chunk = 3, 4096
    dec = D.Decoder(nch, decim=8, ntaps=8, max_blocks=chunk // 1024, repair=True, bitlog=False)
    if base or bit_base:
        dec.set_stream_counters(base, bit_base)
    dec.set_msg_filter(**TF.filter_kw(g["variants"][variant]["args"], g["label_list"]))
    dec.enable_flights(t0=shifted_t0(TF.T0, base), mdly=600, max_flights=64)
    snaps = []
    for s in range(0, x.shape[1], chunk):
        dec.demod_msk(x[:, s:s + chunk])
        msgs = dec.drain_msgs()
        assert len(msgs) <= 1, (variant, s)
        if msgs:
            snaps.append(dec.flights())
    routes = dec.drain_routes()
    dec.close()
    return snaps, routes


@pytest.fixture(scope="module")
def flights_from_zero(D):
    x, g = flights_fixture()
    return x, g, {v: flights_run(D, x, g, v, 0, 0) for v in g["variants"]}


@pytest.mark.parametrize("bi", range(len(U.SINK_BASES)), ids=[str(b) for b in U.SINK_BASES])
def test_flight_fixture_is_the_same_table_under_a_shift(D, flights_from_zero, bi):
    """The flight fixture likewise: the monitor rows after every delivered message and the route JSON equal the reference
    program's; acg_flight.ts_sample / tl_sample and acg_route.soh_sample are those of a run from 0 plus B, every other byte (the
    wall-clock fields among them) equal."""
    from acarsdec_amd import _capi as K
    x, g, zero = flights_from_zero
    base, bit_base = U.SINK_BASES[bi], U.SINK_BIT_BASES[(bi + 1) % 2]
    for v, gv in g["variants"].items():
        snaps, routes = flights_run(D, x, g, v, base, bit_base)
        snaps0, routes0 = zero[v]
        frames = gv["frames"]
        assert len(snaps) == len(snaps0) == len(frames) > 0, v
        for k, (fl, fl0) in enumerate(zip(snaps, snaps0)):
            assert [TF.parse_row(r, 3) for r in D.monitor_rows(fl, 3)] == [g["rows"][i] for i in frames[k]], (v, k)
            assert [unshift_flight(K, f, base) for f in fl] == [bytes(f) for f in fl0], (v, k)
            assert all(f.ts_sample >= base for f in fl)
        assert [D.route_json(r) for r in routes] == [D.route_json(r) for r in routes0], v
        assert [dict(flight=r["flight"], depa=r["depa"], dsta=r["dsta"]) for r in map(D.route_json, routes)] == gv["routes"], v
        assert [unshift_route(K, r, base) for r in routes] == [bytes(r) for r in routes0], v
        for p in (1 << 31, 1 << 32):
            if base < p < base + x.shape[1]:                                 # the counters started below the power of two and passed it
                assert max(f.tl_sample for fl in snaps for f in fl) >= p, (v, base, p)


# ---- d. the selftest entry points at large counters --------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [(1 << 32) - 10 ** 6, 1 << 42], ids=["across-2^32", "2^42"])
def test_selftest_flights_equals_the_list_walk_at_large_sample_indices(D, offset):
    """20 000 random records whose end_sample / soh_sample are offset so that they cross 2^32 (and lie past 2^42), t0 moved back
    to match, in shuffled batches of up to 3000: the time sort's key (end_sample << 20 | chn) has upper digits that are not zero
    and differ inside a batch.  The snapshot after every batch and the routes equal the list walk's (Python integers)."""
    from acarsdec_amd import _capi as K
    rng = np.random.default_rng(4100)
    n = 20000
    recs = TF.random_records(K, rng, n, 500, 1024)
    for i in range(n):
        recs[i].end_sample += offset
        recs[i].soh_sample += offset
        recs[i].end_bit = recs[i].end_sample // 5
    us = TF.T0[0] * 10 ** 6 + TF.T0[1] - offset * 80
    t0 = (us // 10 ** 6, us % 10 ** 6)
    assert t0[0] > 10 ** 9
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(int(rng.integers(1, 3001)), n - sum(sizes)))
    shuffled = (K.Msg * n)()
    at, crossing = 0, 0
    for s in sizes:
        ends = [recs[i].end_sample for i in range(at, at + s)]
        crossing += min(ends) < (1 << 32) <= max(ends)              # the key's digit at bits 48-55 differs inside this batch
        for j, i in enumerate(rng.permutation(s)):
            C.memmove(C.addressof(shuffled) + (at + j) * C.sizeof(K.Msg), C.addressof(recs) + (at + int(i)) * C.sizeof(K.Msg), C.sizeof(K.Msg))
        at += s
    if offset < (1 << 32):
        assert crossing == 1
    else:
        assert all(recs[i].end_sample >> 42 == 1 for i in range(n))  # the key's top digit is not zero
    kw = dict(downlink_only=True, skip_empty=True, labels=TF.LABELS_B)
    f = D.make_msg_filter(**kw)
    cfg = K.FlightConfig(t0[0], t0[1], 2, 8192)
    snap_cap, route_cap = 200000, n
    snaps, routes = (K.Flight * snap_cap)(), (K.Route * route_cap)()
    snap_n, nroutes, dropped = (C.c_int * len(sizes))(), C.c_int(0), C.c_int(0)
    rc = K.load().acg_selftest_flights(shuffled, (C.c_int * len(sizes))(*sizes), len(sizes), C.byref(cfg), C.byref(f), snaps, snap_cap, snap_n,
                                       routes, route_cap, C.byref(nroutes), C.byref(dropped))
    assert rc == K.OK and dropped.value == 0, rc
    walk = FM.ListWalk(2)
    at = sat = nev = 0
    for b, s in enumerate(sizes):
        evs = [e for e in (FM.event_of(recs[i], t0, **TF.model_kw(kw)) for i in range(at, at + s)) if e is not None]
        at += s
        nev += len(evs)
        for e in FM.batch_order(evs):
            walk.add(e)
        want = [FM.flight_bytes(e) for e in walk.entries()]
        assert snap_n[b] == len(want), (b, snap_n[b], len(want))
        got = [bytes(snaps[sat + i]) for i in range(snap_n[b])]
        assert got == want, (b, next(i for i in range(len(want)) if got[i] != want[i]))
        sat += snap_n[b]
    assert nev >= 10000 and len(walk.routes) > 100 and walk.recreated > 100
    assert [bytes(routes[i]) for i in range(nroutes.value)] == [FM.route_bytes(r) for r in walk.routes]


def test_selftest_msg_json_equals_the_model_at_large_counters(D):
    """Records whose end_bit is spread up to 2^44 - 1 (the order key's whole field) and whose soh_sample reaches 2^42: the order
    and the text equal the model's, whole buffer byte for byte."""
    from acarsdec_amd import _capi as K
    L = K.load()
    rng = np.random.default_rng(4400)
    n, nch = 3000, 7
    fr = [131725000, 131525000, 0, 129125000, 136975000, 1090000000, 131825000]
    recs = TJ.random_records(rng, n, K, nch)
    M = K.Msg
    i64 = lambda v: np.frombuffer(np.int64(v).tobytes(), dtype=np.uint8)
    edges = [(1 << 44) - 1, (1 << 44) - 2, 1 << 43, (1 << 32) - 1, 1 << 32, (1 << 31) - 1, 1 << 31, 0, 1]
    end_bits = []
    for i in range(n):
        r = recs[i]
        if i < 4 * len(edges):                                     # the edges of the key's field and of 32 bits, on several channels
            eb = edges[i % len(edges)]
        elif i % 11 == 0:
            eb = end_bits[i - 1]                                   # equal keys now and then: the sort is stable
        else:
            eb = int(rng.integers(0, 1 << int(rng.integers(20, 45))))          # every magnitude up to 2^44
        end_bits.append(eb)
        soh = int(rng.integers(0, (1 << 42) + 1)) if i % 4 else (1 << 42) - int(rng.integers(0, 2))
        r[M.end_bit.offset:M.end_bit.offset + 8] = i64(eb)
        r[M.soh_sample.offset:M.soh_sample.offset + 8] = i64(soh)
        r[M.end_sample.offset:M.end_sample.offset + 8] = i64(soh + int(rng.integers(0, 3000)))
    assert max(end_bits) == (1 << 44) - 1 and sum(e >= 1 << 32 for e in end_bits) > n // 4
    buf = (K.Msg * n).from_buffer_copy(recs.tobytes())
    fr_arr = np.array(fr, dtype=np.int32)
    cfg = D.json_config((10 ** 9, 999999), b"STN1", b"acarsdec", b"3.7")       # t0 + 2^42 / 12500 s keeps ten digits
    for kw in (dict(), dict(downlink_only=True, skip_empty=True, labels="Q1:44:QA:QT:8D:12:33")):
        f = D.make_msg_filter(**kw) if kw else None
        mkw = dict(downlink_only=kw.get("downlink_only", False), skip_empty=kw.get("skip_empty", False), labels=LM.parse_label_filter(kw.get("labels")))
        lines = TJ.model_buffer(K, recs, nch, cfg, fr, mkw)
        want = b"".join(lines)
        cap = len(want) + 4096
        out = np.full(cap, 0xA5, dtype=np.uint8)
        nb, nl = C.c_size_t(0), C.c_int(0)
        rc = L.acg_selftest_msg_json(buf, n, C.byref(f) if f is not None else None, C.byref(cfg), fr_arr.ctypes.data, nch, out.ctypes.data, cap,
                                     C.byref(nb), C.byref(nl))
        assert rc == K.OK, (kw, rc)
        got = out[:nb.value].tobytes()
        if got != want:                                            # name the first line that differs
            gl = TJ.split_lines_loose(got)
            k = next((i for i, (a, b) in enumerate(zip(gl + [None], lines + [None])) if a != b), None)
            assert False, (kw, k, gl[k] if k is not None and k < len(gl) else None, lines[k] if k is not None and k < len(lines) else None)
        assert nl.value == len(lines) > (10 if kw else n // 2) and (out[nb.value:] == 0xA5).all()
    # one past the key's field is refused, not wrapped
    bad = (K.Msg * 1).from_buffer_copy(recs[:1].tobytes())
    bad[0].end_bit = 1 << 44
    assert L.acg_selftest_msg_json(bad, 1, None, C.byref(cfg), fr_arr.ctypes.data, nch, out.ctypes.data, cap, C.byref(nb), C.byref(nl)) == K.EINVAL
