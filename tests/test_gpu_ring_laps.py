"""The block ring when the host falls behind (acarsdec_amd/csrc/results.cpp: ring_upto, ring_claim, ring_result), through every
entry point that consumes blocks: laps, loss counts, what survives and what each call returns, held to tests/ring_model.py (the
contract of include/acarsdec_amd.h for ACG_EOVERFLOW and acg_collect_*) and to the oracle's blocks of the same samples.

Schedules (computed from the oracle's blocks per call and the ring's size; each test asserts that its schedule has the shape it
is meant to have):
  A  no collect, then a drain through a buffer of 5 records: one ACG_EOVERFLOW, ACG_EAGAIN until a last ACG_OK;
  B  no collect until the newest call has lapped the consumer while the mark one call back has not; collect(lag = 1); one more
     call; collect(lag = 1); drain -- the lap a collect used not to see;
  C  collect(lag = 1) through a buffer of 3 records after every call: the remainder goes stale until the newest call laps it;
  D  B with lag = 2;
  E  a host that collects after every call, with every lag: never a loss, the oracle's output complete;
  F  A and B with the 2^32 wrap of the counters inside the lost run, inside the survivors and exactly at upto - cap;
  G  B and C without the acg_sync in front of the collect.
A runs on a ring of 32 records (2 channels) and of 256 (8 channels); B, D, F on B and G run on 8 channels of dense traffic, where
the call that laps the host overwrites six blocks spread over the channels (G also where it overwrites exactly one).
Everything is exact.  Nothing here provokes a fault: a lapped ring is defined behaviour with its own return code.

What these tests found when they were written: the library judged a lap against a collect's own mark.  On B, D and G the first
collect said ACG_OK where the model loses 1 block (the ring of 32 records) or 6 (the ring of 256); on the ring of 32 it handed out
32 records of which one was a block of the newest call sitting in the slot of the block it had
overwritten, lost_blocks stayed 0, and the next call handed that block out again; without the sync that record could be caught
half repaired.  On C two collects said ACG_EAGAIN over overwritten slots, 74 of 540 records were not of the calls claimed, 2 to 6
came twice and the loss was under-counted (94 of 99).  A, E and F on schedule A passed.  tests/test_ring_model.py shows the same
on a brute-force ring without a GPU."""
import collections
import ctypes as C
import functools
import re
from types import SimpleNamespace

import numpy as np
import pytest

import flight_model as FM
import flight_table_model as FTM
import json_model as JM
import label_model as LM
import ring_model as RM
import stats_model as SM
import text_model as TM
from test_gpu_round5 import traffic

pytestmark = pytest.mark.gpu

T0 = (1792301725, 269667)
STATION, APP = "STN1", ("acarsdec", "3.7")
BIG = 1 << 20
CONFIGS = {"small": dict(nch=2, max_blocks=1, max_lag=1, ncalls=256, seed=4711),        # a ring of 32 records
           "lag2": dict(nch=2, max_blocks=1, max_lag=2, ncalls=256, seed=4711),         # the same traffic, lag 2 allowed
           "wide": dict(nch=8, max_blocks=2, max_lag=2, ncalls=256, seed=1147),         # a ring of 256 records
           # ... and traffic dense enough to outrun a collect of 3 records after every call (schedule C)
           "dense": dict(nch=8, max_blocks=2, max_lag=1, ncalls=96, seed=2718, gap=(300, 600), text_len=(8, 30)),
           # ... and, lag 2 allowed, a seed at which the call that laps a silent host overwrites SEVERAL blocks (schedules B, D, F, G:
           # with the sparse traffic above that call queues one block past the ring and the lap loses exactly one)
           "burst": dict(nch=8, max_blocks=2, max_lag=2, ncalls=56, seed=3004, gap=(300, 600), text_len=(8, 30))}
PATHS = ("frames", "frames_repair", "msgs", "msgs_oooi", "json", "text", "outputs")


@pytest.fixture(scope="module")
def D():
    from acarsdec_amd import decoder
    from acarsdec_amd import _capi as K
    assert K.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return decoder


# ---- the reference: the oracle's blocks of the same samples, call by call ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def world(name):
    """the traffic of a configuration and the oracle's view of it: x, the blocks per call (adds), and per key (chn, end_bit) the
    call that queued the block, its place in its channel's sequence and the record every entry point must hand out for it"""
    from acarsdec_amd import synth as S
    from oracle import oracle as O
    cfg = CONFIGS[name]
    nch, clen, ncalls = cfg["nch"], cfg["max_blocks"] * 1024, cfg["ncalls"]
    x = traffic(S, nch, ncalls * clen, cfg["seed"], corrupt=[None, None, "p1", None, "db", None, "crc", None],
                gap=cfg.get("gap", (1200, 2500)), text_len=cfg.get("text_len", (8, 60)))
    adds = [0] * ncalls
    blocks = {}                                                   # key -> SimpleNamespace(call, idx, raw, kept, msg)
    per_chn = []
    for c in range(nch):
        ch = O.Channel(c, max_frames=4096)
        upto = []
        for k in range(ncalls):
            ch.demod(x[c, k * clen:(k + 1) * clen])
            upto.append(int(ch.c.frames_n))
        assert upto[-1] < 4096
        keys, k = [], 0
        for i, f in enumerate(ch.frames):
            while upto[k] <= i:
                k += 1
            adds[k] += 1
            o = O.blk_process(f)
            m = None
            if o is not None:
                s = O.msg_split(o)
                m = SimpleNamespace(**{n: getattr(s, n) for n, _ in O.OrcMsg._fields_})
                m.txt = bytes(s.txt)
                m.chn, m.end_bit, m.end_sample, m.soh_sample = c, int(o.end_bit), int(o.end_sample), int(o.soh_sample)
            key = (c, int(f.end_bit))
            assert key not in blocks
            blocks[key] = SimpleNamespace(call=k, idx=i, raw=frame_rec(O, f), kept=frame_rec(O, o) if o is not None else None, msg=m)
            keys.append(key)
        per_chn.append(keys)
    return SimpleNamespace(cfg=cfg, nch=nch, clen=clen, ncalls=ncalls, x=x, adds=adds, blocks=blocks, per_chn=per_chn)


def lvl_bytes(v):
    return np.float32(v).tobytes()


def frame_rec(O, f):
    return O.frame_tuple(f) + (int(f.end_bit), int(f.end_sample), int(f.soh_sample), lvl_bytes(f.lvl))


def msg_rec(O, m):
    return O.msg_tuple(m) + (int(m.txt_len), int(m.end_bit), int(m.end_sample), int(m.soh_sample), lvl_bytes(m.lvl))


def oooi_rec(m):
    return LM.oooi_bytes(*LM.decode((bytes(m.label) + b"\0\0")[:2], bytes(m.txt), max(0, min(int(m.txt_len), 242))))


def ts_token(m):
    return JM.print_number(JM.tv_double(*JM.tv(T0, m.soh_sample))).encode()


def json_rec(m):
    return JM.line(m, m.chn, ts_token(m), station=STATION.encode(), app=tuple(a.encode() for a in APP))


# ---- the entry points: one C call each, whatever it returns ---------------------------------------------------------------------------
class Path:
    """how one entry point is set up, called once (collect with a lag, or drain) and compared with the reference"""

    def __init__(self, name, D, w):
        from acarsdec_amd import _capi as K
        from oracle import oracle as O
        self.name, self.K, self.O, self.w = name, K, O, w
        self.repair = name != "frames"
        cfg = w.cfg
        self.dec = dec = D.Decoder(w.nch, decim=8, ntaps=8, max_blocks=cfg["max_blocks"], repair=self.repair, bitlog=False, max_lag=cfg["max_lag"])
        self.cap = int(dec.L.acg_lab_block_ring_size(dec.ctx))
        self.max_lag = int(dec.L.acg_max_lag(dec.ctx))
        if self.repair:
            dec.enable_stats()
        if name == "msgs_oooi":
            dec.enable_flights(t0=T0, mdly=600, max_flights=1024)
        elif name == "json":
            dec.enable_json(T0, STATION, *APP)
        elif name == "text":
            dec.enable_text("std", T0, date=True, station_id=STATION)
        elif name == "outputs":
            dec.enable_outputs(["msgs", "json", "oneline", "std"], T0, STATION, *APP)
        self.blocks_seen = self.lost_seen = 0                     # the statistics table's totals after the last C call

    def expected(self, key):
        """the record this entry point hands out for the block, or None: the repair drops it"""
        b = self.w.blocks[key]
        if self.name == "frames":
            return b.raw
        if self.name == "frames_repair":
            return b.kept
        m = b.msg
        if m is None:
            return None
        if self.name == "msgs":
            return msg_rec(self.O, m)
        if self.name == "msgs_oooi":
            return msg_rec(self.O, m) + (oooi_rec(m),)
        if self.name == "json":
            return json_rec(m)
        if self.name == "text":
            return TM.record(m, m.chn, TM.STD, TM.F_DATE, t0=T0, station=STATION.encode())
        return (msg_rec(self.O, m) + (oooi_rec(m),), json_rec(m), TM.record(m, m.chn, TM.ONELINE, 0, t0=T0), TM.record(m, m.chn, TM.STD, 0, t0=T0))

    def call(self, lag, max_recs):
        """one C call (lag None: the drain): (rc, [(key, record)], the messages handed out or None)"""
        K, dec, L = self.K, self.dec, self.dec.L
        n = min(int(max_recs), 2 * self.cap + 8)                  # (room for everything the ring can hold is "as large as you like")
        lead = () if lag is None else (int(lag),)
        cnt = C.c_int(0)
        fn = lambda stem: getattr(L, ("acg_drain_" if lag is None else "acg_collect_") + stem)
        key_of = lambda r: (int(r.chn), int(r.end_bit))
        if self.name in ("frames", "frames_repair"):
            buf = (K.Frame * n)()
            rc = self.note(fn("frames")(dec.ctx, *lead, buf, n, C.byref(cnt)))
            return rc, [(key_of(buf[i]), frame_rec(self.O, buf[i])) for i in range(cnt.value)], None
        if self.name == "msgs":
            buf = (K.Msg * n)()
            rc = self.note(fn("msgs")(dec.ctx, *lead, buf, n, C.byref(cnt)))
            return rc, [(key_of(buf[i]), msg_rec(self.O, buf[i])) for i in range(cnt.value)], None
        if self.name == "msgs_oooi":
            buf, ob = (K.Msg * n)(), (K.Oooi * n)()
            rc = self.note(fn("msgs_oooi")(dec.ctx, *lead, buf, ob, n, C.byref(cnt)))
            msgs = [K.Msg.from_buffer_copy(buf[i]) for i in range(cnt.value)]
            return rc, [(key_of(m), msg_rec(self.O, m) + (bytes(ob[i]),)) for i, m in enumerate(msgs)], msgs
        if self.name == "outputs":
            # the four legs' buffers (acg_out_buf): records and labels for MSGS, bytes and an offset table for each of the others
            mb, ob = (K.Msg * n)(), (K.Oooi * n)()
            recmax = (None, K.JSON_LINE_MAX, K.TEXT_REC_MAX, K.TEXT_REC_MAX)
            outs = [None] + [C.create_string_buffer(n * r) for r in recmax[1:]]
            offs = [None] + [(C.c_uint * (n + 1))() for _ in recmax[1:]]
            bufs = (K.OutBuf * 4)()
            bufs[0].out, bufs[0].cap, bufs[0].oooi = C.addressof(mb), n * C.sizeof(K.Msg), C.addressof(ob)
            for l in (1, 2, 3):
                bufs[l].out, bufs[l].cap, bufs[l].offs = C.addressof(outs[l]), n * recmax[l], C.addressof(offs[l])
            rc = self.note(fn("outputs")(dec.ctx, *lead, bufs, n, C.byref(cnt)))
            nr = cnt.value
            assert bufs[0].nbytes == nr * C.sizeof(K.Msg)
            legs = []
            for l in (1, 2, 3):
                blob = outs[l].raw[:bufs[l].nbytes]
                assert offs[l][0] == 0 and offs[l][nr] == bufs[l].nbytes
                legs.append([blob[offs[l][i]:offs[l][i + 1]] for i in range(nr)])
            keys = self.sink_keys(K.SINK_OUTPUTS, nr)
            assert [key_of(mb[i]) for i in range(nr)] == keys
            recs = [(msg_rec(self.O, mb[i]) + (bytes(ob[i]),), legs[0][i], legs[1][i], legs[2][i]) for i in range(nr)]
            return rc, list(zip(keys, recs)), None
        nb = C.c_size_t(0)
        if self.name == "json":
            buf = C.create_string_buffer(n * K.JSON_LINE_MAX)
            rc = self.note(fn("json")(dec.ctx, *lead, buf, n * K.JSON_LINE_MAX, C.byref(nb), C.byref(cnt)))
            lines = [ln + b"\n" for ln in buf.raw[:nb.value].split(b"\n")[:-1]]
            assert len(lines) == cnt.value
            return rc, list(zip(self.sink_keys(K.SINK_JSON, cnt.value), lines)), None
        assert self.name == "text"
        buf, offs = C.create_string_buffer(n * K.TEXT_REC_MAX), (C.c_uint * (n + 1))()
        rc = self.note(fn("text")(dec.ctx, *lead, buf, n * K.TEXT_REC_MAX, C.byref(nb), offs, n, C.byref(cnt)))
        blob = buf.raw[:nb.value]
        return rc, list(zip(self.sink_keys(K.SINK_TEXT, cnt.value), [blob[offs[i]:offs[i + 1]] for i in range(cnt.value)])), None

    def sink_keys(self, sink, nrecs):
        """acg_sink_keys: (chn, end_bit) of the records the sink's last C call handed out"""
        buf = np.zeros(max(1, nrecs), dtype=np.uint64)
        n = C.c_int(0)
        assert self.dec.L.acg_sink_keys(self.dec.ctx, sink, buf.ctypes.data, len(buf), C.byref(n)) == self.K.OK and n.value == nrecs
        keys = [int(k) for k in buf[:nrecs]]
        return [(k >> self.K.SINK_KEY_END_BITS, k & ((1 << self.K.SINK_KEY_END_BITS) - 1)) for k in keys]

    def consumed_by_last_call(self, nrecs):
        """blocks the last C call consumed: n on the raw path, the delta of the statistics table's `blocks` elsewhere; and the
        delta of lost_blocks (None on the raw path: the table needs the repair)"""
        if not self.repair:
            return nrecs, None
        st, lost = self.dec.stats()
        total = int(st["blocks"].sum())
        d, self.blocks_seen = total - self.blocks_seen, total
        dl, self.lost_seen = lost - self.lost_seen, lost
        return d, dl

    def note(self, rc):
        """the C call's return code, and (before a later call can replace the error text) the loss acg_last_error names"""
        self.said = 0                                             # (None: ACG_EOVERFLOW without a figure)
        if rc == self.K.EOVERFLOW:
            m = re.search(rb"the (\d+) oldest blocks are lost", self.dec.L.acg_last_error(self.dec.ctx))
            self.said = int(m.group(1)) if m else None
        return rc


# ---- a schedule on the device beside the model -------------------------------------------------------------------------------------
def run(p, steps, start=0):
    """Plays the steps on the decoder and on the model and asserts, call by call: the return code, the blocks consumed and the
    loss (acg_last_error's figure, lost_blocks) are the model's; ACG_EOVERFLOW iff blocks were lost; every record is the
    reference's record of its key; no key comes twice; per channel end_bit rises; the blocks a call hands out belong to the
    calls whose part of the queue it claimed, all of those of a call it claimed whole, and on the raw path exactly as many of
    each call as it claimed.  At the end: consumed + lost = produced, the statistics rows' identities, the blocks missing from
    a channel form at most one run per lap, and everything issued after the last lap is there.  Returns the log."""
    w, dec, K = p.w, p.dec, p.K
    ring = RM.Ring(p.cap, start)
    if start:
        assert dec.L.acg_lab_set_block_counter(dec.ctx, C.c_uint(start)) == K.OK
    cum = [0]                                                     # blocks queued before call k, counted from the start
    seen, last_end, log, msgs_out, issued = {}, {}, [], [], 0
    consumed_total = lost_total = 0
    after_last_lap = 0

    def one(lag, max_recs, step):
        nonlocal consumed_total, lost_total, after_last_lap
        want_rc, want_lost, first, take = ring.collect(lag, max_recs) if lag is not None else ring.drain(max_recs)
        rc, recs, msgs = p.call(lag, max_recs)
        ctx = (p.name, step, "issued %d" % issued, "model", (want_rc, want_lost, (first - start) & RM.MASK, take), "device", rc, len(recs))
        assert rc in (K.OK, K.EAGAIN, K.EOVERFLOW), ctx + (dec.L.acg_last_error(dec.ctx),)
        said = p.said
        nblocks, dlost = p.consumed_by_last_call(len(recs))
        ctx += ("consumed", nblocks, "lost", said, dlost)
        assert (rc == K.EOVERFLOW) == (said is not None and said > 0), ctx
        assert rc == want_rc and said == want_lost and nblocks == take, ctx
        assert dlost is None or dlost == want_lost, ctx
        lo = (first - start) & RM.MASK
        hi = lo + take
        per_call = collections.Counter()
        for key, rec in recs:
            assert key in w.blocks, ctx + ("a record with no block of the reference behind it", key)
            assert key not in seen, ctx + ("handed out twice", key, "first by call", seen[key])
            seen[key] = len(log)
            assert rec == p.expected(key), ctx + (key, rec, p.expected(key))
            assert key[1] > last_end.get(key[0], -1), ctx + ("end_bit does not rise", key)
            last_end[key[0]] = key[1]
            k = w.blocks[key].call
            assert k < issued and cum[k] < hi and cum[k + 1] > lo, ctx + ("a block of call %d, outside the claim" % k, key)
            per_call[k] += 1
        assert [k for k, _ in recs] == sorted(k for k, _ in recs), ctx       # (chn, end_bit) order within the call
        for k in range(issued):
            overlap = max(0, min(hi, cum[k + 1]) - max(lo, cum[k]))
            assert per_call[k] <= overlap, ctx + ("call", k)
            if p.name == "frames":
                assert per_call[k] == overlap, ctx + ("call", k)
            if overlap and lo <= cum[k] and cum[k + 1] <= hi:                  # the call's blocks claimed whole
                want = {key for key, b in w.blocks.items() if b.call == k and p.expected(key) is not None}
                assert want == {key for key, _ in recs if w.blocks[key].call == k}, ctx + ("call", k)
        consumed_total += take
        lost_total += want_lost
        if want_lost:
            after_last_lap = issued
        if msgs is not None:
            msgs_out.append(msgs)
        log.append(SimpleNamespace(step=step, rc=rc, lost=want_lost, first=lo, take=take, nrecs=len(recs), issued=issued))
        return rc

    for st in steps:
        if st[0] == "process":
            assert st[1] == issued
            dec.demod_msk(w.x[:, issued * w.clen:(issued + 1) * w.clen])
            ring.process(w.adds[issued])
            cum.append(cum[-1] + w.adds[issued])
            issued += 1
        elif st[0] == "sync":
            dec.sync()
        elif st[0] == "collect":
            one(st[1], st[2], st)
        else:
            assert st[0] == "drain_all"
            for _ in range(4 * p.cap):
                if one(None, st[1], st) == K.OK:
                    break
            else:
                raise AssertionError("the drain never said ACG_OK")
    # the end: everything is accounted for
    assert consumed_total + lost_total == cum[-1] and RM.sdiff(ring.live(), ring.consumed) == 0
    if p.repair:
        st, lost = dec.stats()
        assert lost == lost_total and int(st["blocks"].sum()) == consumed_total
        for c in range(w.nch):
            SM.check_identities({k: int(st[k][c]) for k in SM.COUNTERS}, msgs_only=not p.name.startswith("frames"))
    laps = sum(1 for e in log if e.lost)
    missing_total = 0
    for c in range(w.nch):
        vis = [key for key in w.per_chn[c] if w.blocks[key].call < issued and p.expected(key) is not None]
        gone = [key not in seen for key in vis]
        runs = sum(1 for i, g in enumerate(gone) if g and (i == 0 or not gone[i - 1]))
        assert runs <= laps, (p.name, "channel", c, "missing blocks in", runs, "runs after", laps, "laps")
        missing_total += sum(gone)
        late = [key for key in vis if w.blocks[key].call >= after_last_lap and key not in seen]
        assert not late, (p.name, "blocks of calls issued after the last lap are missing", late[:3])
    assert missing_total <= lost_total and (p.name != "frames" or missing_total == lost_total)
    if p.name == "msgs_oooi":                                     # the flight table saw exactly the messages handed out
        batches = [[e for e in (FM.event_of(m, T0) for m in ms) if e is not None] for ms in msgs_out]
        snaps, routes, drops = FTM.expect_without(dict(mdly=600), batches, [()] * len(batches))
        assert [bytes(f) for f in dec.flights()] == (snaps[-1] if snaps else []) and dec.flights_dropped == drops == 0
        assert [bytes(r) for r in dec.drain_routes()] == routes
        assert sum(map(len, batches)) >= 10 or issued < 100
    return log


def from_zero_after_reset(p):
    """after acg_reset the context is as new: collected after every call, the reference's output complete"""
    p.dec.reset()
    p.blocks_seen = p.lost_seen = 0
    n = 24
    steps = []
    for k in range(n):
        steps += [("process", k), ("collect", 1, BIG)]
    log = run(p, steps + [("drain_all", BIG)])
    assert all(e.rc == p.K.OK and e.lost == 0 for e in log)
    assert sum(e.nrecs for e in log) == sum(1 for key, b in p.w.blocks.items() if b.call < n and p.expected(key) is not None) >= 5


def rcs(log):
    return [e.rc for e in log]


# ---- A, B on every entry point ------------------------------------------------------------------------------------------------------
def shape_a(p, log):
    K, w = p.K, p.w
    total = sum(w.adds)
    assert total >= 3 * p.cap + p.cap // 2, (total, p.cap)        # the ring is lapped several times over
    assert rcs(log) == [K.EOVERFLOW] + [K.EAGAIN] * (len(log) - 2) + [K.OK] and len(log) >= p.cap // 5
    assert log[0].lost == total - p.cap and log[0].take == 5 and sum(e.take for e in log) == p.cap


def shape_b(p, log, lag=1, min_lost=2):
    K, w = p.K, p.w
    n = RM.first_silent_lap(w.adds, p.cap, lag)
    cnt = np.cumsum(w.adds)
    assert cnt[n - 1 - lag] <= p.cap < cnt[n - 1]                 # the mark `lag` calls back fits the ring, the newest call does not
    first = log[0]
    assert first.issued == n and first.rc == K.EOVERFLOW and first.lost == cnt[n - 1] - p.cap >= min_lost
    assert first.take == cnt[n - 1 - lag] - first.lost > 0        # what survived of the collect's own part is handed out
    assert all(e.rc == K.OK and e.lost == 0 for e in log[1:])     # the loss is reported once


@pytest.mark.parametrize("path", PATHS)
def test_schedule_a_a_ring_lapped_several_times_drained_through_five_records(D, path):
    w = world("small")
    p = Path(path, D, w)
    assert p.cap == 32 and p.max_lag >= 1
    shape_a(p, run(p, RM.schedule_a(w.adds, small=5)))
    from_zero_after_reset(p)
    p.dec.close()


@pytest.mark.parametrize("path", PATHS)
def test_schedule_b_the_newest_call_laps_a_collect_that_stays_behind(D, path):
    """the lapping call overwrites six blocks, spread over the channels: the collect loses those, says so, and hands out the rest
    of what it came for"""
    w = world("burst")
    p = Path(path, D, w)
    assert p.cap == 256 and p.max_lag >= 2
    shape_b(p, run(p, RM.schedule_b(w.adds, p.cap, lag=1)))
    p.dec.close()


def test_schedule_a_on_a_ring_of_256_records(D):
    w = world("wide")
    p = Path("frames", D, w)
    assert p.cap == 256 and p.max_lag >= 2
    shape_a(p, run(p, RM.schedule_a(w.adds, small=5)))
    p.dec.close()


# ---- C, D, E, G on the raw path and one sink -----------------------------------------------------------------------------------------
OTHER = ("frames", "json")


def shape_c(p, log):
    """the collects keep up at first (ACG_OK), then fall behind (ACG_EAGAIN), then the newest call laps the stale remainder"""
    K = p.K
    seq = rcs(log)
    assert K.EOVERFLOW in seq and K.EAGAIN in seq[:seq.index(K.EOVERFLOW)]
    first = log[seq.index(K.EOVERFLOW)]
    assert first.step[0] == "collect" and first.take == 3        # the lap is met by a collect, and it still hands out survivors
    assert seq[-1] == K.OK and sum(e.lost for e in log) > 0


@pytest.mark.parametrize("sync", [True, False], ids=["sync", "nosync"])
@pytest.mark.parametrize("path", OTHER)
def test_schedule_c_a_small_buffer_lets_the_remainder_go_stale(D, path, sync):
    """(nosync: schedule G -- the outcome does not depend on whether the newest call has run yet)"""
    w = world("dense")
    p = Path(path, D, w)
    assert p.cap == 256 and sum(w.adds) - 3 * w.ncalls > p.cap + 64      # the buffer of 3 falls a ring and more behind
    shape_c(p, run(p, RM.schedule_c(w.adds, p.cap, small=3, lag=1, sync=sync)))
    p.dec.close()


@pytest.mark.parametrize("name", ["burst", "small"])
@pytest.mark.parametrize("path", OTHER)
def test_schedule_g_b_without_the_sync(D, path, name):
    """(small: the ring of 32 records, where the lapping call overwrites exactly one block)"""
    w = world(name)
    p = Path(path, D, w)
    shape_b(p, run(p, RM.schedule_b(w.adds, p.cap, lag=1, sync=False)), min_lost=2 if name == "burst" else 1)
    p.dec.close()


@pytest.mark.parametrize("sync", [True, False], ids=["sync", "nosync"])
@pytest.mark.parametrize("path", OTHER)
def test_schedule_d_b_with_lag_2(D, path, sync):
    """the same lap met two calls behind: the collect's own part ends a call earlier than in B, the loss is the same"""
    w = world("burst")
    p = Path(path, D, w)
    assert p.max_lag >= 2 and p.cap == 256
    n = RM.first_silent_lap(w.adds, p.cap, 2)
    assert w.adds[n - 2] > 0                                      # (so lag 2 claims fewer blocks than lag 1 would)
    shape_b(p, run(p, RM.schedule_b(w.adds, p.cap, lag=2, sync=sync)), lag=2)
    p.dec.close()


@pytest.mark.parametrize("path", OTHER)
def test_schedule_e_a_host_that_keeps_up_never_loses(D, path):
    """every lag in 0 .. acg_max_lag, a full-size buffer, a collect after every call: never ACG_EOVERFLOW, lost_blocks 0, the
    oracle's output complete"""
    w = world("lag2")
    p = Path(path, D, w)
    n = 64
    for lag in range(p.max_lag + 1):
        p.dec.reset()
        p.blocks_seen = p.lost_seen = 0
        steps = []
        for k in range(n):
            steps += [("process", k), ("collect", lag, BIG)]
        log = run(p, steps + [("drain_all", BIG)])
        assert all(e.rc == p.K.OK and e.lost == 0 for e in log), lag
        assert sum(e.nrecs for e in log) == sum(1 for key, b in w.blocks.items() if b.call < n and p.expected(key) is not None) >= 20
        if lag:
            assert all(e.take == w.adds[e.issued - 1 - lag] for e in log[lag:n])     # each collect: exactly the call `lag` back
    p.dec.close()


# ---- F: the laps at the wrap of the 32-bit counters ----------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ["A", "B"])
@pytest.mark.parametrize("path", OTHER)
def test_schedule_f_laps_at_the_wrap_of_the_counters(D, path, schedule):
    """the counters preset to 2^32 - back, so that block number `back` of the run is the one counted 0: 2^32 inside the lost run
    (0 < back < lost), exactly at upto - cap (back = lost: the first survivor is counted 0) and inside the survivors of the first
    claim's mark (lost < back < lost + survivors): three distinct places, and in each the run from 0, shifted"""
    w = world("small" if schedule == "A" else "burst")
    p = Path(path, D, w)
    if schedule == "A":
        steps, lost, survivors = RM.schedule_a(w.adds, small=5), sum(w.adds) - p.cap, p.cap
    else:
        steps = RM.schedule_b(w.adds, p.cap, lag=1)
        cnt = np.cumsum(w.adds)
        n = RM.first_silent_lap(w.adds, p.cap, 1)
        lost = int(cnt[n - 1]) - p.cap
        survivors = int(cnt[n - 2]) - lost                       # of the collect's own part
    places = dict(in_the_lost_run=lost // 2, at_upto_minus_cap=lost, in_the_survivors=lost + survivors // 2)
    assert 0 < places["in_the_lost_run"] < lost == places["at_upto_minus_cap"] < places["in_the_survivors"] < lost + survivors
    base = None
    for where, back in places.items():
        p.dec.reset()
        p.blocks_seen = p.lost_seen = 0
        log = run(p, steps, start=(1 << 32) - back)
        (shape_a if schedule == "A" else shape_b)(p, log)
        assert log[0].lost == lost and log[0].first == lost and sum(e.take for e in log if e.first < lost + survivors) == survivors
        view = [(e.rc, e.lost, e.first, e.take, e.nrecs) for e in log]
        base = base or view
        assert view == base, where
    p.dec.close()
