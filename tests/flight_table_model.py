"""What the flight table's slots do, restated for tests (acarsdec_amd/csrc/flight.hip, THE TABLE): the key and the hash that place an
aircraft, addresses that share a home slot, a record builder, the list walk with the aircraft a call dropped left out, a condition
under which no claim order can drop anybody, and the traffic of tests/test_gpu_flight_pressure.py.  tests/test_flight_table_model.py
proves the conditions of that traffic on this side alone; the GPU tests then hold the device to the list walk.

Slot positions are never modelled: which slot a new aircraft takes depends on the race between the waves of a pass and cannot be
observed.  What can be observed -- who is in the table, with which bytes, and how many were dropped -- is determined in every
traffic below, and the docstrings say why."""
import ctypes as C
import functools

import numpy as np

import flight_model as FM
import label_model as LM

FL_PROBE = 128                                        # flight.hip: a lookup and a claim end after this many slots
MDLY = 2
EVENT_LABELS = (b"QP", b"QA", b"QN", b"12", b"H1")    # all inside the -b list of tests/test_gpu_flights.py: every record is an event
HOT = b"HOT1"
M64 = (1 << 64) - 1


def _gf():
    """tests/test_gpu_flights.py, for its label_text(), T0 and -b list (imported when first used, not copied)"""
    import test_gpu_flights
    return test_gpu_flights


def filter_kw():
    return dict(downlink_only=True, skip_empty=True, labels=_gf().LABELS_B)


# ---- key and hash ------------------------------------------------------------------------------------------------------------
def key_of(addr):
    """flight_extract_kernel's key of an address: its first 7 bytes as a little-endian word, cut at the first NUL, bit 63 set"""
    return int.from_bytes(bytes(addr)[:7].split(b"\0")[0], "little") | (1 << 63)


def fl_hash(k):
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M64
    k ^= k >> 33
    return k & 0xffffffff


def home(addr, cap):
    """The slot an aircraft's probe path starts at: fl_hash (the 64-bit finaliser, its low 32 bits) & (cap - 1), in Python
    integers.  THIS PINS THE HASH: the crowded-window tests of tests/test_gpu_flight_pressure.py put 128 aircraft on one home
    slot found with this function and expect the 129th to be dropped.  If the device's hash or key drifts from this restatement,
    the addresses spread out, nothing is dropped and those tests fail -- that is the cross-check, there is no other."""
    assert cap > 0 and cap & (cap - 1) == 0
    return fl_hash(key_of(addr)) & (cap - 1)


@functools.lru_cache(maxsize=None)
def _hashes(c):
    """fl_hash of b"%c%05d" % (c, i) for i = 0 .. 99999"""
    return tuple(fl_hash(key_of(b"%c%05d" % (c, i))) for i in range(100000))


def same_home(cap, h, n, prefix):
    """n distinct 6-character addresses whose home in a table of `cap` slots is h: b"%c%05d" enumerated, for each character of
    `prefix` in turn (one character gives about 100 000 / cap of them)"""
    out = []
    for c in bytes(prefix):
        for i, x in enumerate(_hashes(c)):
            if x & (cap - 1) == h:
                out.append(b"%c%05d" % (c, i))
                if len(out) == n:
                    return out
    raise ValueError("only %d addresses with home %d under %r" % (len(out), h, prefix))


# ---- records -----------------------------------------------------------------------------------------------------------------
def build_records(rng, items, nch=64, soh_back=(600, 10200)):
    """One split record per (addr, end_sample) of `items`, in that order: a downlink with bs = STX (so every record reaches
    addFlight()), label and text from test_gpu_flights.label_text() so that routes and OOOI fields occur, one text in seven
    empty (-e then keeps the message away from routejson()), one flight id in ten empty; the SOH lies soh_back samples before
    the end (a block of 13 .. 241 bytes by default: tv runs backwards between neighbours)."""
    from acarsdec_amd import _capi as K
    label_text = _gf().label_text
    recs = (K.Msg * max(len(items), 1))()
    for i, (addr, end) in enumerate(items):
        m = recs[i]
        m.chn = int(rng.integers(0, nch))
        m.end_sample = int(end)
        m.end_bit = int(end) // 5
        m.soh_sample = int(end) - int(rng.integers(soh_back[0], soh_back[1]))
        m.mode = b"2"
        m.addr = addr
        m.bid = b"5"
        m.down = b"\x01"
        m.ack = b"!"
        lab = EVENT_LABELS[int(rng.integers(0, len(EVENT_LABELS)))]
        m.label = lab
        m.bs = b"\x02"
        m.be = b"\x03"
        m.no = b"M01A"
        m.fid = b"" if rng.random() < 0.1 else b"XY%04d" % int(rng.integers(0, 40))
        if rng.random() < 0.85:
            t = label_text(rng, lab)
            C.memmove(C.addressof(m) + K.Msg.txt.offset, t, len(t))
            m.txt_len = len(t)
    return recs


def events_of(recs, n):
    """the events of recs[0 .. n) under the filters the GPU tests set (-A, -e and the -b list of tests/test_gpu_flights.py)"""
    kw = filter_kw()
    mkw = dict(downlink_only=kw["downlink_only"], skip_empty=kw["skip_empty"], labels=LM.parse_label_filter(kw["labels"]))
    return [FM.event_of(recs[i], _gf().T0, **mkw) for i in range(n)]


class Traffic:
    """records in time order, cut into batches; .batches = the events of each batch (every record is one)"""

    def __init__(self, recs, sizes, evs=None, **meta):
        self.recs, self.sizes, self.n = recs, list(sizes), sum(sizes)
        self.__dict__.update(meta)
        evs = events_of(recs, self.n) if evs is None else evs
        assert all(e is not None for e in evs), "a record that is no event"
        assert len({(e.end, e.chn) for e in evs}) == len(evs), "two events with the same sort key: their order would be unspecified"
        self.batches, at = [], 0
        for s in self.sizes:
            self.batches.append(evs[at:at + s])
            at += s

    def shuffled(self, rng, nbatch=None):
        """the records of the first nbatch batches, in an arbitrary order inside each batch (as the block queue delivers them)"""
        from acarsdec_amd import _capi as K
        sizes = self.sizes[:nbatch]
        out, at, sz = (K.Msg * max(sum(sizes), 1))(), 0, C.sizeof(K.Msg)
        for s in sizes:
            for j, i in enumerate(rng.permutation(s)):
                C.memmove(C.addressof(out) + (at + j) * sz, C.addressof(self.recs) + (at + int(i)) * sz, sz)
            at += s
        return out


def addr8(a):
    return FM.cstr(a, 8)


# ---- the list walk, minus what a call dropped --------------------------------------------------------------------------------
def expect_without(walk_kw, batches, dropped_addrs_per_batch):
    """The ListWalk of tests/flight_model.py over `batches` (lists of events, applied in batch_order), leaving out in each batch
    the events of the aircraft that batch dropped: ([the entries' bytes after every batch], [the routes' bytes], drops).

    This is the documented behaviour (flight table): an aircraft that finds no slot is counted once per call in
    which it has messages, and its messages of that call reach neither the table nor the route queue.  They were still seen:
    G, the newest second, moves with every event, so a left-out event still runs the list's expiry scan (output.c:407-423)."""
    walk = FM.ListWalk(**walk_kw)
    snaps, drops = [], 0
    for evs, gone in zip(batches, dropped_addrs_per_batch):
        gone = {addr8(a) for a in gone}
        drops += len(gone & {e.addr for e in evs})
        for e in FM.batch_order(evs):
            if e.addr in gone:
                walk.head = [f for f in walk.head if not f["tl"][0] < e.sec - walk.mdly]
            else:
                walk.add(e)
        snaps.append([FM.flight_bytes(f) for f in walk.entries()])
    return snaps, [FM.route_bytes(r) for r in walk.routes], drops


def live_before(batches, mdly):
    """per batch: the entries the list holds when the batch starts.  These are the entries with tl_sec + mdly >= G (the lazy rule
    equals the list walk: tests/test_flight_model.py), i.e. the slots a claim of that batch must not take."""
    walk, out = FM.ListWalk(mdly), []
    for evs in batches:
        out.append(len(walk.entries()))
        for e in FM.batch_order(evs):
            walk.add(e)
    return out


def claimable_everywhere(batches, mdly, reach):
    """A sufficient condition for 'no aircraft is dropped, whatever order the claims of a pass come in': for every batch,
    (entries live before the batch) + (distinct aircraft in the batch) <= reach - 1.

    A claim may take any slot of its `reach`-slot window that is neither live with respect to G before the pass nor marked by
    this pass.  Live slots: at most the first term.  Marked slots: one per aircraft of the batch that was found or has claimed,
    so at most the second term minus the claimant itself.  If the sum is at most reach - 1, fewer than `reach` slots of ANY
    window are barred, and the probe finds one.  Only the list walk is needed -- no slot positions, which depend on the race."""
    return all(l + len({e.addr for e in evs}) <= reach - 1 for l, evs in zip(live_before(batches, mdly), batches))


# ---- (a) a table many times older than its size ------------------------------------------------------------------------------
AGED_AIRCRAFT, AGED_RATE, AGED_RETURNS = 20000, 24.0, 500


@functools.lru_cache(maxsize=None)
def aged_traffic():
    """AGED_AIRCRAFT aircraft b"N%05d" arriving AGED_RATE a second, each with 1 .. 3 messages 20 .. 400 ms apart; HOT with a message
    every 40 ms on average and never more than 150 ms apart; AGED_RETURNS aircraft heard once more, half of them 5 .. 7 s after
    their last message (expired, their slot probably still carries their key), half 100 .. 400 s after it (some 2 400 .. 9 600
    aircraft later).  Batch sizes are drawn from 1 .. 400 and cut where claimable_everywhere(.., reach = FL_PROBE) would fail."""
    rng = np.random.default_rng(20261019)
    first = (np.arange(AGED_AIRCRAFT) + rng.random(AGED_AIRCRAFT)) / AGED_RATE + 1.0
    times, addrs, last = [], [], np.zeros(AGED_AIRCRAFT)
    for i in range(AGED_AIRCRAFT):
        t = float(first[i])
        for _ in range(int(rng.integers(1, 4))):
            times.append(t)
            addrs.append(b"N%05d" % i)
            last[i] = t
            t += float(rng.uniform(0.02, 0.4))
    back = rng.permutation(AGED_AIRCRAFT // 2)[:AGED_RETURNS]          # (the first half: the late return still lies inside the traffic)
    for k, i in enumerate(back):
        times.append(float(last[i]) + float(rng.uniform(5.0, 7.0) if k % 2 else rng.uniform(100.0, 400.0)))
        addrs.append(b"N%05d" % i)
    t, end = 1.0, max(times) + 0.1
    while t < end:
        times.append(t)
        addrs.append(HOT)
        t += min(float(rng.exponential(0.04)), 0.15)
    order = np.argsort(np.asarray(times), kind="stable")
    ends, prev = [], 0
    for i in order:
        prev = max(int(round(times[i] * 12500)), prev + 1)             # distinct end samples: the order of a batch is determined
        ends.append(prev)
    recs = build_records(rng, [(addrs[i], e) for i, e in zip(order, ends)], nch=1024)
    evs = events_of(recs, len(ends))
    walk, sizes, at = FM.ListWalk(MDLY), [], 0
    while at < len(evs):
        want, live, seen, s = int(rng.integers(1, 401)), len(walk.entries()), set(), 0
        while s < want and at + s < len(evs) and live + len(seen | {evs[at + s].addr}) <= FL_PROBE - 1:
            seen.add(evs[at + s].addr)
            s += 1
        assert s >= 1, "more than %d live entries: no batch fits" % (FL_PROBE - 2)
        for e in FM.batch_order(evs[at:at + s]):
            walk.add(e)
        sizes.append(s)
        at += s
    return Traffic(recs, sizes, evs=evs, returned=[b"N%05d" % i for i in back])


@functools.lru_cache(maxsize=None)
def aged_expected():
    """the plain list walk over aged_traffic(): computed once, shared by every test that needs it, never changed"""
    tr = aged_traffic()
    return expect_without(dict(mdly=MDLY), tr.batches, [()] * len(tr.batches))


# ---- (b), (c) one probe window filled one aircraft at a time -----------------------------------------------------------------
CAP = 1024
STEP = 63                                             # samples between two events: 5 ms


def _other_home(cap, hs, prefix):
    """one address per home slot of hs"""
    return [same_home(cap, h % cap, 1, prefix)[0] for h in hs]


@functools.lru_cache(maxsize=None)
def window_traffic(h, full):
    """The batches of the crowded-window test around home slot h of a 1024-slot table; .step maps a step's name to its batch.
    One new aircraft per batch, so the slots ARE determined here: S[i] sits i slots behind h.

      fill      S[0 .. 127], one per batch, 5 ms apart: all stay live and occupy the whole window
      alone     S[128] alone: every slot of its window is live -> dropped
      with3     S[128] with a message of S[3]: dropped again, S[3] updated
      plus64    (full) an aircraft with home h + 64: its window reaches 64 slots past the crowd -> fits
      minus1    (full) an aircraft with home h - 1: its own home is empty -> fits
      keep      S[7] once a second for 9 s: it alone stays live while S[0 .. 6] before it on its path expire, and every lookup from
                the third second on has to walk past their expired keys to find it (one entry, nbm 2 .. 10)
      clock     10 s after the fill a message of an aircraft from the far side of the table: all but S[7] have expired
      back      S[128] and S[5]: S[5] finds its own tombstone and restarts in place, S[128] takes one that this pass did not mark
      s0        (full) S[0] again: its tombstone is the first on the path and has probably gone to S[128] -> a fresh entry
      s5        (full) S[5] once more: found where it is, nbm = 2"""
    rng = np.random.default_rng(1000 + h)
    S = same_home(CAP, h, 131, b"ST")
    plus64, minus1, clock = _other_home(CAP, (h + 64, h - 1, h + 512), b"P")
    batches, step, t = [], {}, 30000

    def batch(name, addrs, gap=STEP):
        nonlocal t
        items = []
        for k, a in enumerate(addrs):
            t += gap if k == 0 else STEP
            items.append((a, t))
        step[name] = len(batches)
        batches.append(items)

    for i in range(128):
        batch("fill", [S[i]])
    batch("alone", [S[128]])
    batch("with3", [S[128], S[3]])
    if full:
        batch("plus64", [plus64])
        batch("minus1", [minus1])
    for _ in range(9):
        batch("keep", [S[7]], gap=12500)
    batch("clock", [clock], gap=12500)
    batch("back", [S[128], S[5]])
    if full:
        batch("s0", [S[0]])
        batch("s5", [S[5]])
    recs = build_records(rng, [it for b in batches for it in b], soh_back=(600, 1200))
    gone = [()] * len(batches)
    gone[step["alone"]] = gone[step["with3"]] = (S[128],)
    return Traffic(recs, [len(b) for b in batches], S=S, step=step, gone=gone, others=dict(plus64=plus64, minus1=minus1, clock=clock))


# ---- (d) contended claims, (e) more new aircraft than free slots -------------------------------------------------------------
def _crowd(rng, S, nseq, new, per_new, old):
    """nseq aircraft of S one per batch, then ONE batch: per_new() events of each aircraft of `new` and one of each of `old`,
    interleaved at random, 20 samples apart"""
    batches, t = [], 30000
    for i in range(nseq):
        t += STEP
        batches.append([(S[i], t)])
    pool = [a for a in new for _ in range(per_new())] + list(old)
    big = []
    for i in rng.permutation(len(pool)):
        t += 20
        big.append((pool[int(i)], t))
    batches.append(big)
    return batches, t


@functools.lru_cache(maxsize=None)
def contended_traffic(h=400):
    """28 aircraft of one home slot, one per batch, kept alive; then ONE batch with 100 new ones of the same home (2 .. 5 events
    each) and 60 events of the 28: 128 aircraft for the 128 slots of the window, the 100 claims racing for the 100 free slots --
    all fit only if no claim wastes a slot or shares one.  Then a batch with 5 more of that home and 40 aircraft from elsewhere
    (homes 200 .. 590 slots on, one each): the window is full of live entries, so NONE of the five can fit whatever the order
    -- the dropped identities are determined -- and the 40 fit."""
    rng = np.random.default_rng(77)
    S = same_home(CAP, h, 140, b"ST")
    batches, t = _crowd(rng, S, 28, S[28:128], lambda: int(rng.integers(2, 6)), S[:28] + [S[int(i)] for i in rng.integers(0, 28, 32)])
    others = _other_home(CAP, [h + 200 + 10 * j for j in range(40)], b"P")
    last = [S[128 + int(i) % 5] for i in range(8)] + others
    nxt = []
    for i in rng.permutation(len(last)):
        t += 20
        nxt.append((last[int(i)], t))
    batches.append(nxt)
    recs = build_records(rng, [it for b in batches for it in b], soh_back=(600, 1200))
    gone = [()] * (len(batches) - 1) + [tuple(S[128:133])]
    return Traffic(recs, [len(b) for b in batches], S=S, gone=gone, others=others)


@functools.lru_cache(maxsize=None)
def overfull_traffic(h=700):
    """120 aircraft of one home slot, one per batch, kept alive; then ONE batch with 20 new ones of that home, 3 .. 5 events each:
    8 slots for 20 claims.  Which 8 get them is unspecified; that exactly 12 are dropped is not."""
    rng = np.random.default_rng(78)
    S = same_home(CAP, h, 140, b"ST")
    batches, _ = _crowd(rng, S, 120, S[120:140], lambda: int(rng.integers(3, 6)), [S[int(i)] for i in rng.integers(0, 120, 30)])
    recs = build_records(rng, [it for b in batches for it in b], soh_back=(600, 1200))
    return Traffic(recs, [len(b) for b in batches], S=S)
