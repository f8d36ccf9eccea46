"""What the reassembly table's slots do, restated for tests (acarsdec_amd/csrc/reasm.hip: reasm_extract_kernel's key words, rs_hash,
reasm_heads_kernel's lookup, reasm_claim): the two key words and the hash that place a chain, keys that share a home slot, the
expectation with the keys that found no slot left out, and the traffic of tests/test_gpu_reasm_pressure.py.
tests/test_reasm_table_model.py proves the premises of that traffic on this side alone; the GPU tests then hold the device to
tests/reasm_model.py, as tests/flight_table_model.py does for the flight table.

Slot positions are never modelled: which slot a new key takes depends on the race between the waves of a pass.  What can be observed
-- every block's status, the completed messages and `dropped` -- is determined in every traffic below but one (which 28 of 40 racing
keys win), and there the counts and every key's own consistency are."""
import ctypes as C
import functools
import random
import types

from acarsdec_amd import _capi as K

import reasm_cases as RC
import reasm_model as RM

RS_PROBE = 128                                        # reasm.hip: a lookup and a claim end after this many slots
M64 = (1 << 64) - 1
T0 = (1700000000, 250000)
T0_US = T0[0] * 10**6 + T0[1]
S2, S90, S660 = 25000, 1125000, 8250000               # 2 s (the take-over margin), VAT4 and VGT4 in 12.5 kHz samples
assert S2 * RM.SAMPLE_US == RM.RECLAIM_US and S90 * RM.SAMPLE_US == RM.VAT4_US and S660 * RM.SAMPLE_US == RM.VGT4_US


# ---- key words and hash --------------------------------------------------------------------------------------------------------
def _word(b, n):
    """n bytes as a little-endian word, a C string: nothing behind its NUL counts (rs_cstr)"""
    return int.from_bytes(RM.cstr(bytes(b)[:n]), "little")


def key_words(addr, label, msn, down):
    """(k0, k1) of reasm_extract_kernel: k0 = addr as a C string of 7 bytes, label[0] in bits 56 and up; k1 = label[1], the
    downlink's msn as a C string of 3 bytes in bits 8 and up (an uplink: none), bit 63 set"""
    lab = _word(label, 2)
    return (_word(addr, 7) | ((lab & 0xff) << 56), (lab >> 8) | ((_word(msn, 3) if down else 0) << 8) | (1 << 63))


def key_words_of(m):
    """... of a record"""
    return key_words(RM.raw(m, "addr", 7), RM.raw(m, "label", 2), RM.raw(m, "no", 3), 0x30 <= RM._c(m.bid) <= 0x39)


def rs_hash(k0, k1):
    k = k0 ^ ((k1 * 0x9e3779b97f4a7c15) & M64)
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M64
    k ^= k >> 33
    return k & 0xffffffff


def home(key, cap):
    """The slot a key's probe path starts at: rs_hash of its two words & (cap - 1).  THIS PINS THE KEY WORDS AND THE HASH: the
    window tests of tests/test_gpu_reasm_pressure.py put 128 keys on one home found with this function and expect the 129th to
    find no slot.  If the device's words or hash drift from this restatement the keys spread out, nothing is dropped and those
    tests fail -- that is the cross-check, there is no other."""
    assert cap > 0 and cap & (cap - 1) == 0
    return rs_hash(*key) & (cap - 1)


def make_key(c, i):
    """the i-th enumerated key under prefix character c: every fourth an uplink (no msn in its key), the others downlinks with
    one of 100 message numbers and one of three labels"""
    up = i % 4 == 3
    return types.SimpleNamespace(addr=b"%c%05d" % (c, i), label=(b"H1", b"5Z", b"80")[i % 3], msn=b"" if up else b"K%02d" % (i % 100), up=up)


def words(k):
    return key_words(k.addr, k.label, k.msn, not k.up)


@functools.lru_cache(maxsize=None)
def _hashes(c):
    return tuple(rs_hash(*words(make_key(c, i))) for i in range(100000))


def same_home(cap, h, n, prefix=b"ST", kinds="both"):
    """n distinct keys whose home in a table of `cap` slots is h: make_key enumerated for each character of `prefix` in turn.
    kinds: "both" (downlinks and uplinks as they come, both kinds present), "down" or "up" """
    out = []
    for c in bytes(prefix):
        for i, x in enumerate(_hashes(c)):
            if x & (cap - 1) == h % cap:
                k = make_key(c, i)
                if kinds == "both" or (kinds == "up") == k.up:
                    out.append(k)
                    if len(out) == n:
                        assert kinds != "both" or n < 8 or {k.up for k in out} == {False, True}
                        return out
    raise ValueError("only %d keys with home %d under %r" % (len(out), h, prefix))


# ---- records -------------------------------------------------------------------------------------------------------------------
def block(k, blk, final, soh, n, txt):
    """block `blk` (0 = A) of key k's chain with its SOH at sample `soh`; n numbers the record: its channel and its length"""
    back = 600 + (n * 37) % 9000
    if k.up:
        return RC.msg(addr=k.addr, label=k.label, bid=bytes([65 + blk]), no=b"", be=RC.ETX if final else RC.ETB, txt=txt, end_sample=soh + back, chn=n % 8, back=back)
    return RC.msg(addr=k.addr, label=k.label, bid=b"1", no=k.msn + bytes([65 + blk]), be=RC.ETX if final else RC.ETB, txt=txt, end_sample=soh + back, chn=n % 8, back=back)


class Scenario:
    """msgs in calls of `batches` records, each call's records shuffled; lost: the indices of the records whose key finds no slot
    in their call; note: names for record indices and lists of them"""

    def __init__(self, seed, cap):
        self.rng = random.Random(seed)
        self.cap = cap
        self.msgs, self.batches, self.lost, self.note, self.keys = [], [], [], {}, {}
        self.G = 0                                    # the largest SOH sample so far: what the device's G stands at after the call

    def call(self, name, items, lost=False):
        """one call: items = (key, blk, final, soh); returns the records' indices in the order of `items`"""
        at = len(self.msgs)
        recs = [block(k, blk, final, soh, at + j, self._text_for(at + j)) for j, (k, blk, final, soh) in enumerate(items)]
        order = list(range(len(recs)))
        self.rng.shuffle(order)
        where = [0] * len(recs)
        for pos, j in enumerate(order):
            where[j] = at + pos
        self.msgs += [recs[j] for j in order]
        self.batches.append(len(recs))
        self.note.setdefault(name, []).extend(where)
        if lost:
            self.lost += where
        self.G = max([self.G] + [it[3] for it in items])
        return where

    def _text_for(self, n):
        """1, 2, 3 or 5 printable bytes: a row's last dword is incomplete when its slot changes hands"""
        return bytes(self.rng.randrange(0x21, 0x7f) for _ in range((1, 2, 3, 5)[n % 4]))

    def behind(self):
        """a SOH sample at or below G that no earlier record of this kind used: the record leaves G where it is"""
        self._b = getattr(self, "_b", 0) + 1
        return self.G - 40 - self._b


def no_slot_status(m):
    """what the walk gives a block whose key has neither an entry nor a slot: UNKNOWN where the block would create the entry"""
    down = 0x30 <= RM._c(m.bid) <= 0x39
    if down and RM._sc(RM.raw(m, "no", 4)[3:4]) - 65 != 0:
        return RM.OUT_OF_SEQUENCE
    if RM._c(m.be) != RM.ETB:
        return RM.SKIPPED
    return RM.UNKNOWN


def _without(msgs, batches, lost):
    lost = set(lost)
    kept = [i for i in range(len(msgs)) if i not in lost]
    sizes, dropped, at = [], 0, 0
    for n in batches:
        sizes.append(sum(1 for i in range(at, at + n) if i not in lost))
        dropped += len({RM.key_of(msgs[i]) for i in range(at, at + n) if i in lost and RM.creates(msgs[i])})
        at += n
    return kept, sizes, dropped


def expect(msgs, batches, lost, t0_us=T0_US, reclaim=False):
    """(statuses, completed tuples, dropped): reasm_model.run over the same calls without the records of `lost`; those get what a
    block without an entry and without a slot gets.  dropped: once per call and key that found no slot."""
    kept, sizes, dropped = _without(msgs, batches, lost)
    st, done, _ = RM.run([msgs[i] for i in kept], sizes, t0_us=t0_us, reclaim=reclaim)
    status = [None] * len(msgs)
    for i, s in zip(kept, st):
        status[i] = s
    for i in lost:
        status[i] = no_slot_status(msgs[i])
    return status, RC.completed_tuples(done), dropped


def occupancy(msgs, batches, lost, t0_us=T0_US):
    """per call: (the entries no claim may take: live and not expired by more than 2 s against G when the call starts, the new keys
    of the call that find a slot, the keys of the call that find none).  The reclaiming model's table is exactly the first."""
    kept, sizes, _ = _without(msgs, batches, lost)
    lostset = set(lost)
    t = RM.Table(t0_us, reclaim=True)
    out, at, full = [], 0, 0
    for n, nfull in zip(sizes, batches):
        t.begin_call()
        before = set(t.table)
        part = [msgs[i] for i in kept[at:at + n]]
        new = {RM.key_of(m) for m in part if RM.creates(m)} - before
        for i in RM.call_order(part):
            t.add(part[i])
        out.append((len(before), len(new), len({RM.key_of(msgs[i]) for i in range(full, full + nfull) if i in lostset})))
        at += n
        full += nfull
    return out


# ---- (a) the expiry take-over at its edge ------------------------------------------------------------------------------------------
A_UP = tuple(3 + 4 * k for k in range(28))            # which of the 128 first chains are uplinks: 3 is the earliest of them


def a_first(i):
    return 100000 + 700 * i                           # the SOH sample of chain i's first block


@functools.lru_cache(maxsize=None)
def expiry_takeover():
    """A table of 128 slots (one probe window) filled by 100 downlink and 28 uplink chains, then single-record calls around the
    moment the earliest uplink entry, then the earliest downlink entry, becomes claimable: G > first + time-out + 2 s, strictly.
    A lone final block of a foreign key is an event that takes no slot and moves G; every other record of those calls lies at or
    below G and leaves it alone.  See the steps below; sc.note names them."""
    sc = Scenario(11, 128)
    downs = [types.SimpleNamespace(addr=b"D%05d" % i, label=b"H1", msn=b"M%02d" % (i % 100), up=False) for i in range(128)]
    ups = [types.SimpleNamespace(addr=b"U%05d" % i, label=b"5Z", msn=b"", up=True) for i in range(128)]
    old = [ups[i] if i in A_UP else downs[i] for i in range(128)]
    new = iter(types.SimpleNamespace(addr=b"N%05d" % i, label=b"80", msn=b"" if i % 3 == 2 and i >= 40 else b"Q%02d" % (i % 100), up=i % 3 == 2 and i >= 40)
               for i in range(1000))                                         # the first 40 are downlinks: they outlive the steps
    foreign = types.SimpleNamespace(addr=b"FOREIGN", label=b"H1", msn=b"F00", up=False)
    sc.keys.update(old=old)
    sc.call("fill", [(old[i], 0, False, a_first(i)) for i in range(128)])

    def move_G(name, soh):
        sc.call(name, [(foreign, 0, True, soh)])                            # a lone final block: SKIPPED by the walk, no slot

    def newcomer(name, lost):
        k = next(new)
        sc.call(name, [(k, 0, False, sc.behind())], lost=lost)
        return k

    def edge(tag, first, timeout):
        newcomer(tag + "_full", True)                                        # 128 live entries: UNKNOWN
        move_G(tag + "_at", first + timeout + S2)                            # G == first + time-out + 2 s: not yet
        newcomer(tag + "_still", True)
        move_G(tag + "_past", first + timeout + S2 + 1)                      # one sample later: exactly one entry is claimable
        k = newcomer(tag + "_takes", False)
        again = newcomer(tag + "_fullagain", True)
        sc.call(tag + "_done", [(k, 1, True, sc.behind())])                 # completes in the slot it took over: its own text
        sc.call(tag + "_idle", [(again, 0, False, sc.behind())])            # ... whose slot, idle now, goes to the key that found none
        return k

    edge("up", a_first(A_UP[0]), S90)
    # the other 27 uplink entries expire within the next 75 600 samples: fill their slots, so that the table is full of entries
    # that last 660 s when G reaches the earliest downlink's edge
    move_G("up_all", a_first(A_UP[-1]) + S90 + S2 + 1)
    sc.keys["fillers"] = [next(new) for _ in range(27)]
    sc.call("fillers", [(k, 0, False, sc.behind()) for k in sc.keys["fillers"]])
    edge("down", a_first(0), S660)
    # past every entry's expiry: the newest entry began at or below G
    move_G("all", sc.G + S660 + S2 + 1000)
    sc.keys["last"] = [next(new) for _ in range(127)]
    sc.call("last", [(k, 0, False, sc.behind()) for k in sc.keys["last"]])
    sc.call("last_done", [(k, 1, True, sc.G + 100 + j) for j, k in enumerate(sc.keys["last"])])
    # the old keys come back: their entries expired long ago
    sc.call("old_b", [(k, 1, False, sc.G + 100 + j) for j, k in enumerate(old)])
    sc.call("old_c", [(k, 2, True, sc.G + 100 + j) for j, k in enumerate(old)])
    return sc


# ---- (b) the probe window inside a larger table ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def probe_window(h, cap=256):
    """128 keys of home h begin chains in one call of a `cap`-slot table and fill the window h .. h + 127 (mod cap); the 129th finds
    no slot although cap - 128 are free; keys of home h + 1 and h - 1 do; the 128 final blocks in one call; the 129th again."""
    sc = Scenario(1000 + h, cap)
    S = same_home(cap, h, 129)
    plus, minus = same_home(cap, h + 1, 1, b"P")[0], same_home(cap, h - 1, 1, b"P")[0]
    sc.keys.update(S=S, plus=plus, minus=minus)
    t = [50000]

    def at():
        t[0] += 300
        return t[0]

    sc.call("fill", [(k, 0, False, at()) for k in S[:128]])
    sc.call("129th", [(S[128], 0, False, at())], lost=True)
    sc.call("neighbours", [(plus, 0, False, at()), (minus, 0, False, at())])
    sc.call("finals", [(k, 1, True, at()) for k in S[:128]])
    sc.call("129th_again", [(S[128], 0, False, at())])
    sc.call("rest", [(k, 1, True, at()) for k in (S[128], plus, minus)])
    return sc


# ---- (c) claims racing in one pass -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def racing_claims():
    """100 chains live in a table of 128 slots; ONE call brings the first blocks of 40 new downlink keys: 28 slots for 40 claims.
    Which 28 get them is the race's; that exactly 12 find none is not.  Then all 140 final blocks in one call.  The records of the
    losers are not known here: sc.lost stays empty and the GPU test reads them off the statuses."""
    sc = Scenario(31, 128)
    old = [make_key(ord("R"), i) for i in range(100)]
    new = [k for k in (make_key(ord("W"), i) for i in range(60)) if not k.up][:40]
    sc.keys.update(old=old, new=new)
    t = [70000]

    def at():
        t[0] += 300
        return t[0]

    sc.call("old", [(k, 0, False, at()) for k in old])
    sc.call("new", [(k, 0, False, at()) for k in new])
    sc.call("finals", [(k, 1, True, at()) for k in old + new])
    return sc


# ---- (d) large sample indices ------------------------------------------------------------------------------------------------------
OFFSETS = ((1 << 32) - 10**6, 1 << 42)


def shifted(msgs, off):
    """copies of the records with end_sample and soh_sample `off` samples later (end_bit stays: bits are counted on their own)"""
    out = []
    for m in msgs:
        c = K.Msg.from_buffer_copy(m)
        c.end_sample, c.soh_sample = m.end_sample + off, m.soh_sample + off
        out.append(c)
    return out


def shifted_done(done, off):
    """completed tuples with their three sample stamps `off` later"""
    return [d[:3] + (d[3] + off, d[4] + off, d[5] + off) + d[6:] for d in done]


def t0_before(off, t0_us=T0_US):
    """t0 moved back by `off` samples: (sec, usec), and the same in microseconds"""
    us = t0_us - RM.SAMPLE_US * off
    return (us // 10**6, us % 10**6), us


def straddles(msgs, batches, off, bit=32):
    """the calls that hold end samples on both sides of 2^bit once shifted by `off`"""
    out, at = [], 0
    for b, n in enumerate(batches):
        side = {(m.end_sample + off) >> bit for m in msgs[at:at + n]}
        if len(side) > 1:
            out.append(b)
        at += n
    return out


@functools.lru_cache(maxsize=None)
def large_index_traffic():
    """(msgs, batches): RC.random_traffic() in shuffled calls of up to 2000 records, the first seed of RC.random_batches with which
    one call straddles 2^32 under OFFSETS[0]"""
    traffic = RC.random_traffic()
    for seed in range(100):
        batches = RC.random_batches(len(traffic), seed=seed)
        if straddles(traffic, batches, OFFSETS[0]):
            return RC.shuffled_within(traffic, batches, seed=seed + 50), batches
    raise ValueError("no call straddles 2^32")
