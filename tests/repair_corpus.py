"""One deterministic corpus of crafted transmissions for the block repair (acars.c:93-215; csrc/blk.hip blk_repair_kernel;
oracle/acars_oracle.c orc_blk_process), and a third, independent opinion on every block: the repair restated in Python
integers.  Plain module (like label_model.py): tests/test_repair_corpus.py runs it on the CPU against the oracle and the real
blk_thread, tests/test_gpu_repair.py on the device.  `python -m tests.repair_corpus` prints the category counts.

What the corpus is for (none of it is reached by the random short blocks of the other tests):
  * blocks of every length the framing can queue, 13 .. 241 bytes: a wave's lane L holds bytes L, L + 64, L + 128, L + 192, so
    every byte at index >= 64 is a different register, ballot and write-back of the kernel;
  * damage at CHOSEN positions: every byte index, the slot boundaries (63 / 64, 127 / 128, 191 / 192), two flagged bytes in
    the same lane (64 apart), first and last byte, byte 12 (whose STX / ETX bits acars.c:132-133 forces before the parity count);
  * ORDER-SENSITIVE blocks, found by search: the CRC has 17 acceptable remainders (0 and the syndromes of the 16 bits of the
    CRC bytes), fixprerr tries up to 512 candidates and fixdberr 28 * len, so some damaged blocks have more than one
    acceptable candidate and the reference delivers the FIRST of its loop order -- which may not be the damage that was
    injected.  `mine_*` draw damage, evaluate all candidates by syndrome arithmetic and keep the blocks where that matters;
  * the longest block: a 241-byte block indexes syndrome row len - i + 1 = 242 at i = 0 (acars.c:46,78), one row beyond the
    reference's table (syndrom.h: rows 0..241).  The device and the oracle define that row by the table's recurrence; the real
    blk_thread reads out of bounds there, so the leg that runs it leaves those blocks (and only those) out.

The audio is noiseless, so the block the demodulator queues is the crafted one, byte for byte (the CPU test asserts it).  One
thing is left to the oracle's demodulator when the corpus is laid out (`place`): the carrier phase / offset of a transmission is
re-drawn where the reference's loop would not lock onto it (a few per cent of the draws, noise or no noise).

Two readings of the specification that the framing forces (acars.c:303-341), stated here because the tests assert them:
  * the terminator of a 239 .. 241-byte block cannot be damaged and still be queued (the block runs into the length reset,
    acars.c:334), and a 13 .. 17-byte block whose terminator is damaged is never queued either (the DEL rule needs len > 20,
    acars.c:324).  For lengths 18 .. 238 a damaged terminator is exactly the "block that ends at DEL" case: the CRC bytes are
    taken as text, DEL takes them back (acars.c:326-329), and the block queued is the crafted one.  So "every byte index" of a
    241-byte block is 0 .. 239, and byte 12 holding ETX (a 13-byte block) can only lose its block: the corpus has those
    transmissions and checks that nothing is queued;
  * every fixdberr search of a 241-byte block that gets past the CRC bytes starts at k = 0, i.e. in row 242.  "Two bits in a byte
    at every index" is therefore laid on a 240-byte block (indices 0 .. 238 span all four slots and all three opinions, the
    real blk_thread included, see every one of them), and on the 241-byte block at every 16th index and the slot boundaries: the
    blocks the reference leg must leave out stay under 3 % of the corpus.
"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from acarsdec_amd import synth as S                                    # noqa: E402
from test_lean_framing_model import St, decode_acars, WSYN            # noqa: E402  (acars.c:246-375 in Python integers)

SEED = 241242
NCH, SLOTS, PERIOD, CALL = 1024, 3, 12288, 8 * 1024                    # channels, transmissions per channel, samples per slot / call
NSAMP = 5 * CALL                                                       # per channel (SLOTS * PERIOD = 4.5 calls)
TAIL, LEAD, END_MARGIN = 56, 1000, 200                                 # one-bits behind DEL; carrier before / behind a transmission
ETXP, ETBP, DELP, STXP = 0x83, 0x97, 0x7F, 0x02                        # with parity, as on the air
EDGE_LENS = (13, 14, 63, 64, 65, 127, 128, 129, 191, 192, 193, 239, 240, 241)
MAXPERR = 3


# ------------------------------------------------------------------------------------ tables (syndrom.h by its definition)
def _crc_update(crc, b):                                              # update_crc (syndrom.h:296), reflected CRC-CCITT
    return (crc >> 8) ^ int(S._CRC[(crc ^ b) & 0xFF])


def syndrome_table(rows=243):
    """entry i + 8 k: the remainder left by bit i of a byte that has k more bytes (text or CRC) behind it"""
    t, row = [], [int(S._CRC[1 << i]) for i in range(8)]
    for _ in range(rows):
        t += row
        row = [(s >> 8) ^ int(S._CRC[s & 0xFF]) for s in row]
    return t


SYND = syndrome_table()
ACCEPT = frozenset([0] + SYND[:16])                                    # acars.c:54-62 / 70-74
_SY = np.array(SYND, dtype=np.int64).reshape(-1, 8)
_PAIRS = [(a, b) for a in range(8) for b in range(a + 1, 8)]           # first appearance in the (i, j) loops of acars.c:79-80
_PAIR_SY = np.stack([_SY[:, a] ^ _SY[:, b] for a, b in _PAIRS], axis=1)      # [row, pair]
_ACC = np.array(sorted(ACCEPT), dtype=np.int64)


def popc(b):
    return bin(b).count("1")


# ------------------------------------------------------------------------------------ the repair, as written
def model_blk(ln, txt, crc0, crc1, mutate=None):
    """acars.c:123-207 on a raw block.  Returns dict(kept, err, txt (what outputmsg receives), rows (syndrome rows read),
    crc (the remainder the searches start from), pr (flagged bytes)).  `mutate` applies a deliberate fault of the kind a wave-wide
    search could have (tests only: shows that the corpus would notice): "db_from_64" starts fixdberr at k = 64, "last_hit" takes
    the last acceptable candidate instead of the first, "slot0" writes every fixprerr flip into index pr & 63."""
    rows = set()

    def syn(i):
        rows.add(i >> 3)
        return SYND[i]

    res = dict(kept=False, err=0, txt=None, rows=rows, crc=None, pr=[])
    if ln < 13:                                                        # acars.c:124
        return res
    t = bytearray(txt[:ln])
    t[12] = (t[12] & (ETXP | STXP)) | (ETXP & STXP)                    # acars.c:132-133
    pn, pr = 0, []
    for i in range(ln):                                                # acars.c:136-144
        if popc(t[i]) & 1 == 0:
            if pn < MAXPERR:
                pr.append(i)
            pn += 1
    res["pr"] = pr
    if pn > MAXPERR:                                                   # acars.c:145
        return res
    res["err"] = pn
    crc = 0
    for b in t:                                                        # acars.c:159-165
        crc = _crc_update(crc, b)
    crc = _crc_update(_crc_update(crc, crc0), crc1)
    res["crc"] = crc

    def fixprerr(crc, d):                                              # acars.c:39-64
        if d < pn:
            order = range(8) if mutate != "last_hit" else range(7, -1, -1)
            for i in order:
                if fixprerr(crc ^ syn(i + 8 * (ln - pr[d] + 1)), d + 1):
                    t[pr[d] & 63 if mutate == "slot0" else pr[d]] ^= 1 << i
                    return True
            return False
        if crc == 0:
            return True
        for i in range(16):
            if syn(i) == crc:
                return True
        return False

    def fixdberr(crc):                                                 # acars.c:66-90
        for i in range(16):
            if syn(i) == crc:
                return True
        ks = range(64 if mutate == "db_from_64" else 0, ln)
        for k in (reversed(ks) if mutate == "last_hit" else ks):
            bo = 8 * (ln - k + 1)
            for i in range(8):
                for j in range(8):
                    if i == j:
                        continue
                    if crc ^ syn(i + bo) ^ syn(j + bo) == 0:
                        t[k] ^= 1 << i
                        t[k] ^= 1 << j
                        return True
        return False

    if pn:                                                             # acars.c:170-192
        if not fixprerr(crc, 0):
            return res
    elif crc:
        if not fixdberr(crc):
            return res
    bad = 0
    for i in range(ln):                                                # acars.c:195-207
        bad += popc(t[i]) & 1 == 0
        t[i] &= 0x7F
    if bad:
        return res
    res["kept"], res["txt"] = True, bytes(t)
    return res


# ------------------------------------------------------------------------------------ all acceptable candidates, in the reference's order
def prerr_candidates(ln, crc, pr):
    """indices (i0 * 8^(pn-1) + ... : the recursion's visiting order) of every candidate fixprerr would accept"""
    c = np.array([crc], dtype=np.int64)
    for p in pr:
        c = (c[:, None] ^ _SY[ln - p + 1][None, :]).reshape(-1)
    return [int(i) for i in np.nonzero(np.isin(c, _ACC))[0]]


def dberr_candidates(ln, crc):
    """(k, i, j) of every candidate fixdberr would accept in its visiting order; (-1, 0, 0) = the CRC bytes' own 16 bits"""
    out = [(-1, 0, 0)] if crc in SYND[:16] else []
    rows = ln + 1 - np.arange(ln)
    k, p = np.nonzero(_PAIR_SY[rows] == crc)
    return out + sorted((int(kk),) + _PAIRS[int(pp)] for kk, pp in zip(k, p))


def damage_syndrome(ln, flips, crcflips=()):
    """remainder of a block whose clean form has remainder 0 (the CRC is linear): flips = [(index, mask)], crcflips = [(0 | 1, mask)]"""
    s = 0
    for i, m in flips:
        for b in range(8):
            if m >> b & 1:
                s ^= SYND[b + 8 * (ln - i + 1)]
    for i, m in crcflips:
        for b in range(8):
            if m >> b & 1:
                s ^= SYND[b + 8 * (1 - i)]
    return s


# ------------------------------------------------------------------------------------ transmissions
def seal(body_p):
    """head + body (parity already applied) + CRC + DEL: acars_frame's last lines for a body of any shape"""
    crc = S.crc_ccitt(body_p)
    return bytes(S.odd_parity(b) for b in (ord("+"), ord("*"), S.SYN, S.SYN, S.SOH)) + bytes(body_p) + bytes([crc & 0xFF, crc >> 8, S.DEL])


def clean_frame(rng, ln, etb=None):
    """a transmission whose block (mode .. terminator) has `ln` bytes: the 12 head bytes of a synth.message_zoo transmission
    (uplink / downlink, dotted addresses, NAK, DEL in the label), STX, random text, ETX or ETB.  ln < 13: the head cut short."""
    z = S.message_zoo(rng, 1)[0]
    head = z[5:17]
    if etb is None:
        etb = bool(rng.integers(0, 4) == 0)
    term = bytes([ETBP if etb else ETXP])
    if ln < 13:
        return seal(head[: ln - 1] + term)
    if ln == 13:
        return seal(head + term)
    text = S.random_text(rng, ln - 14, ln - 14) if ln > 14 else b""
    return seal(head + bytes(S.odd_parity(b) for b in bytes([S.STX]) + text) + term)


def block_of(frame):
    """(len, text, crc0, crc1) of an undamaged-shape transmission: what decodeAcars queues if the terminator is where it was put"""
    return len(frame) - 8, bytes(frame[5:-3]), frame[-3], frame[-2]


def framing_expect(frame):
    """putbit() + decodeAcars() (msk.c:53-63, acars.c:246-375) over the transmission's bits, polarity switch included: the blocks
    put on the queue [(len, text, crc0, crc1, via)] and whether the machine is back to searching when the transmission is over"""
    st = St()
    bits = S.frame_bits(frame, tail=TAIL)
    for i in range(len(bits)):
        b = int(bits[i]) ^ (st.S >> 1 & 1)
        st.outbits = ((st.outbits >> 1) & 0x7F) | (0x80 if b else 0)
        st.nbits -= 1
        if st.nbits <= 0:
            decode_acars(st, i)
    return [(b[1], b[5], b[3], b[4], b[6]) for b in st.blocks], st.astate == WSYN and st.S == 0


def apply_damage(frame, flips, crcflips=()):
    f = bytearray(frame)
    for i, m in flips:
        f[5 + i] ^= m
    for i, m in crcflips:
        f[len(f) - 3 + i] ^= m
    return bytes(f)


SPECIAL = (ETXP, ETBP, DELP)


def damage_is_plain(frame, flips):
    """positioned damage must not create or destroy ETX / ETB / DEL inside the text (it would move the block's end); a damaged
    terminator of an 18 .. 238-byte block is let through: DEL closes that block with the same length and CRC bytes (make_item
    checks with the framing machine that it does: the CRC bytes, read as text on the way, must not end the block either)"""
    ln = len(frame) - 8
    for i, m in flips:
        old, new = frame[5 + i], frame[5 + i] ^ m
        if i == ln - 1:
            if not 18 <= ln <= 238 or new in SPECIAL:
                return False
        elif old in SPECIAL or new in SPECIAL:
            return False
    return True


class Item:
    """one transmission: `frame` as sent (damaged), `clean` as composed, `tag` what the generator meant it to be, `want_raw` the
    block the framing machine queues from it (None: nothing), `direct` whether want_raw is the crafted block itself"""
    __slots__ = ("frame", "clean", "tag", "want_raw", "direct", "chn", "slot", "attempt")

    def __init__(self, frame, clean, tag, want_raw, direct):
        self.frame, self.clean, self.tag, self.want_raw, self.direct = frame, clean, tag, want_raw, direct
        self.chn = self.slot = self.attempt = -1


def make_item(rng, ln, tag, flips=(), crcflips=(), etb=None):
    """a transmission of block length ln with the given damage, content re-drawn until the damage is plain (see damage_is_plain)
    and the framing machine queues exactly the crafted block"""
    for _ in range(200):
        clean = clean_frame(rng, ln, etb)
        if not damage_is_plain(clean, flips):
            continue
        fr = apply_damage(clean, flips, crcflips)
        got, settled = framing_expect(fr)
        l0, t0, c0, c1 = block_of(fr)
        if settled and len(got) == 1 and got[0][:4] == (l0, t0, c0, c1):
            return Item(fr, clean, tag, got[0][:4], True)
    raise AssertionError("no plain transmission for %s len %d %r" % (tag, ln, flips))


def make_framing_item(rng, ln, tag, flips=(), crcflips=(), etb=None):
    """damage that moves or removes the block's end ON PURPOSE: what is queued is whatever the framing machine says"""
    for _ in range(200):
        clean = clean_frame(rng, ln, etb)
        fr = apply_damage(clean, flips, crcflips)
        got, settled = framing_expect(fr)
        if settled and len(got) <= 1:
            return Item(fr, clean, tag, got[0][:4] if got else None, False)
    raise AssertionError("framing never settles for %s len %d" % (tag, ln))


def one_bit_flips(rng, ln, idxs):
    return [(i, 1 << int(rng.integers(0, 8)) if i != 12 else (0x01, 0x80)[int(rng.integers(0, 2))]) for i in idxs]


def two_bits(rng):
    a, b = rng.choice(8, size=2, replace=False)
    return (1 << int(a)) | (1 << int(b))


def placements(ln, n):
    """index sets for n = 2 / 3 flagged bytes: (a) all in slot 0, (b) one per slot, (c) same lane in different slots,
    (d) adjacent across a slot boundary, (e) first and last byte"""
    out = {}
    out["a"] = [3, 40, 61][:n] if ln > 62 else [1, 5, 9][:n]
    if ln > 64 * (n - 1) + 7:
        out["b"] = [5 + 64 * s + 2 * s for s in range(n)]
    if ln > 64 * (n - 1) + 21:
        out["c"] = [21 + 64 * s for s in range(n)]
    for lo in (63, 127, 191):
        if ln > lo + 2:
            out["d%d" % lo] = [lo, lo + 1] + ([lo - 30] if n == 3 else [])
    if 18 <= ln <= 238:
        out["e"] = [0, ln - 1] + ([ln // 2] if n == 3 else [])
    return {k: sorted(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------ mining (syndrome arithmetic only)
def mine_prerr(rng, want_multi=30, want_wrong=10, want_groups=10):
    """two and three parity errors whose search has more than one acceptable candidate.  Kept until `want_multi` such blocks are
    held, `want_wrong` of them with a first candidate that is not the injected damage and `want_groups` with the first two
    candidates in different 64-candidate groups of the device's walk."""
    kept, multi, wrong, groups, trials = [], 0, 0, 0, 0
    while multi < want_multi or wrong < want_wrong or groups < want_groups:
        trials += 1
        pn = 2 + int(rng.integers(0, 4) > 0)
        ln = int(rng.integers(20, 242))
        idxs = sorted(int(i) for i in rng.choice([i for i in range(ln - 1) if i != 12], size=pn, replace=False))
        bits = [int(rng.integers(0, 8)) for _ in idxs]
        cands = prerr_candidates(ln, damage_syndrome(ln, [(i, 1 << b) for i, b in zip(idxs, bits)]), idxs)
        injected = sum(b << (3 * (pn - 1 - d)) for d, b in enumerate(bits))
        assert injected in cands
        if len(cands) < 2:
            continue
        w, g = cands[0] != injected, cands[0] >> 6 != cands[1] >> 6
        if multi >= want_multi and not (w and wrong < want_wrong) and not (g and groups < want_groups):
            continue
        multi, wrong, groups = multi + 1, wrong + w, groups + g
        kept.append((ln, [(i, 1 << b) for i, b in zip(idxs, bits)]))
    return kept, trials


def mine_dberr(rng, want_multi=30, want_wrong=10, want_groups=10):
    """two wrong bits in one byte of a long block, with more than one acceptable candidate (same three counts; groups = 64-byte
    groups of k)"""
    kept, multi, wrong, groups, trials, long241 = [], 0, 0, 0, 0, 0
    while multi < want_multi or wrong < want_wrong or groups < want_groups:
        trials += 1
        ln = int(rng.integers(100, 242))
        k = int(rng.choice([i for i in range(ln - 1) if i != 12]))
        m = two_bits(rng)
        cands = dberr_candidates(ln, damage_syndrome(ln, [(k, m)]))
        injected = (k,) + tuple(b for b in range(8) if m >> b & 1)
        assert injected in cands
        if len(cands) < 2 or (ln == 241 and long241 >= 3):             # (every such 241-byte block reads row 242: only a few)
            continue
        w = cands[0] != injected
        g = cands[0][0] >= 0 and cands[0][0] >> 6 != cands[1][0] >> 6
        if multi >= want_multi and not (w and wrong < want_wrong) and not (g and groups < want_groups):
            continue
        multi, wrong, groups, long241 = multi + 1, wrong + w, groups + g, long241 + (ln == 241)
        kept.append((ln, [(k, m)]))
    return kept, trials


def same_group_table():
    """Competing candidates INSIDE one 64-candidate group of the device's walk.  Two acceptable candidates differ by a code word
    (all of even weight: the polynomial has the factor x + 1) that lies inside the flagged bytes and the CRC bytes.  With text
    bytes alone that takes two bits in each of two bytes, which the code only has at byte distances 142, 144 and 208 -- never
    inside a 64-byte group of fixdberr, and only for flagged bytes that far apart in fixprerr.  With a wrong CRC bit it takes
    two bits of ONE flagged byte and two CRC bits: entries (row, bit, bit', crc bit, crc bit') for a byte in syndrome row
    len - i + 1 = row.  A block with bit (or bit') of that byte and crc bit (crc bit') wrong has both bits of the byte as
    acceptable candidates, next to each other in the search when the byte is the last flagged one."""
    pairs = {}
    for x in range(16):
        for y in range(x + 1, 16):
            pairs.setdefault(SYND[x] ^ SYND[y], []).append((x, y))
    return [(r, a, b, x, y) for r in range(2, 243) for a in range(8) for b in range(a + 1, 8)
            for x, y in pairs.get(SYND[a + 8 * r] ^ SYND[b + 8 * r], [])]


def mine_same_group(rng):
    """two blocks per entry of same_group_table (the injected bit first in the search, and second), with 0 .. 2 more flagged
    bytes in front of the byte in question: (len, flips, crcflips)"""
    out = []
    for n, (r, a, b, x, y) in enumerate(same_group_table()):
        for swap in (0, 1):
            lo, hi = (18, 238) if r == 2 else (max(20, r - 1), 241)      # (row 2 is the terminator: a block that DEL ends)
            bit, cbit = (b, y) if swap else (a, x)
            crcflips = [(1 - (cbit >> 3), 1 << (cbit & 7))]
            while True:                                                  # (re-drawn when another flagged byte brings a candidate of its own)
                ln = int(rng.integers(lo, hi + 1))
                idx = ln + 1 - r
                if idx == 12 or not 0 <= idx <= ln - 1:
                    continue
                extra = [] if idx < 20 else sorted(int(i) for i in rng.choice([i for i in range(idx) if i != 12], size=(n + swap) % 3, replace=False))
                flips = [(i, 1 << int(rng.integers(0, 8))) for i in extra] + [(idx, 1 << bit)]
                cands = prerr_candidates(ln, damage_syndrome(ln, flips, crcflips), [i for i, _ in flips])
                assert len(cands) >= 2, (r, a, b, x, y)
                if len(cands) == 2 and cands[0] >> 6 == cands[1] >> 6:
                    break
            out.append((ln, flips, crcflips))
    return out


def draw_unrepairable(rng, kind, ln):
    """damage that leaves the parity of the block intact or pairs up, and that no single candidate explains"""
    body = [i for i in range(ln - 1) if i != 12]
    if kind == "2x2":                                                  # two bytes with two wrong bits each
        a, b = (int(i) for i in rng.choice(body, size=2, replace=False))
        return [(a, two_bits(rng)), (b, two_bits(rng))], []
    if kind == "3+1":                                                  # three bits in a byte and one in another: two parity errors
        a, b = (int(i) for i in rng.choice(body, size=2, replace=False))
        three = 0
        for x in rng.choice(8, size=3, replace=False):
            three |= 1 << int(x)
        return [(a, three), (b, 1 << int(rng.integers(0, 8)))], []
    return [], [(int(rng.integers(0, 2)), two_bits(rng))]              # "crc2": a CRC byte with two wrong bits


def mine_false_accepts(rng, want=12):
    """unrepairable damage that the searches accept all the same, through a candidate that was never sent"""
    kept, trials = [], 0
    per = {"2x2": 0, "3+1": 0, "crc2": 0}
    while len(kept) < want:
        trials += 1
        kind = ("2x2", "3+1", "crc2")[trials % 3]
        if per[kind] >= (want + 2) // 3:
            continue
        ln = int(rng.integers(60, 241))
        flips, crcflips = draw_unrepairable(rng, kind, ln)
        crc = damage_syndrome(ln, flips, crcflips)
        if kind == "3+1":
            ok = bool(prerr_candidates(ln, crc, sorted(i for i, _ in flips)))
        else:
            ok = bool(dberr_candidates(ln, crc))
        if ok:
            per[kind] += 1
            kept.append((kind, ln, flips, crcflips))
    return kept, trials


# ------------------------------------------------------------------------------------ the corpus
def build_items(seed=SEED):
    rng = np.random.default_rng(seed)
    items = []
    add = items.append
    rlen = lambda lo=15, hi=241: int(rng.integers(lo, hi + 1))
    # every length, clean
    for ln in range(13, 242):
        add(make_item(rng, ln, "clean"))
    # one parity error at every index of the longest block and of a 130-byte block, the bit cycling; byte 12: all eight bits
    for ln in (241, 130):
        last = ln - 1 if ln <= 238 else ln - 2
        for i in range(last + 1):
            for b in (range(8) if i == 12 else [(i + ln) % 8]):
                for bb in [b] + [(b + d) % 8 for d in range(1, 8)]:      # (a bit that would create a terminator: the next one)
                    try:
                        add(make_item(rng, ln, "p1@%d" % ln, [(i, 1 << bb)]))
                        break
                    except AssertionError:
                        if i == 12:
                            raise
    for ln in (15, 64, 200):                                            # byte 12 once more at other lengths (STX there)
        for b in range(8):
            add(make_item(rng, ln, "p1@12", [(12, 1 << b)]))
    # byte 12 holding ETX (13-byte block): any damage loses the terminator, nothing may be queued; STX turned into ETX
    for b in range(8):
        add(make_framing_item(rng, 13, "etx12", [(12, 1 << b)], etb=False))
    for ln in (40, 150):
        add(make_framing_item(rng, ln, "stx>etx", [(12, 0x81)]))
    # two and three parity errors by placement, at the edge lengths and at random ones
    for n in (2, 3):
        for ln in EDGE_LENS + tuple(rlen(70) for _ in range(6)):
            for name, idxs in placements(ln, n).items():
                if all(i < ln for i in idxs) and len(set(idxs)) == n:
                    add(make_item(rng, ln, "p%d%s" % (n, name[0]), one_bit_flips(rng, ln, idxs)))
    for n in (1, 2, 3):
        for _ in range(30):
            ln = rlen()
            idxs = sorted(int(i) for i in rng.choice(ln - 1, size=n, replace=False))
            add(make_item(rng, ln, "p%d" % n, one_bit_flips(rng, ln, idxs)))
    # four parity errors (dropped by the block thread), five (the framing resets: never queued)
    for ln in EDGE_LENS[2:] + tuple(rlen(30) for _ in range(6)):
        idxs = sorted(int(i) for i in rng.choice([i for i in range(ln - 1) if i != 12], size=5, replace=False))
        add(make_item(rng, ln, "p4", one_bit_flips(rng, ln, idxs[:4])))
        add(make_framing_item(rng, ln, "p5", one_bit_flips(rng, ln, idxs)))
    # two bits in one byte: every index of a 240-byte block; every 16th and the slot boundaries of the 241-byte block; boundaries elsewhere
    for i in range(239):
        m = 0x84 if i == 12 else two_bits(rng)                          # (byte 12: bits 0 and 7 together would make it ETX)
        for _ in range(8):
            try:
                add(make_item(rng, 240, "db@240", [(i, m)]))
                break
            except AssertionError:
                m = two_bits(rng)
    for i in sorted(set(range(0, 240, 16)) | {63, 127, 128, 191, 239}):
        add(make_item(rng, 241, "db@241", [(i, two_bits(rng))]))
    for ln in EDGE_LENS[:-1] + tuple(rlen(70) for _ in range(8)):
        for i in (0, 11, 12, 13, 63, 64, 127, 128, 191, 192, ln - 2, ln - 1):
            if 0 <= i < ln and (i < ln - 1 or 18 <= ln <= 238):
                m = 0x84 if i == 12 else two_bits(rng)
                while i == ln - 1 and m == ETXP ^ ETBP:                  # (would turn one terminator into the other)
                    m = two_bits(rng)
                add(make_item(rng, ln, "db", [(i, m)]))
    # the CRC bytes: each of the 16 bits alone; with one and with two parity errors
    for c in range(2):
        for b in range(8):
            add(make_item(rng, rlen(), "crc", (), [(c, 1 << b)]))
            ln = rlen(80)
            idxs = sorted(int(i) for i in rng.choice([i for i in range(ln - 1) if i != 12], size=2, replace=False))
            add(make_item(rng, ln, "p1crc", one_bit_flips(rng, ln, idxs[:1]), [(c, 1 << b)]))
            add(make_item(rng, ln, "p2crc", one_bit_flips(rng, ln, idxs), [(1 - c, 1 << b)]))
    # unrepairable with the parity intact: the searches run to their end, or to a false hit
    for kind in ("2x2", "3+1", "crc2"):
        for ln in EDGE_LENS[2:] + tuple(rlen(30) for _ in range(10)):
            flips, crcflips = draw_unrepairable(rng, kind, ln)
            add(make_item(rng, ln, kind, flips, crcflips))
    mined = {}
    kept, mined["false_accept_trials"] = mine_false_accepts(rng)
    for kind, ln, flips, crcflips in kept:
        add(make_item(rng, ln, kind + "!", flips, crcflips))
    # order-sensitive blocks
    kept, mined["prerr_trials"] = mine_prerr(rng)
    for ln, flips in kept:
        add(make_item(rng, ln, "order-pr", flips))
    kept, mined["dberr_trials"] = mine_dberr(rng)
    for ln, flips in kept:
        add(make_item(rng, ln, "order-db", flips))
    for ln, flips, crcflips in mine_same_group(rng):
        add(make_item(rng, ln, "order-same", flips, crcflips))
    # too short for the block thread (acars.c:124); blocks that DEL ends (terminator lost); ETB blocks; long texts of every message shape
    for ln in range(2, 13):
        add(make_framing_item(rng, ln, "short"))
    for _ in range(16):
        ln = rlen(18, 238)
        add(make_item(rng, ln, "del-end", [(ln - 1, 1 << int(rng.integers(0, 8)))]))
    for _ in range(24):
        add(make_item(rng, rlen(), "etb", etb=True))
    for _ in range(60):
        add(make_item(rng, rlen(120), "zoo"))
    return items, mined


def reads_row_242(item):
    return item.want_raw is not None and 242 in model_blk(*item.want_raw)["rows"]


def slot_audio(item, attempt, seed=SEED):
    """(first sample, float32 envelope) of a transmission in its slot: it ends END_MARGIN .. END_MARGIN + 2000 samples before the
    slot does, at a carrier phase and an offset drawn from (seed, channel, slot, attempt)"""
    rng = np.random.default_rng([seed, item.chn, item.slot, attempt])
    a = S.msk_audio(S.frame_bits(item.frame, tail=TAIL), phase0=float(rng.uniform(0, 2 * np.pi)))
    end = (item.slot + 1) * PERIOD - END_MARGIN
    room = end - (item.slot * PERIOD + LEAD) - len(a)
    assert room >= 0, (len(a), item.tag)
    end -= int(rng.integers(0, min(room, 2000) + 1))
    return end - len(a), S.envelope(a)


CARRIER = S.envelope(np.zeros(1))[0]                                   # the un-modulated carrier between transmissions


def place(items, seed=SEED):
    """item.attempt for every item.  The reference's demodulator (msk.c:67-137) does not lock onto every noiseless transmission:
    for a few per cent of (carrier phase, offset) pairs its loop settles between two decision axes and slips after some
    hundred bits, so the block never arrives -- nothing to do with the repair.  A corpus whose every block must reach the repair
    cannot leave that to luck: channel by channel, slot by slot, the phase / offset draw is repeated (attempt 0, 1, ...) until the
    oracle's demodulator, continuing from the state the channel is in, queues what the framing machine says this transmission
    queues, and is back to searching at the end of the slot."""
    import ctypes as C
    from oracle import oracle as O
    tries = 0
    for c, its in by_channel(items).items():
        ch = O.Channel(c, max_frames=64)
        at = {it.slot: it for it in its}
        for slot in range(SLOTS):
            it = at.get(slot)
            if it is None:
                ch.demod(np.full(PERIOD, CARRIER, dtype=np.float32))
                continue
            snap = O.OrcChan.from_buffer_copy(ch.c)
            for attempt in range(64):
                seg = np.full(PERIOD, CARRIER, dtype=np.float32)
                start, a = slot_audio(it, attempt, seed)
                seg[start - slot * PERIOD: start - slot * PERIOD + len(a)] = a
                n0 = int(snap.frames_n)
                ch.demod(seg)
                new = [raw_tuple(f) for f in ch.frames[n0:]]
                tries += 1
                if new == ([it.want_raw] if it.want_raw is not None else []) and ch.c.Acarsstate == 0:
                    it.attempt = attempt
                    break
                C.memmove(C.byref(ch.c), C.byref(snap), C.sizeof(snap))
            else:
                raise AssertionError("no placement for %s on channel %d slot %d" % (it.tag, c, slot))
    return tries


@functools.lru_cache(maxsize=2)
def corpus(seed=SEED):
    """(items, mined): the items placed on NCH channels x SLOTS slots (item.chn, item.slot, item.attempt), slot j of every
    channel ending inside the same call of CALL samples so that one repair pass sees hundreds of blocks.  The blocks whose search
    reads syndrome row 242 sit in the last slot of their channels: leaving them out (the leg against the real blk_thread does)
    changes nothing for any other transmission."""
    items, mined = build_items(seed)
    assert len(items) <= NCH * SLOTS, len(items)
    order = [int(o) for o in np.random.default_rng(seed + 1).permutation(NCH * SLOTS)]
    last = [o for o in order if o % SLOTS == SLOTS - 1]
    flagged = [it for it in items if reads_row_242(it)]
    for it, o in zip(flagged, last):
        it.chn, it.slot = o // SLOTS, o % SLOTS
    taken = set(last[: len(flagged)])
    rest = [o for o in order if o not in taken]
    for it, o in zip([it for it in items if it.chn < 0], rest):
        it.chn, it.slot = o // SLOTS, o % SLOTS
    mined["placement_tries"] = place(items, seed)
    return items, mined


def by_channel(items):
    out = {}
    for it in sorted(items, key=lambda it: (it.chn, it.slot)):
        out.setdefault(it.chn, []).append(it)
    return out


def audio(items, channels=None, seed=SEED):
    """float32 [len(channels), NSAMP]: the envelopes of the given channels (default all), without noise"""
    channels = list(range(NCH)) if channels is None else list(channels)
    row = {c: r for r, c in enumerate(channels)}
    x = np.full((len(channels), NSAMP), CARRIER, dtype=np.float32)
    for it in items:
        if it.chn in row:
            start, a = slot_audio(it, it.attempt, seed)
            x[row[it.chn], start:start + len(a)] = a
    return x


def raw_tuple(f):
    """(len, text, crc0, crc1) of an oracle / device / reference block"""
    return (int(f.len), bytes(f.txt[: max(0, f.len)]), int(f.crc[0]), int(f.crc[1]))


# ------------------------------------------------------------------------------------ categories, from what was queued and delivered
def categorize(item, raw, out):
    """names of the categories a block belongs to, from the block that was QUEUED (`raw`: (len, text, crc0, crc1) or None), the
    clean transmission it came from and what the repair DELIVERED (`out`: (err, text) or None) -- not from the generator's tag,
    except where nothing was queued at all"""
    cats = set()
    if raw is None:
        cats.add("nothing-queued:" + item.tag)
        return cats
    ln, txt, c0, c1 = raw
    cl, ctxt, cc0, cc1 = block_of(item.clean)
    if ln < 13:
        cats.add("short")
        return cats
    if ln != cl:
        cats.add("end-moved")
        return cats
    diff = [(i, txt[i] ^ ctxt[i]) for i in range(ln) if txt[i] != ctxt[i]]
    cdiff = [(i, m) for i, m in ((0, c0 ^ cc0), (1, c1 ^ cc1)) if m]
    forced = bytearray(txt)
    forced[12] = (forced[12] & 0x83) | 0x02
    pr = [i for i in range(ln) if popc(forced[i]) & 1 == 0]
    pn = len(pr)
    kept = out is not None
    same = kept and out[1] == bytes(b & 0x7F for b in ctxt[:12]) + bytes([(ctxt[12] & 0x03) | 0x02]) + bytes(b & 0x7F for b in ctxt[13:])
    if txt[ln - 1] == ETBP or ctxt[ln - 1] == ETBP:
        cats.add("etb")
    if txt[ln - 1] not in (ETXP, ETBP):
        cats.add("ended-by-del")
    if not diff and not cdiff:
        cats.add("clean")
        if kept and same and out[0] == 0:
            cats.add("clean-delivered:%d" % ln)
        return cats
    onebit = all(popc(m) == 1 for _, m in diff)
    if diff and onebit and not cdiff:
        if any(i == 12 and m & 0x7E for i, m in diff) and len(diff) == 1:
            cats.add("byte12-vanishes")
            if kept and same and out[0] == 0:
                cats.add("byte12-vanishes-delivered")
        if pn == 1 and len(diff) == 1:
            cats.add("p1")
            if kept and same:
                cats.add("p1@%d:%d" % (ln, pr[0]))
                cats.add("p1-bit:%d" % (diff[0][1].bit_length() - 1))
            if pr[0] == 12:
                cats.add("p1-byte12")
        if pn in (2, 3) and len(diff) == pn:
            if all(p < 64 for p in pr):
                cats.add("p%d-slot0" % pn)
            if len(set(p >> 6 for p in pr)) == pn:
                cats.add("p%d-one-per-slot" % pn)
            if any(a != b and (a - b) % 64 == 0 for a in pr for b in pr):
                cats.add("p%d-same-lane" % pn)
            if any(b - a == 1 and b % 64 == 0 for a in pr for b in pr):
                cats.add("p%d-across-boundary" % pn)
            if pr[0] == 0 and pr[-1] == ln - 1:
                cats.add("p%d-first-and-last" % pn)
            if kept and same:
                cats.add("p%d-repaired" % pn)
        if pn == 4 and not kept:
            cats.add("p4-dropped")
    if len(diff) == 1 and popc(diff[0][1]) == 2 and not cdiff and pn == 0:
        cats.add("db")
        if kept:
            cats.add("db-delivered")
            if ln in (240, 241):
                cats.add("db@%d:%d" % (ln, diff[0][0]))
            if diff[0][0] in (63, 64, 127, 128, 191, 192) and ln < 240:
                cats.add("db-boundary")
    if not diff and len(cdiff) == 1 and popc(cdiff[0][1]) == 1 and kept and same:
        cats.add("crc-bit:%d" % (8 * cdiff[0][0] + cdiff[0][1].bit_length() - 1))
    if diff and onebit and len(cdiff) == 1 and popc(cdiff[0][1]) == 1 and pn == len(diff) and pn in (1, 2):
        cats.add("p%d+crc-bit" % pn)
        if kept and same:
            cats.add("p%d+crc-bit-repaired" % pn)
    unrep = None
    if len(diff) == 2 and all(popc(m) == 2 for _, m in diff) and not cdiff and pn == 0:
        unrep = "2x2"
    if len(diff) == 2 and sorted(popc(m) for _, m in diff) == [1, 3] and not cdiff and pn == 2:
        unrep = "3+1"
    if not diff and len(cdiff) == 1 and popc(cdiff[0][1]) == 2:
        unrep = "crc2"
    if unrep:
        cats.add("unrepairable-" + unrep)
        cats.add("unrepairable-accepted" if kept else "unrepairable-dropped")
    if kept and not same:
        cats.add("delivered-other-text")
    return cats


def order_facts(raw, model):
    """for a block that reaches a search: (which search, number of acceptable candidates, first two in different 64-groups,
    first two in the same 64-group)"""
    ln = raw[0]
    if model["crc"] is None:
        return None
    if model["err"]:
        c = prerr_candidates(ln, model["crc"], model["pr"])
        return ("pr", len(c), len(c) > 1 and c[0] >> 6 != c[1] >> 6, len(c) > 1 and c[0] >> 6 == c[1] >> 6)
    if model["crc"]:
        c = dberr_candidates(ln, model["crc"])
        return ("db", len(c), len(c) > 1 and c[0][0] >= 0 and c[0][0] >> 6 != c[1][0] >> 6,
                len(c) > 1 and c[0][0] >= 0 and c[0][0] >> 6 == c[1][0] >> 6)
    return None


if __name__ == "__main__":
    import collections
    items, mined = corpus()
    print(len(items), "transmissions;", mined)
    print(sorted(collections.Counter(it.tag for it in items).items()))
