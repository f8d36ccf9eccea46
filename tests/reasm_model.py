"""Reassembly of multi-block messages, restated for tests: the specification of acarsdec_amd/csrc/reasm.hip and its oracle, as
tests/rate_ref.py is for the rational grid.  A plain dict walk.

It follows libacars' documented behaviour from the reference's call site outward (output.c:33-101, 528-531, 552-559, 579-626 in the
HAVE_LIBACARS build: the key (addr, label, msn), the sequence numbers, the wrap, "ETB means more fragments", rx_time = blk->tv, the
time-outs VGT4 = 660 s and VAT4 = 90 s, squitters and bs == ETX skipped, a completed payload replaces the text) and HAS NOT BEEN RUN
AGAINST libacars: libacars is not part of this project's toolchain.  The H1 sublabel / MFI prefix that libacars strips per fragment
is not stripped: the fragment data is acg_msg.txt.

A message is anything with the attributes of acg_msg that the rule reads: mode, addr, label, bid, no, bs, be, txt, txt_len,
soh_sample (and chn, end_bit, end_sample for the completed record).  Strings are bytes; single characters are ints or 1-byte
strings (ctypes hands out the latter)."""

UNKNOWN, COMPLETE, IN_PROGRESS, SKIPPED, DUPLICATE, OUT_OF_SEQUENCE, ARGS_INVALID, OVERFLOW = range(8)
NAMES = ("unknown", "complete", "in progress", "skipped", "duplicate", "out of sequence", "invalid args", "overflow")
VGT4_US, VAT4_US = 660 * 10**6, 90 * 10**6
ETX, ETB = 0x03, 0x17
SAMPLE_US = 80                                        # a 12.5 kHz sample
RECLAIM_US = 2 * 10**6                                # the device takes over a slot whose entry expired more than this before G
DEFAULT_MAX_TEXT = 3584


def _c(v):
    """a char field as an unsigned int"""
    if isinstance(v, (bytes, bytearray)):
        return v[0] if v else 0
    return int(v) & 0xff


def _sc(v):
    """... as C's signed char"""
    v = _c(v)
    return v - 256 if v >= 128 else v


def raw(m, name, n):
    """the n bytes of a char-array field, NULs and what lies behind them included (ctypes hands out C strings otherwise)"""
    import ctypes
    if isinstance(m, ctypes.Structure):
        return ctypes.string_at(ctypes.addressof(m) + getattr(type(m), name).offset, n)
    return bytes(getattr(m, name))[:n].ljust(n, b"\0")


def cstr(b, n=None):
    """a char array as a C string: up to the first NUL (ctypes' .value does the same; raw bytes are cut here)"""
    b = bytes(b)[:n]
    return b.split(b"\0", 1)[0]


class Entry:
    __slots__ = ("prev", "first_us", "timeout_us", "text", "nfrag", "first_soh_sample")


class Completed:
    """what acg_drain_reassembled hands out for one message"""
    __slots__ = ("chn", "nfrag", "end_bit", "end_sample", "soh_sample", "first_soh_sample", "down", "addr", "label", "msn", "text")

    def astuple(self):
        return tuple(getattr(self, k) for k in self.__slots__)


def key_of(m):
    down = 0x30 <= _c(m.bid) <= 0x39
    return (cstr(raw(m, "addr", 7)), cstr(raw(m, "label", 2)), cstr(raw(m, "no", 3)) if down else b"")


def msg_text(m):
    n = max(0, min(int(m.txt_len), 242))
    return raw(m, "txt", n)


class Table:
    """table = Table(t0_us, max_text); status = table.add(m) for the messages past -A / -b in the order rule's order; the completed
    messages collect in table.done.  reclaim=True: the device's slot rule as well -- at the start of a call (begin_call) every entry
    that expired more than RECLAIM_US before G, the largest tv of the EARLIER calls, is thrown away, as if another key had taken
    its slot over."""

    def __init__(self, t0_us=0, max_text=DEFAULT_MAX_TEXT, reclaim=False):
        self.t0_us, self.max_text, self.reclaim = t0_us, max_text, reclaim
        self.table, self.done = {}, []
        self.G, self.Gnext = None, None

    def begin_call(self):
        if self.Gnext is not None and (self.G is None or self.Gnext > self.G):
            self.G = self.Gnext
        if self.reclaim and self.G is not None:
            for k in [k for k, e in self.table.items() if self.G > e.first_us + e.timeout_us + RECLAIM_US]:
                del self.table[k]

    def live(self):
        return len(self.table)

    def add(self, m):
        tv_us = self.t0_us + SAMPLE_US * int(m.soh_sample)
        if _c(m.bs) == ETX or _c(m.bid) == 0:
            return SKIPPED                                            # no table access
        self.Gnext = tv_us if self.Gnext is None else max(self.Gnext, tv_us)
        down = 0x30 <= _c(m.bid) <= 0x39
        key = key_of(m)
        seq = (_sc(raw(m, "no", 4)[3:4]) if down else _sc(m.bid)) - 65
        first = 0 if down else None
        wrap = None if down else (26 if _c(m.mode) == 0x32 else 23)
        final = _c(m.be) != ETB
        text = msg_text(m)
        table = self.table
        e = table.get(key)
        if e is not None and tv_us > e.first_us + e.timeout_us:       # strict; the ENTRY's time-out
            del table[key]
            e = None
        if e is None:
            if first is not None and seq != first:
                return OUT_OF_SEQUENCE
            if final:
                return SKIPPED
            e = table[key] = Entry()
            e.prev, e.first_us, e.timeout_us, e.text, e.nfrag = None, tv_us, (VGT4_US if down else VAT4_US), b"", 0
            e.first_soh_sample = int(m.soh_sample)
        if wrap is not None and seq == 0 and e.prev is not None and e.prev + 1 == wrap:
            e.prev = -1
        if e.prev is not None and seq == e.prev:
            return DUPLICATE                                          # entry untouched
        if e.prev is not None and seq != e.prev + 1:
            del table[key]
            return OUT_OF_SEQUENCE
        if len(e.text) + len(text) > self.max_text:
            del table[key]
            return OVERFLOW
        e.text += text
        e.nfrag += 1
        e.prev = seq
        if final:
            del table[key]
            c = Completed()
            c.chn, c.nfrag, c.end_bit, c.end_sample, c.soh_sample = int(m.chn), e.nfrag, int(m.end_bit), int(m.end_sample), int(m.soh_sample)
            c.first_soh_sample, c.down, c.addr, c.label, c.msn, c.text = e.first_soh_sample, int(down), key[0], key[1], key[2], e.text
            self.done.append(c)
            return COMPLETE
        return IN_PROGRESS


def creates(m):
    """can this message begin an entry (given none)?  What a key's claim of a slot hangs on."""
    if _c(m.bs) == ETX or _c(m.bid) == 0 or _c(m.be) != ETB:
        return False
    down = 0x30 <= _c(m.bid) <= 0x39
    return (not down) or _sc(raw(m, "no", 4)[3:4]) - 65 == 0


def call_order(msgs):
    """the indices of one call's messages in the order rule's order: ascending (end_sample, chn)"""
    return sorted(range(len(msgs)), key=lambda i: (int(msgs[i].end_sample), int(msgs[i].chn)))


def run(msgs, batches, t0_us=0, max_text=DEFAULT_MAX_TEXT, reclaim=False, keep=None):
    """msgs cut into consecutive batches (their lengths) = calls: (statuses in input order, the completed messages in the order of
    their final fragments, the table's occupancy [live before the call + its new keys] per call).  keep(m) -> bool: -A / -b."""
    t = Table(t0_us, max_text, reclaim)
    status = [None] * len(msgs)
    load = []
    at = 0
    for n in batches:
        part = msgs[at:at + n]
        t.begin_call()
        before = set(t.table)
        newkeys = set()
        for i in call_order(part):
            m = part[i]
            if keep is not None and not keep(m):
                status[at + i] = SKIPPED
                continue
            if creates(m) and key_of(m) not in before:
                newkeys.add(key_of(m))
            status[at + i] = t.add(m)
        load.append(len(before) + len(newkeys))
        at += n
    assert at == len(msgs)
    return status, t.done, load
