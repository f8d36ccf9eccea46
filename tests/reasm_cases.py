"""Inputs for the reassembly tests (tests/test_reasm_model.py on the CPU, tests/test_gpu_reasm.py on the device): records as
acg_drain_msgs hands them out, built by hand or drawn at random, and the conditions the random traffic keeps."""
import ctypes as C
import random

from acarsdec_amd import _capi as K

import reasm_model as RM

STX, ETX, ETB = 0x02, 0x03, 0x17
BLOCK_SAMPLES = 10875                                 # a block lasts less than this (0.87 s): tv runs backwards by less in call order
FL_PROBE = 128


def msg(addr=b"N123AB", label=b"H1", bid=b"1", no=b"M01A", be=ETB, bs=STX, mode=b"2", txt=b"", end_sample=0, chn=0, back=3000, fid=b"XX0001",
        txt_len=None):
    """one record; a downlink when bid is a digit.  soh_sample = end_sample - back"""
    m = K.Msg()
    m.chn, m.err, m.lvl = chn, 0, -10.0
    m.txt_len = len(txt) if txt_len is None else txt_len
    m.end_bit, m.end_sample, m.soh_sample = end_sample // 5, end_sample, end_sample - back
    m.mode, m.addr, m.ack, m.label, m.bid, m.no = mode, addr, b"!", label, bid or b"\0", no
    down = b"0" <= bid <= b"9" if bid else False
    m.fid = fid if down else b""
    m.bs, m.be, m.down = bytes([bs]), bytes([be]), (b"\x01" if down else b"\x00")
    C.memmove(C.addressof(m) + K.Msg.no.offset, no, min(len(no), 4))      # (bytes behind a NUL too: a field assignment stops there)
    C.memmove(C.addressof(m) + K.Msg.txt.offset, txt, min(len(txt), 242))
    return m


def pack(msgs):
    arr = (K.Msg * max(len(msgs), 1))()
    for i, m in enumerate(msgs):
        C.memmove(C.addressof(arr) + i * C.sizeof(K.Msg), C.addressof(m), C.sizeof(K.Msg))
    return arr


def text_of(i, n):
    return bytes((0x20 + (i * 7 + k * 13) % 0x5f) for k in range(n))


def hand_chains():
    """(msgs, want): the hand-written chains, one after the other in time, and the statuses written down by hand"""
    R = RM
    out, want = [], []
    t = [100000]

    def add(st, **kw):
        t[0] += 4000
        kw.setdefault("end_sample", t[0])
        kw.setdefault("txt", text_of(len(out), 17 + len(out) % 9))
        out.append(msg(**kw))
        want.append(st)

    # a 3-block downlink A/B/C, the middle block repeated: DUPLICATE leaves the entry intact
    add(R.IN_PROGRESS, no=b"M01A")
    add(R.IN_PROGRESS, no=b"M01B", chn=2)
    add(R.DUPLICATE, no=b"M01B", chn=1)
    add(R.COMPLETE, no=b"M01C", be=ETX)
    # a lost block: OUT_OF_SEQUENCE with the entry gone; the chain's later blocks are OUT_OF_SEQUENCE too
    add(R.IN_PROGRESS, no=b"M02A")
    add(R.OUT_OF_SEQUENCE, no=b"M02C")
    add(R.OUT_OF_SEQUENCE, no=b"M02D")
    add(R.OUT_OF_SEQUENCE, no=b"M02E", be=ETX)
    # a lone final block
    add(R.SKIPPED, no=b"M03A", be=ETX)
    # uplinks: across the wrap in mode '2' (Y, Z, A), in another mode (V, W, A), and X after W without a wrap
    add(R.IN_PROGRESS, addr=b"UP2", bid=b"Y", no=b"", mode=b"2")
    add(R.IN_PROGRESS, addr=b"UP2", bid=b"Z", no=b"", mode=b"2")
    add(R.COMPLETE, addr=b"UP2", bid=b"A", no=b"", mode=b"2", be=ETX)
    add(R.IN_PROGRESS, addr=b"UPX", bid=b"V", no=b"", mode=b"X")
    add(R.IN_PROGRESS, addr=b"UPX", bid=b"W", no=b"", mode=b"X")
    add(R.IN_PROGRESS, addr=b"UPX", bid=b"A", no=b"", mode=b"X")
    add(R.COMPLETE, addr=b"UPX", bid=b"B", no=b"", mode=b"X", be=ETX)
    add(R.IN_PROGRESS, addr=b"UPW", bid=b"W", no=b"", mode=b"X")
    add(R.COMPLETE, addr=b"UPW", bid=b"X", no=b"", mode=b"X", be=ETX)
    add(R.IN_PROGRESS, addr=b"UPZ", bid=b"W", no=b"", mode=b"2")      # mode '2' does not wrap at W ...
    add(R.OUT_OF_SEQUENCE, addr=b"UPZ", bid=b"A", no=b"", mode=b"2")  # ... so A after W is out of sequence there
    # a short message number: no[3] == 0 is sequence -65
    add(R.OUT_OF_SEQUENCE, no=b"M04")
    # bs == ETX and a squitter
    add(R.SKIPPED, no=b"M05A", bs=ETX)
    add(R.SKIPPED, bid=b"", no=b"")
    # an empty fragment in a chain, and a one-byte one (the row's seam)
    add(R.IN_PROGRESS, no=b"M06A", txt=b"abcde")
    add(R.IN_PROGRESS, no=b"M06B", txt=b"")
    add(R.IN_PROGRESS, no=b"M06C", txt=b"f")
    add(R.IN_PROGRESS, no=b"M06D", txt=text_of(3, 242))
    add(R.COMPLETE, no=b"M06E", txt=b"xyz", be=ETX)
    return out, want


def overflow_chain(max_text):
    """fills a row to max_text exactly (COMPLETE), then a chain that reaches max_text + 1 (OVERFLOW, and the rest OUT_OF_SEQUENCE)"""
    out, want = [], []
    t = 500000
    for tag, extra in ((b"OV1", 0), (b"OV2", 1)):
        left, k = max_text + extra, 1
        t += 4000
        out.append(msg(no=tag + b"A", txt=b"", end_sample=t))         # (an empty first block: the chain is one whatever max_text is)
        want.append(RM.IN_PROGRESS)
        while left > 0:
            n = min(left, 242)
            left -= n
            t += 4000
            st = RM.IN_PROGRESS if left else (RM.OVERFLOW if extra else RM.COMPLETE)
            out.append(msg(no=tag + bytes([65 + k]), txt=text_of(k, n), be=ETB if left else ETX, end_sample=t))
            want.append(st)
            k += 1
        if extra:
            t += 4000
            out.append(msg(no=tag + bytes([65 + k]), txt=b"z", be=ETX, end_sample=t))
            want.append(RM.OUT_OF_SEQUENCE)
    return out, want


def timeout_chains():
    """(msgs, want) in time order: a fragment at first + 660 s exactly (8 250 000 samples) continues, one sample later restarts;
    the same at 90 s (1 125 000 samples) for an uplink; the time-out kept is the entry's, not the fragment's (a chain begun by an
    uplink keeps 90 s when a downlink of the same key joins)"""
    both = []
    s0 = 1000000

    def at(soh, st, **kw):
        both.append((msg(end_sample=soh + 3000, back=3000, txt=b"t%d" % len(both), **kw), st))

    at(s0, RM.IN_PROGRESS, addr=b"TD1", no=b"T01A")
    at(s0 + 8250000, RM.IN_PROGRESS, addr=b"TD1", no=b"T01B")
    at(s0 + 8250001, RM.OUT_OF_SEQUENCE, addr=b"TD1", no=b"T01C")     # the entry is gone: C is not a first fragment
    at(s0 + 8250002, RM.IN_PROGRESS, addr=b"TD1", no=b"T01A")         # ... and A restarts
    at(s0, RM.IN_PROGRESS, addr=b"TU1", bid=b"C", no=b"", chn=1)
    at(s0 + 1125000, RM.IN_PROGRESS, addr=b"TU1", bid=b"D", no=b"", chn=1)
    at(s0 + 1125001, RM.IN_PROGRESS, addr=b"TU1", bid=b"E", no=b"", chn=1)   # restarts: an uplink has no first
    at(s0 + 1125002, RM.COMPLETE, addr=b"TU1", bid=b"F", no=b"", chn=1, be=ETX)   # ... a chain of E, F
    # one key for an uplink and a downlink: addr, label and an empty msn.  The uplink begins the entry: it holds for 90 s
    at(s0, RM.IN_PROGRESS, addr=b"TX1", bid=b"@", no=b"", chn=2)      # '@' - 'A' = -1
    at(s0 + 1125001, RM.SKIPPED, addr=b"TX1", bid=b"1", no=b"\0\0\0A", be=ETX, chn=2)   # expired at 90 s: a lone final downlink
    at(s0 + 10, RM.IN_PROGRESS, addr=b"TX2", bid=b"@", no=b"", chn=3)
    at(s0 + 1125000, RM.COMPLETE, addr=b"TX2", bid=b"1", no=b"\0\0\0A", be=ETX, chn=3)    # within 90 s: sequence 0 follows -1
    both.sort(key=lambda p: (p[0].end_sample, p[0].chn))
    return [p[0] for p in both], [p[1] for p in both]


def one_field_keys():
    """keys that differ in exactly one character of addr, of label, of msn, and an uplink and a downlink of one aircraft and label,
    interleaved in ONE batch: a segment must be an exact-key segment"""
    keys = [dict(addr=b"N100AA", label=b"H1", no=b"K01"), dict(addr=b"N100AB", label=b"H1", no=b"K01"), dict(addr=b"M100AA", label=b"H1", no=b"K01"),
            dict(addr=b"N100AA", label=b"H2", no=b"K01"), dict(addr=b"N100AA", label=b"I1", no=b"K01"), dict(addr=b"N100AA", label=b"H1", no=b"K02"),
            dict(addr=b"N100AA", label=b"H1", no=b"L01"), dict(addr=b"N100AA", label=b"H1", no=b"K0"), dict(addr=b"N100AA", label=b"H", no=b"K01"),
            dict(addr=b"N100A", label=b"H1", no=b"K01")]
    out = []
    t = 200000
    for blk in range(4):
        for j, k in enumerate(keys):
            t += 900
            out.append(msg(addr=k["addr"], label=k["label"], no=k["no"].ljust(3, b"\0") + bytes([65 + blk]), txt=b"%d:%d;" % (j, blk) * (1 + j % 3),
                           be=ETX if blk == 3 else ETB, end_sample=t, chn=j % 3))
        t += 900
        out.append(msg(addr=b"N100AA", label=b"H1", bid=bytes([65 + blk]), no=b"", txt=b"up%d" % blk, be=ETX if blk == 3 else ETB, end_sample=t, chn=1))
    return out


def random_traffic(n=20000, nkeys=300, seed=1, pool=20, group=40, span=2500):
    """n records over nkeys keys: ETB chains of 2-16 blocks from at most `pool` keys at a time, with duplicates, losses, abandoned
    chains, single blocks, squitters, ties in end_sample and jumps in time that run chains into their time-outs.  New chains take
    their key from a group of `group` keys that moves on every `span` records, so that a call of at most 2000 records meets at most
    two groups (test_reasm_model.py proves the occupancy bound from the model)."""
    rng = random.Random(seed)
    keys = []
    for i in range(nkeys):
        up = i % 5 == 4
        keys.append(dict(addr=b"%c%05d" % (65 + i % 7, i // 3), label=(b"H1", b"5Z", b"80")[i % 3], up=up, msn=b"%c%02d" % (77 + i % 3, i % 100)))
    active = {}                                       # key index -> [next block, blocks, mode]
    out = []
    t = 50000
    used = set()                                      # channels that already ended a block at t: (end_sample, chn) is distinct

    def channel():
        nonlocal t, used
        free = [c for c in range(8) if c not in used]
        if not free:
            t, used, free = t + 1, set(), list(range(8))
        c = rng.choice(free)
        used.add(c)
        return c

    while len(out) < n:
        r = rng.random()
        dt = rng.choice((0, 0, 700, 2500, 4000, 9000)) if r > 0.002 else rng.choice((1200000, 8300000))
        if dt:
            t, used = t + dt, set()
        g0 = (len(out) // span * group) % nkeys
        if (len(active) < pool and rng.random() < 0.3) or not active:
            ki = (g0 + rng.randrange(group)) % nkeys
            if ki not in active:
                active[ki] = [0, rng.randint(2, 16), rng.choice((b"2", b"X"))]
        ki = rng.choice(sorted(active))
        k = keys[ki]
        st = active[ki]
        r = rng.random()
        if r < 0.03:                                                  # a single block or a squitter of that aircraft
            out.append(msg(addr=k["addr"], label=b"Q0", bid=b"" if r < 0.01 else b"3", no=b"" if r < 0.01 else b"S99A", be=ETX, txt=text_of(len(out), rng.randint(0, 40)),
                           end_sample=t, chn=channel(), back=rng.randint(500, BLOCK_SAMPLES - 1)))
            continue
        blk = st[0]
        if r < 0.08 and blk > 0:
            blk -= 1                                                  # retransmission of the last block
        elif r < 0.11:
            st[0] += 1                                                # a lost block
            blk = st[0]
        last = blk >= st[1] - 1
        ln = rng.choice((0, 1, 2, 3, 5, 17, 100, 219, 220, 238))
        if k["up"]:
            first = 20 if st[2] == b"X" else 22                       # crosses the wrap of its mode
            wrap = 23 if st[2] == b"X" else 26
            bid, no = bytes([65 + (first + blk) % wrap]), b""
        else:
            bid, no = b"%d" % (ki % 10), k["msn"] + bytes([65 + blk])
        out.append(msg(addr=k["addr"], label=k["label"], bid=bid, no=no, mode=st[2], be=ETX if last else ETB, txt=text_of(len(out), ln), end_sample=t,
                       chn=channel(), back=rng.randint(500, BLOCK_SAMPLES - 1)))
        if blk == st[0]:
            st[0] += 1
        if last or rng.random() < 0.01:                               # done, or abandoned
            del active[ki]
    return out[:n]


def random_batches(n, seed, lo=1, hi=2000):
    rng = random.Random(seed)
    out = []
    while n:
        b = min(n, rng.choice((lo, rng.randint(lo, 50), rng.randint(lo, hi), hi)))
        out.append(b)
        n -= b
    return out


def shuffled_within(msgs, batches, seed):
    """the same calls with each call's records in a random order (the order rule is the device's to apply)"""
    rng = random.Random(seed)
    out, at = [], 0
    for b in batches:
        part = list(msgs[at:at + b])
        rng.shuffle(part)
        out += part
        at += b
    return out


def completed_tuples(done):
    return [c.astuple() for c in done]
