"""A Python model of the flight table: addFlight() and routejson() (output.c:361-456) restated as the reference runs them -- a
move-to-front list, and after every message a walk over the whole list that deletes what is older than mdly -- plus, apart
from it, the lazy rule the device uses (acarsdec_amd/csrc/flight.hip).  The CPU tests check the list walk against the
reference program's monitor frames and route lines (tests/golden/flights_golden.json) and the lazy rule against the list walk;
the GPU tests check the device against the list walk.

An event is a message that reaches addFlight(): it passed -A / -b and is a downlink with bs != 0x03 (output.c:545-567,647).
-e is tested after addFlight(); routejson() runs only for a message that passed it too."""
import struct

import label_model as LM

FIELDS = LM.FIELDS                                                    # da sa eta gout gin woff won


def cstr(b, n):
    """strncpy(dst, b, n) of a C string: cut at the first NUL, NUL padded"""
    b = bytes(b).split(b"\0")[0][:n]
    return b + b"\0" * (n - len(b))


def tv(t0_sec, t0_usec, soh_sample):
    """t0 + soh_sample / 12500 s: a sample is exactly 80 us"""
    us = t0_usec + soh_sample * 80
    return t0_sec + us // 1000000, us % 1000000


class Event:
    __slots__ = ("addr", "fid", "chn", "soh", "end", "sec", "usec", "fields", "e_ok")

    def __init__(self, addr, fid, chn, soh, end, sec, usec, fields, e_ok):
        self.addr, self.fid, self.chn, self.soh, self.end = cstr(addr, 8), cstr(fid, 7), int(chn), int(soh), int(end)
        self.sec, self.usec, self.fields, self.e_ok = int(sec), int(usec), fields, bool(e_ok)


def event_of(m, t0=(0, 0), downlink_only=False, skip_empty=False, labels=()):
    """The event of a split record (a K.Msg, or anything with its fields), or None when the record never reaches addFlight()."""
    label = (bytes(m.label) + b"\0\0")[:2]
    down = m.down not in (b"\x00", 0)
    txt = bytes(m.txt)
    if not LM.keep(down, label, txt, m.txt_len, downlink_only=downlink_only, skip_empty=False, labels=labels):
        return None
    if not down or m.bs == b"\x03":
        return None
    decoded, fields = LM.decode(label, txt, m.txt_len)
    sec, usec = tv(t0[0], t0[1], m.soh_sample)
    e_ok = LM.keep(down, label, txt, m.txt_len, downlink_only=downlink_only, skip_empty=skip_empty, labels=labels)
    return Event(m.addr, m.fid, m.chn, m.soh_sample, m.end_sample, sec, usec, tuple(fields[f] for f in FIELDS), e_ok)


def _new_entry(ev):
    return dict(addr=ev.addr, fid=b"\0" * 7, nbm=0, chm=0, first_chn=ev.chn, last_chn=ev.chn, ts_sample=ev.soh, tl_sample=ev.soh,
                ts=(ev.sec, ev.usec), tl=(ev.sec, ev.usec), fields=[b"\0" * 4] * 7, rt=0)


def _update(fl, ev):
    """output.c:386-399"""
    fl["fid"] = ev.fid
    fl["tl"] = (ev.sec, ev.usec)
    fl["tl_sample"] = ev.soh
    fl["last_chn"] = ev.chn
    fl["chm"] |= 1 << (ev.chn % 64)
    fl["nbm"] += 1
    fl["fields"] = [new if new[0] else old for old, new in zip(fl["fields"], ev.fields)]


def _route(fl, ev):
    """routejson() (output.c:428-456), called only for a message that passed -e"""
    if ev.e_ok and fl["rt"] == 0 and fl["fid"][0] and fl["fields"][1][0] and fl["fields"][0][0]:
        fl["rt"] = 1
        return dict(soh_sample=ev.soh, sec=ev.sec, usec=ev.usec, chn=ev.chn, fid=fl["fid"], sa=fl["fields"][1], da=fl["fields"][0], addr=fl["addr"])
    return None


class ListWalk:
    """the reference: a list, most recently updated first, scanned for expired entries after every message"""

    def __init__(self, mdly=600):
        self.mdly, self.head, self.routes = int(mdly), [], []
        self.seen, self.recreated = set(), 0                          # aircraft ever entered; entries made anew after an expiry

    def add(self, ev):
        fl = None
        for i, f in enumerate(self.head):                              # output.c:366-372
            if f["addr"] == ev.addr:
                fl = self.head.pop(i)
                break
        if fl is None:
            fl = _new_entry(ev)
            self.recreated += ev.addr in self.seen
            self.seen.add(ev.addr)
        _update(fl, ev)
        self.head.insert(0, fl)                                        # output.c:401-405
        self.head = [f for f in self.head if not f["tl"][0] < ev.sec - self.mdly]      # output.c:407-423
        r = _route(fl, ev)
        if r:
            self.routes.append(r)
        return r

    def entries(self):
        return self.head


class LazyTable:
    """the device's rule: an entry is live iff tl_sec + mdly >= G (the largest tv_sec seen); a message restarts its aircraft's
    entry when the largest tv_sec seen BEFORE it exceeds the entry's tl_sec + mdly"""

    def __init__(self, mdly=600):
        self.mdly, self.tab, self.G, self.seq, self.routes = int(mdly), {}, None, 0, []

    def add(self, ev):
        fl = self.tab.get(ev.addr)
        if fl is None or (self.G is not None and self.G > fl["tl"][0] + self.mdly):
            fl = self.tab[ev.addr] = _new_entry(ev)
        _update(fl, ev)
        self.seq += 1
        fl["seq"] = self.seq
        self.G = ev.sec if self.G is None else max(self.G, ev.sec)
        r = _route(fl, ev)
        if r:
            self.routes.append(r)
        return r

    def entries(self):
        live = [f for f in self.tab.values() if f["tl"][0] + self.mdly >= self.G]
        return sorted(live, key=lambda f: -f["seq"])


def entry_key(f):
    """everything an entry holds, for comparing two models"""
    return (f["addr"], f["fid"], f["nbm"], f["chm"], f["first_chn"], f["last_chn"], f["ts_sample"], f["tl_sample"], f["ts"], f["tl"],
            tuple(f["fields"]), f["rt"])


def flight_bytes(f):
    """the 120-byte acg_flight of an entry"""
    return (f["addr"] + f["fid"] + bytes([f["rt"]]) + struct.pack("<iiiiQqqqqii", f["nbm"], f["first_chn"], f["last_chn"], 0, f["chm"],
            f["ts_sample"], f["tl_sample"], f["ts"][0], f["tl"][0], f["ts"][1], f["tl"][1]) +
            b"".join(x + b"\0" for x in f["fields"]) + b"\0" * 5)


def route_bytes(r):
    """the 56-byte acg_route"""
    return (struct.pack("<qqii", r["soh_sample"], r["sec"], r["usec"], r["chn"]) + r["fid"] + r["sa"] + b"\0" + r["da"] + b"\0" +
            r["addr"] + b"\0" * 7)


def batch_order(events):
    """the order a pass applies the events of one drain / collect call in: ascending (end_sample, chn)"""
    return sorted(events, key=lambda e: (e.end, e.chn))


def monitor_row(f, nbch):
    """printmonitor()'s row (output.c:471-478) as (addr, fid, nbm, mask, DEP, ARR, ETA)"""
    s = lambda b: bytes(b).split(b"\0")[0].decode("latin1")
    return [s(f["addr"]), s(f["fid"]), f["nbm"], "".join("x" if (f["chm"] >> i) & 1 else "." for i in range(nbch)),
            s(f["fields"][1]), s(f["fields"][0]), s(f["fields"][2])]


def record_of(addr, label, bid, text, chn, end_sample, soh_sample):
    """outputmsg()'s field split (output.c:502-568) of a transmission given by its parts, with the attributes event_of() reads:
    dots leave the address, a downlink's text starts with message number (4) and flight id (6), no text at all = an ETX-only block"""
    from types import SimpleNamespace
    down = b"0" <= bid <= b"9"
    body = bytes(text)
    fid = b""
    if body and down:
        fid, body = body[4:10], body[10:]
    return SimpleNamespace(addr=bytes(addr).replace(b".", b""), fid=fid.split(b"\0")[0], label=bytes(label).replace(b"\x7f", b"d"),
                           down=1 if down else 0, bs=b"\x02" if text else b"\x03", txt=body + b"\0" * (242 - len(body)), txt_len=len(body),
                           chn=chn, end_sample=end_sample, soh_sample=soh_sample)
