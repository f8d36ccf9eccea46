"""A Python model of the two outputs the reference prints from its flight list: printmonitor()'s screen (output.c:458-484, -o 3)
and routejson()'s line through cJSON_PrintPreallocated(.., fmt = 0) (output.c:428-456,677-683, -o 5), byte for byte, written from
the reference's format strings independently of acarsdec_amd/csrc/flight_text.hip.  Built on flight_model (the entries and routes),
json_model (print_number, the string escape) and text_model (gmtime's calendar).  The CPU tests check it against the bytes the
reference program printed (tests/golden/monitor_golden.json); the GPU tests check the device against it.

An entry is a flight_model entry: a dict with addr, fid, nbm, chm, ts = (sec, usec), tl, fields = [da, sa, eta, gout, gin, woff,
won]; a route is a flight_model route: a dict with sec, usec, fid, sa, da."""
import re

import json_model as JM
import text_model as TM

CLS = b"\x1b[H\x1b[2J"                                               # cls(), output.c:103-106
TITLE = b"             Acarsdec monitor "
COLUMNS = b"\n Aircraft Flight   Nb Channels     First    DEP   ARR   ETA\n"
CLS_LEN, HDR_LEN, ROW_MAX, LINE_MAX = 7, 110, 78, 363
MAXNBCHANNELS = 16
TIME_RE = rb"\d\d:\d\d:\d\d\.\d\d\d"
TIME_MASK = b"hh:mm:ss.mmm"
T0 = (1700000000, 250000)                                            # the sample clock's start in the tests of this format


def time_text(sec, usec):
    """printtime(): "%02d:%02d:%02d.%03ld" of gmtime_r(tv_sec) and tv_usec / 1000 (output.c:138-146)"""
    return TM.date_text(sec, usec)[11:]


def row(f, nbch):
    """output.c:471-478"""
    cs = JM.cstr
    out = b" %-8s %-7s %3d " % (cs(f["addr"], 8), cs(f["fid"], 7), f["nbm"])
    out += b"".join((b"x" if (f["chm"] >> i) & 1 else b".") if i < nbch else b" " for i in range(MAXNBCHANNELS))
    out += b" " + time_text(*f["ts"])
    for k in (1, 0, 2):                                               # sa, da, eta of (da, sa, eta, ...)
        s = cs(f["fields"][k], 4)
        out += b" %4s " % s if s else b"      "
    return out + b"\n"


def header(tv):
    """output.c:462-465"""
    return CLS + TITLE + time_text(*tv) + COLUMNS


def header_tv(entries, t0, soh_sample):
    """the time acg_flight_monitor_text prints in the header: the named message's tv; negative: the newest entry's tl, or t0"""
    if soh_sample >= 0:
        return JM.tv(t0, soh_sample)
    return tuple(entries[0]["tl"]) if entries else tuple(t0)


def frame(entries, nbch, tv):
    return header(tv) + b"".join(row(f, nbch) for f in entries)


def row_spans(entries, nbch):
    """(first byte, one past the last byte) of every row within its frame"""
    out, at = [], HDR_LEN
    for f in entries:
        n = len(row(f, nbch))
        out.append((at, at + n))
        at += n
    return out


def route_line(r, station=b""):
    """output.c:442-447 printed by cJSON (fmt = 0), and the newline of output.c:680"""
    out = b'{"timestamp":' + JM.print_number(JM.tv_double(r["sec"], r["usec"])).encode()
    if JM.cstr(station):
        out += b',"station_id":' + JM.quoted(station)
    return out + b',"flight":' + JM.quoted(r["fid"], 7) + b',"depa":' + JM.quoted(r["sa"], 4) + b',"dsta":' + JM.quoted(r["da"], 4) + b"}\n"


def mask_times(b):
    """every printtime() token masked: the reference's file front end stamps the wall clock"""
    return re.sub(TIME_RE, TIME_MASK, b)


def mask_route(line):
    """a route line with its timestamp number masked"""
    head = b'{"timestamp":'
    assert line.startswith(head), line[:40]
    return head + b"T" + line[line.index(b",", len(head)):]


def split_frames(blob):
    """the frames of a -o 3 capture: everything from a cls() that is followed by the title up to the next one (the reference
    also clears the screen once at start-up)"""
    parts = blob.split(CLS)[1:]
    return [CLS + p for p in parts if p.startswith(TITLE)]


def entry_of(f):
    """a flight_model entry from an acg_flight record (K.Flight)"""
    c = lambda b, n: bytes(b).split(b"\0")[0][:n].ljust(n, b"\0")
    return dict(addr=c(f.addr, 8), fid=c(f.fid, 7), nbm=int(f.nbm), chm=int(f.chm), first_chn=int(f.first_chn), last_chn=int(f.last_chn),
                ts_sample=int(f.ts_sample), tl_sample=int(f.tl_sample), ts=(int(f.ts_sec), int(f.ts_usec)), tl=(int(f.tl_sec), int(f.tl_usec)),
                fields=[c(getattr(f, k), 4) for k in ("da", "sa", "eta", "gout", "gin", "woff", "won")], rt=int(f.rt))


def route_of(r):
    """a flight_model route from an acg_route record (K.Route)"""
    c = lambda b, n: bytes(b).split(b"\0")[0][:n].ljust(n, b"\0")
    return dict(soh_sample=int(r.soh_sample), sec=int(r.sec), usec=int(r.usec), chn=int(r.chn), fid=c(r.fid, 7), sa=c(r.sa, 4), da=c(r.da, 4),
                addr=c(r.addr, 8))


# ---- designed records: what no traffic produces (the GPU self test's inputs; the CPU tests assert their seam coverage) --------
ROW_COUNTS = (0, 1, 2, 63, 64, 65, 256, 257, 1025)                    # the last two cross the scan's 256-rank workgroups
ROUTE_COUNTS = (0, 1, 64, 65, 257)
NBCH = (0, 1, 3, 16)
HDR_SOH = (-1, 0, 2 ** 31 + 5, 2 ** 32 + 7, 2 ** 40 + 11)
NBM = (1, 999, 1000, 2 ** 31 - 1, 7, 42, 1000, 12345)
CHM = (0xFFFFFFFFFFFFFFFF, 0, 0xFFFFFFFFFFFF0000, 0b101, 0x8001, 0x1234)
# usec 0, 999, 999999; a day's last and first second; tv_sec >= 2^31 and >= 2^32
TIMES = ((1700006399, 0), (1700006400, 999), (1700006399, 999999), (1700000000, 0), (2 ** 31, 999999), (2 ** 32 + 5, 1000), (2 ** 33, 123456),
         (4107542399, 999), (4107542400, 0))
STATIONS = (b"", bytes(range(1, 32)) + b"\x1f", b'st"1\\')                  # none; 32 control characters; a quote and a backslash
_FIELD = (b"EGLL", b"", b"ABC", b"K", b"KJFK", b"X1", b"0815", b"")
_STRINGS = (b'A"\\\x01\xe9\x7f', b"XY0123", b"\n\t\r\x1f\x08\x0c", b"", b"\x80\xff", b"Q")


def designed_entries(n, salt):
    """n entries that cycle through the cases at co-prime periods, so that they meet in many combinations: nbm of three, four and
    ten digits (rows of 70, 71 and 77 bytes), an empty fid, fields empty and shorter than 4, a 7-character addr"""
    out = []
    for i in range(n):
        k = i + salt
        addr = (b"N%06d" % (k % 1000000)) if k % 3 == 0 else (b"N%d" % (k % 977))
        fid = b"" if k % 5 == 1 else (b"XY%04d" % (k % 10000))
        fields = [_FIELD[(k + 3 * j) % len(_FIELD)] for j in range(7)]
        if k % 11 == 4:
            fields[0] = fields[1] = fields[2] = b""
        pad = lambda b, m: b + b"\0" * (m - len(b))
        out.append(dict(addr=pad(addr, 8), fid=pad(fid, 7), nbm=NBM[k % len(NBM)], chm=CHM[k % len(CHM)], first_chn=k % 16, last_chn=(k + 1) % 16,
                        ts_sample=12500 * k, tl_sample=12500 * k + 77, ts=TIMES[k % len(TIMES)], tl=TIMES[(k + 4) % len(TIMES)],
                        fields=[pad(x, 4) for x in fields], rt=k % 2))
    return out


def designed_routes(n, salt):
    out = []
    pad = lambda b, m: b + b"\0" * (m - len(b))
    for i in range(n):
        k = i + salt
        fid = _STRINGS[k % len(_STRINGS)] if k % 4 else b"ZW%04d" % (k % 10000)
        sa, da = _STRINGS[(k + 2) % len(_STRINGS)][:4], _FIELD[k % len(_FIELD)]
        sec, usec = TIMES[k % len(TIMES)]
        out.append(dict(soh_sample=1000 * k, sec=sec, usec=(usec + 1009 * k) % 1000000, chn=k % 16, fid=pad(fid, 7), sa=pad(sa, 4), da=pad(da, 4),
                        addr=pad(b"N%d" % k, 8)))
    return out


def designed_cases():
    """one case per row count; the other dimensions cycle, so that every nbch, header time, route count and station turns up"""
    cases = []
    for j, n in enumerate(ROW_COUNTS):
        cases.append(dict(entries=designed_entries(n, 17 * j), routes=designed_routes(ROUTE_COUNTS[j % len(ROUTE_COUNTS)], 5 * j),
                          nbch=NBCH[j % len(NBCH)], hdr_soh=HDR_SOH[j % len(HDR_SOH)], station=STATIONS[j % len(STATIONS)], t0=T0))
    return cases
