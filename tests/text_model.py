"""A Python model of the reference's per-message text formats, written from the reference's behaviour independently of
acarsdec_amd/csrc/text.hip: printoneline() (output.c:327-346, -o 1), printmsg() (output.c:162-224, -o 2, the build without
libacars), and the packets Netoutpp() (netout.c:101-120, -N) and Netoutsv() (netout.c:122-140, -n) format.  The CPU tests check
the first two against what the reference program printed (tests/golden/msgtext_golden.json); the GPU tests check the device against
the model, byte for byte.

A record is anything with the fields of K.Msg / the oracle's OrcMsg; strings are C strings (they end at their first NUL)."""
import datetime
import re
from fractions import Fraction

import numpy as np

import label_model as LM
from json_model import cstr, keep, tv  # noqa: F401  (tv: t0 + soh_sample / 12500 s in integers; keep: the CLI's filters)

ONELINE, STD, PP, SV = 1, 2, 3, 4
F_DATE, F_FREQ = 1, 2
REC_MAX = 704
FLAGS_OF = {ONELINE: (0, F_DATE), STD: (0, F_DATE, F_FREQ, F_DATE | F_FREQ), PP: (0,), SV: (0,)}
OOOI_LINES = (("da", b"Destination Airport : "), ("sa", b"Departure Airport : "), ("eta", b"Estimation Time of Arrival : "),
              ("gout", b"Gate out Time : "), ("gin", b"Gate in Time : "), ("woff", b"Wheels off Tme : "), ("won", b"Wheels on Time : "))
DATE_RE = rb"\d\d/\d\d/\d{4} \d\d:\d\d:\d\d\.\d{3}"
DATE_MASK = b"DD/MM/YYYY hh:mm:ss.mmm"
# 10^9; 2038-01-19 03:14:07 / 08; both sides of 2100-02-28 / 03-01 (no leap day) and of 2104-02-29 (one)
NAMED_SECONDS = (10 ** 9, 2 ** 31 - 1, 2 ** 31, 4107542399, 4107542400, 4107542400 - 86400, 4233686399, 4233686400, 4233772799, 4233772800)


def pad(s, width, maxlen=None):
    """"%<width>s" of a C string: right-justified to at least width, never cut"""
    s = cstr(s, maxlen)
    return b" " * max(0, width - len(s)) + s


def ch(v):
    """"%1c": the byte itself, a NUL included"""
    return bytes([v]) if isinstance(v, int) else (bytes(v)[:1] or b"\0")


def level_text(f):
    """"%+5.1f" of a float32: its exact value rounded half-even to one decimal, the sign forced, space padded to 5; non-finite as
    glibc prints them"""
    f = np.float32(f)
    sign = "-" if np.signbit(f) else "+"
    if np.isnan(f):
        body = "nan"
    elif np.isinf(f):
        body = "inf"
    else:
        x = abs(Fraction(float(f))) * 10
        n = x.numerator // x.denominator
        r = x - n
        if r > Fraction(1, 2) or (r == Fraction(1, 2) and n % 2):
            n += 1
        body = "%d.%d" % (n // 10, n % 10)
    return (sign + body).rjust(5).encode()


def level_libc(f):
    """the same from the C library's formatter (Python's % drops a NaN's sign; glibc prints it)"""
    f = np.float32(f)
    if np.isnan(f):
        return (("-" if np.signbit(f) else "+") + "nan").rjust(5).encode()
    return ("%+5.1f" % f).encode()


def trunc_int(f):
    """(int)lvl as the x86 build converts it: toward zero; NaN, infinities and everything outside int give -2147483648"""
    f = np.float32(f)
    if not np.isfinite(f) or not (-2147483648.0 <= float(f) < 2147483648.0):
        return -2147483648
    return int(float(f))


def date_text(sec, usec, ms=True):
    """printdate(): "%02d/%02d/%04d %02d:%02d:%02d.%03ld" of gmtime_r (proleptic Gregorian, no leap seconds)"""
    d = datetime.datetime(1970, 1, 1) + datetime.timedelta(seconds=int(sec))
    s = "%02d/%02d/%04d %02d:%02d:%02d" % (d.day, d.month, d.year, d.hour, d.minute, d.second)
    return (s + (".%03d" % (usec // 1000) if ms else "")).encode()


def freq_token(fr_hz):
    """printmsg()'s "F:%3.3f " of the double Fr / 1000000.0 (output.c:168-169)"""
    return b"F:%3.3f " % (fr_hz / 1000000.0)


def _fields(m):
    txt_len = max(0, min(int(m.txt_len), 242))
    txt = cstr(bytes(m.txt)[:txt_len])
    label = (bytes(m.label) + b"\0\0")[:2]
    return txt, txt_len, label


def _unline(t):
    return t.replace(b"\n", b" ").replace(b"\r", b" ")


def oneline(m, chn, date=None):
    """date: printdate()'s text or None (the reference: inmode == 2)"""
    txt, _, label = _fields(m)
    out = b"#%d (L:%s E:%d) " % (chn + 1, level_text(m.lvl), int(m.err)) + (date or b"")
    out += b" " + pad(m.addr, 7, 7) + b" " + pad(m.fid, 6, 6) + b" " + ch(m.mode) + b" " + pad(label, 2, 2) + b" " + pad(m.no, 4, 4) + b" "
    return out + _unline(txt[:59]) + b"\n"


def std(m, chn, date=None, freq=None, oooi=None):
    """freq: freq_token() or None (the reference: inmode < 3); oooi: (decoded, {field: bytes}) (default: label_model's decode)"""
    txt, txt_len, label = _fields(m)
    out = b"\n[#%d (" % (chn + 1) + (freq or b"") + b"L:%s E:%d) " % (level_text(m.lvl), int(m.err)) + (date or b"")
    out += b" " + b"-" * 32 + b"\n"
    out += b"Mode : " + ch(m.mode) + b" " + b"Label : " + pad(label, 2, 2) + b" "
    bid = ch(m.bid)
    if bid != b"\0":
        out += b"Id : " + bid + b" "
        out += b"Nak\n" if ch(m.ack) == b"!" else b"Ack : " + ch(m.ack) + b"\n"
        out += b"Aircraft reg: " + cstr(m.addr, 7) + b" "
        if b"0" <= bid <= b"9":
            out += b"Flight id: " + cstr(m.fid, 6) + b"\n" + b"No: " + pad(m.no, 4, 4)
    out += b"\n"
    if txt:
        out += txt + b"\n"
    if ch(m.be) == b"\x17":
        out += b"ETB\n"
    decoded, fields = oooi if oooi is not None else LM.decode(label, bytes(m.txt), txt_len)
    if decoded:
        out += b"#" * 26 + b"\n"
        for f, head in OOOI_LINES:
            v = cstr(fields[f], 4)
            if v:
                out += head + v + b"\n"
    return out


def _tail(m, txt):
    _, _, label = _fields(m)
    bid = ch(m.bid)
    return (ch(m.mode) + b" " + pad(m.addr, 7, 7) + b" " + ch(m.ack) + b" " + pad(label, 2, 2) + b" " + (bid if bid != b"\0" else b".") + b" " +
            pad(m.no, 4, 4) + b" " + pad(m.fid, 6, 6) + b" " + txt)


def pp(m):
    """the bytes of Netoutpp()'s snprintf ("AC%1c %7s %1c %2s %1c %4s %6s %s")"""
    return b"AC" + _tail(m, _unline(_fields(m)[0]))


def sv(m, chn, sec, station=b""):
    """the bytes of Netoutsv()'s snprintf ("%8s %1d %02d/%02d/%04d %02d:%02d:%02d %1d %03d %1c %7s %1c %2s %1c %4s %6s %s")"""
    return (pad(station, 8) + b" %d " % (chn + 1) + date_text(sec, 0, ms=False) + b" %d %03d " % (int(m.err), trunc_int(m.lvl)) +
            _tail(m, _fields(m)[0]))


def record(m, chn, fmt, flags=0, t0=(1700000000, 0), station=b"", fr_hz=0, oooi=None):
    """what the sink hands out for m: fmt / flags as acg_text_config, tv = t0 + m.soh_sample / 12500 s (a record without a
    soh_sample, such as the oracle's, is stamped t0)"""
    sec, usec = tv(t0, getattr(m, "soh_sample", 0))
    date = date_text(sec, usec) if flags & F_DATE else None
    if fmt == ONELINE:
        return oneline(m, chn, date)
    if fmt == STD:
        return std(m, chn, date, freq_token(fr_hz) if flags & F_FREQ else None, oooi)
    if fmt == PP:
        return pp(m)
    assert fmt == SV
    return sv(m, chn, sec, station)


def mask_dates(b):
    """the date's digits replaced by a placeholder of the same shape"""
    return re.sub(DATE_RE, DATE_MASK, b)


def split_oneline(blob):
    """-o 1 stdout into records at "#<digits> (L:" behind a newline: a record is one line unless a header field holds a '\\n' (the
    text's are substituted), and what follows such a newline never looks like a record's start in the fixtures"""
    at = [m.start() for m in re.finditer(rb"(?:\A|(?<=\n))#\d+ \(L:[ +-]", blob)]
    assert (not blob and not at) or (at and at[0] == 0), blob[:40]
    return [blob[a:b] for a, b in zip(at, at[1:] + [len(blob)])]


def split_std(blob):
    """-o 2 stdout into records at "\\n[#<digits> (": a text line of the fixtures never starts like that"""
    at = [m.start() for m in re.finditer(rb"\n\[#\d+ \((?:F:[-\d.]+ )?L:", blob)]
    assert (not blob and not at) or (at and at[0] == 0), blob[:40]
    return [blob[a:b] for a, b in zip(at, at[1:] + [len(blob)])]


def chn_of(rec):
    """the channel a ONELINE / STD record names"""
    return int(re.match(rb"\n?\[?#(\d+) \(", rec).group(1)) - 1

