"""A Python model of the reference's JSON line: buildjson() (output.c:227-324) printed by cJSON_PrintPreallocated(.., fmt = 0)
in the build without libacars, written from the reference's behaviour independently of acarsdec_amd/csrc/json.hip.  The CPU tests
check it against the lines the reference program printed (tests/golden/msgjson_golden.json); the GPU tests check the device
against it, byte for byte.

Two number printers are stated twice: as the C library does it ('%1.15g' / '%1.17g', '%2.1f'), and in the integer arithmetic
the kernel uses, so that the tests can hold one against the other."""
import struct

import numpy as np

import label_model as LM

LINE_MAX = 2496
_TWO = {0x22: b'\\"', 0x5C: b"\\\\", 0x08: b"\\b", 0x0C: b"\\f", 0x0A: b"\\n", 0x0D: b"\\r", 0x09: b"\\t"}
OOOI_KEYS = (("sa", b"depa"), ("da", b"dsta"), ("eta", b"eta"), ("gout", b"gtout"), ("gin", b"gtin"), ("woff", b"wloff"), ("won", b"wlin"))


def cstr(b, maxlen=None):
    """the C string at the start of b (at most maxlen bytes of it)"""
    b = bytes(b)
    if maxlen is not None:
        b = b[:maxlen]
    return b.split(b"\0")[0]


def escape(s):
    """print_string_ptr (cJSON.c:828-950) of a C string, without the quotes"""
    out = bytearray()
    for b in cstr(s):
        if b in _TWO:
            out += _TWO[b]
        elif b < 32:
            out += b"\\u%04x" % b
        else:
            out.append(b)
    return bytes(out)


def quoted(s, maxlen=None):
    return b'"' + escape(cstr(s, maxlen)) + b'"'


# ---- the time stamp -------------------------------------------------------------------------------------------------------
def tv(t0, soh_sample):
    """t0 + soh_sample / 12500 s in integers: a sample is exactly 80 us"""
    us = t0[1] + soh_sample * 80
    return t0[0] + us // 1000000, us % 1000000


def tv_double(sec, usec):
    """output.c:244"""
    return float(sec) + float(usec) / 1e6


def print_number(t):
    """print_number (cJSON.c:475-506) for a finite double"""
    s = "%1.15g" % t
    if float(s) != t:
        s = "%1.17g" % t
    return s


def _round_shift(x, s):
    q, r, half = x >> s, x & ((1 << s) - 1), 1 << (s - 1)
    return q + 1 if (r > half or (r == half and (q & 1))) else q


def print_number_int(sec, usec):
    """The same text from integer arithmetic on the double's fraction (the kernel's algorithm), for 10^9 <= sec < 10^10 - 2:
    t = I + k / 2^s, N = k 10^p / 2^s rounded half-even for p = 5; that text parses back iff 2 |N 2^s - k 10^5| < 10^5 (or equal
    and k even); otherwise p = 7.  Trailing zeros are stripped."""
    assert 10 ** 9 <= sec < 10 ** 10 - 2 and 0 <= usec < 10 ** 6
    bits = struct.unpack("<Q", struct.pack("<d", tv_double(sec, usec)))[0]
    s = 52 - (((bits >> 52) & 0x7FF) - 1023)
    mant = (bits & ((1 << 52) - 1)) | (1 << 52)
    I, k = mant >> s, mant & ((1 << s) - 1)
    p, N = 5, _round_shift(k * 10 ** 5, s)
    dist = abs((N << s) - k * 10 ** 5)
    if not (2 * dist < 10 ** 5 or (2 * dist == 10 ** 5 and k % 2 == 0)):
        p, N = 7, _round_shift(k * 10 ** 7, s)
    if N == 10 ** p:
        I, N = I + 1, 0
    frac = ("%0*d" % (p, N)).rstrip("0")
    return str(I) + ("." + frac if frac else "")


# ---- the level ------------------------------------------------------------------------------------------------------------
def level_text(f):
    """snprintf(8 bytes, "%2.1f", f) for a float32 (output.c:250), from integers: (double)f * 10 is exact, rounded half-even; the
    sign is the sign bit; the buffer cuts the text to 7 characters"""
    f = np.float32(f)
    neg = bool(np.signbit(f))
    if np.isnan(f):
        return ("-nan" if neg else "nan")
    if np.isinf(f):
        return ("-inf" if neg else "inf")
    from fractions import Fraction
    x = abs(Fraction(float(f))) * 10
    n = x.numerator // x.denominator
    r = x - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n % 2):
        n += 1
    return (("-" if neg else "") + "%d.%d" % (n // 10, n % 10))[:7]


def level_libc(f):
    """'%2.1f' cut to 7 characters.  (Python's % drops the sign of a NaN, glibc prints it: "-nan"; tests/json_num_check.cpp holds
    the kernel's printer against glibc itself.)"""
    f = np.float32(f)
    return (("-" if np.isnan(f) and np.signbit(f) else "") + "%2.1f" % f)[:7]


def freq_token(fr_hz):
    """output.c:232,248"""
    return ("%3.3f" % np.float32(fr_hz / 1000000.0))[:7].encode()


# ---- the line -------------------------------------------------------------------------------------------------------------
def line(m, chn, ts_token, station=b"", freq=b"0.000", app=(b"acarsdec", b""), level=None, oooi=None):
    """The line of a split record m (a K.Msg / OrcMsg, or anything with their fields), bytes, '\\n' included.  ts_token: the
    number behind "timestamp"; level: the level's text (default: from m.lvl); oooi: (decoded, {field: 4 bytes}) (default:
    label_model's decode of the record)."""
    f1 = lambda v: bytes(v)[:1] if not isinstance(v, int) else bytes([v])
    txt_len = max(0, min(int(m.txt_len), 242))
    txt = bytes(m.txt)[:txt_len]
    label = (bytes(m.label) + b"\0\0")[:2]
    out = [b'{"timestamp":' + ts_token]
    if cstr(station):
        out.append(b',"station_id":' + quoted(station))
    lv = level if level is not None else level_text(m.lvl)
    out.append(b',"channel":%d,"freq":%s,"level":%s,"error":%d' % (chn, freq, lv.encode() if isinstance(lv, str) else lv, int(m.err)))
    out.append(b',"mode":' + quoted(f1(m.mode)))
    out.append(b',"label":' + quoted(label, 2))
    bid = f1(m.bid)
    if cstr(bid):
        out.append(b',"block_id":' + quoted(bid))
        ack = f1(m.ack)
        out.append(b',"ack":false' if ack == b"!" else b',"ack":' + quoted(ack))
        out.append(b',"tail":' + quoted(m.addr, 7))
        if b"0" <= bid <= b"9":
            out.append(b',"flight":' + quoted(m.fid, 6) + b',"msgno":' + quoted(m.no, 4))
    if cstr(txt):
        out.append(b',"text":' + quoted(txt))
    if f1(m.be) == b"\x17":
        out.append(b',"end":true')
    decoded, fields = oooi if oooi is not None else LM.decode(label, bytes(m.txt), txt_len)
    if decoded:
        for f, key in OOOI_KEYS:
            if cstr(fields[f]):
                out.append(b',"' + key + b'":' + quoted(fields[f], 4))
    out.append(b',"app":{"name":' + quoted(app[0]) + b',"ver":' + quoted(app[1]) + b"}}\n")
    return b"".join(out)


def cut_timestamp(ln):
    """(the line with the time stamp's number cut out, that number)"""
    head = b'{"timestamp":'
    assert ln.startswith(head), ln[:40]
    end = ln.index(b",", len(head))
    return head + ln[end:], ln[len(head):end]


def keep(m, downlink_only=False, skip_empty=False, labels=()):
    """the CLI's filters on a split record (label_model.keep)"""
    return LM.keep(m.down not in (b"\x00", 0), (bytes(m.label) + b"\0\0")[:2], bytes(m.txt), m.txt_len, downlink_only=downlink_only,
                   skip_empty=skip_empty, labels=labels)
