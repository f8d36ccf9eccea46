"""A Python model of the batch sink's filters and of label.c's DecodeLabel() as a table, written from the reference's behaviour
independently of the device table in acarsdec_amd/csrc/label.hip.  The CPU tests check it against the reference program's JSON
(tests/golden/labels_golden.json); the GPU tests check the device against it.

Rules the device follows too (include/acarsdec_amd.h): bytes at or past txt_len read as 0; a label is the C string of its two
bytes; a -b token longer than a label never matches."""

FIELDS = ("da", "sa", "eta", "gout", "gin", "woff", "won")          # oooi_t order (acarsdec.h:94-102)
JSON_KEYS = {"sa": "depa", "da": "dsta", "eta": "eta", "gout": "gtout", "gin": "gtin", "woff": "wloff", "won": "wlin"}

# label -> (guards, copies, optional prefix).  A guard is (offset, alternatives): the bytes at offset equal one of them.
# A copy is (field, offset): 4 bytes.  "26" marks label 26's own routine.
_Q = lambda *c: ((), c, None)
TABLE = {
    "10": (((0, (b"ARR01",)),), (("da", 12), ("eta", 16)), None),
    "11": (((13, (b"/DS ",)), (21, (b"/ETA ",))), (("da", 17), ("eta", 26)), None),
    "12": (((4, (b",",)),), (("sa", 0), ("da", 5)), None),
    "15": (((0, (b"FST01",)),), (("sa", 5), ("da", 9)), None),
    "17": (((0, (b"ETA ",)), (8, (b",",)), (13, (b",",))), (("eta", 4), ("sa", 9), ("da", 14)), None),
    "1G": (((4, (b",",)),), (("sa", 0), ("da", 5)), None),
    "20": (((0, (b"RST",)),), (("sa", 22), ("da", 26)), None),
    "21": (((6, (b",",)), (11, (b",",))), (("sa", 7), ("da", 12)), None),
    "26": "26",
    "2N": (((0, (b"TKO01",)), (11, (b"/",))), (("sa", 20), ("da", 24)), None),
    "2Z": ((), (("da", 0),), None),
    "33": (((0, (b",",)), (20, (b",",)), (25, (b",",))), (("sa", 21), ("da", 26)), None),
    "39": (((0, (b"GTA01",)), (15, (b"/",))), (("sa", 24), ("da", 28)), None),
    "44": (((0, (b"POS0", b"ETA0")), (4, (b"2", b"3")), (23, (b",",)), (28, (b",",)), (33, (b",",)), (38, (b",",)), (43, (b",",))),
           (("da", 24), ("eta", 29), ("eta", 44)), b"00"),
    "45": (((0, (b"A",)),), (("da", 1),), None),
    "80": (((6, (b"/DEST",)),), (("da", 12),), None),
    "83": (((4, (b",",)),), (("sa", 0), ("da", 5)), None),
    "8D": (((4, (b",",)), (35, (b",",)), (40, (b",",))), (("sa", 36), ("da", 41)), None),
    "8E": (((4, (b",",)),), (("da", 0), ("eta", 5)), None),
    "8S": (((4, (b",",)),), (("da", 0), ("eta", 5)), None),
    "RB": "26",
    "Q1": _Q(("sa", 0), ("gout", 4), ("woff", 8), ("won", 12), ("gin", 16), ("da", 24)),
    "Q2": _Q(("sa", 0), ("eta", 4)),
    "QA": _Q(("sa", 0), ("gout", 4)),
    "QB": _Q(("sa", 0), ("woff", 4)),
    "QC": _Q(("sa", 0), ("won", 4)),
    "QD": _Q(("sa", 0), ("gin", 4)),
    "QE": _Q(("sa", 0), ("gout", 4), ("da", 8)),
    "QF": _Q(("sa", 0), ("woff", 4), ("da", 8)),
    "QG": _Q(("sa", 0), ("gout", 4), ("gin", 8)),
    "QH": _Q(("sa", 0), ("gout", 4)),
    "QK": _Q(("sa", 0), ("won", 4), ("da", 8)),
    "QL": _Q(("da", 0), ("gin", 8), ("sa", 13)),
    "QM": _Q(("da", 0), ("sa", 8)),
    "QN": _Q(("da", 4), ("eta", 8)),
    "QP": _Q(("sa", 0), ("da", 4), ("gout", 8)),
    "QQ": _Q(("sa", 0), ("da", 4), ("woff", 8)),
    "QR": _Q(("sa", 0), ("da", 4), ("won", 8)),
    "QS": _Q(("sa", 0), ("da", 4), ("gin", 8)),
    "QT": _Q(("sa", 0), ("da", 4), ("gout", 8), ("gin", 12)),
}


def _reader(txt, txt_len):
    n = max(0, min(int(txt_len), 242, len(txt)))
    return lambda i: txt[i] if 0 <= i < n else 0


def _eq(b, at, s):
    return all(b(at + k) == s[k] for k in range(len(s)))


def _find(b, start, c):
    """strchr from `start`: the index of c, or None at the first NUL"""
    i = start
    while True:
        x = b(i)
        if x == c:
            return i
        if x == 0:
            return None
        i += 1


def _label26(b):
    if not _eq(b, 0, b"VER/077"):
        return None
    p = _find(b, 0, 0x0A)
    if p is None:
        return None
    p += 1
    if not _eq(b, p, b"SCH/"):
        return None
    p = _find(b, p + 4, ord("/"))
    if p is None:
        return None
    copies = [("sa", p + 1), ("da", p + 6)]
    p = _find(b, p, 0x0A)
    if p is None:
        return copies
    p += 1
    if not _eq(b, p, b"ETA/"):
        return None
    return copies + [("eta", p + 4)]


def label_str(label):
    """the label as the C string the split reports (label[0], label[1]; label[2] is the terminator)"""
    l0, l1 = label[0], label[1]
    return b"" if l0 == 0 else bytes([l0]) if l1 == 0 else bytes([l0, l1])


def decode(label, txt, txt_len):
    """DecodeLabel(): (decoded, {field: 4 bytes}) -- all fields b"\\0" * 4 when not decoded"""
    b = _reader(bytes(txt), txt_len)
    spec = TABLE.get(label_str(label).decode("latin1"))
    out = {f: b"\0" * 4 for f in FIELDS}
    if spec is None:
        return 0, out
    if spec == "26":
        copies = _label26(b)
        if copies is None:
            return 0, out
    else:
        guards, cps, opt = spec
        base = 0
        if opt is not None and b(0) == opt[0]:
            if b(1) != opt[1]:
                return 0, out
            base = 2
        for off, alts in guards:
            if not any(_eq(b, base + off, a) for a in alts):
                return 0, out
        copies = [(f, base + off) for f, off in cps]
    for f, at in copies:
        out[f] = bytes(b(at + k) for k in range(4))
    return 1, out


def oooi_bytes(decoded, fields):
    """the 40-byte acg_oooi"""
    return b"".join(fields[f] + b"\0" for f in FIELDS) + bytes([decoded]) + b"\0" * 4


def json_keys(decoded, fields):
    """buildjson's OOOI keys (output.c:280-295)"""
    out = {}
    if decoded:
        for f in FIELDS:
            s = fields[f].split(b"\0")[0]
            if s:
                out[JSON_KEYS[f]] = s.decode("latin1")
    return out


def parse_label_filter(arg):
    """build_label_filter (strtok on ':'): the list of tokens, [] = no label filter"""
    if not arg:
        return []
    if isinstance(arg, str):
        arg = arg.encode("latin1")
    return [t for t in arg.split(b":") if t]


def keep(down, label, txt, txt_len, downlink_only=False, skip_empty=False, labels=(), valid=True):
    """output.c:537-540 (-A, -b) and 650 (-e) on a split record"""
    if not valid:
        return False
    if downlink_only and not down:
        return False
    if labels:
        s = label_str(label)
        if not s or s not in [bytes(t) for t in labels]:
            return False
    if skip_empty and _reader(bytes(txt), txt_len)(0) == 0:
        return False
    return True
