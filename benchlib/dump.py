"""bench.py --dump-outputs DIR: what the timed path computed in its last step, as float32 / float64 .npy files, so that two builds
of the project can be compared output for output (the input of a case is seeded: the same arguments give the same bytes).

  msg_fields.npy   float64 [n, f]   the acg_msg records (or, with --raw-blocks, the acg_frame blocks) the host received for the
                                    last pass of the last step, sorted by (chn, end_bit); columns MSG_FIELDS / FRAME_FIELDS
  msg_chars.npy    float32 [n, k]   their character fields as byte values: addr 8, label 3, no 5, fid 7, then txt (zero past
                                    txt_len); with --raw-blocks crc 2, then txt (zero past len)
  dm.npy           float32 [c, s]   the 12.5 kHz down-converter output of the last call (acg_read_dm) of DUMP_CHANNELS channels
  dm_channels.npy  float64 [c]      which channels (a fixed, seeded sample where the case has more)
  bits_vo.npy      float32 [c, b]   the demodulator's per-bit soft decisions of the last call (acg_read_bits), zero past the count
  bits_lvl.npy     float32 [c, b]   their levels, the same shape
  bits_count.npy   float64 [c]      how many bits each of those channels has in the last call
At most MAX_BYTES in all: beyond it a fixed, seeded sample of the records is kept (in record order)."""
import ctypes as C
import os

DUMP_CHANNELS = 128
MAX_BYTES = 64 << 20
MSG_FIELDS = ("chn", "err", "lvl", "txt_len", "end_bit", "end_sample", "soh_sample", "mode", "ack", "bid", "bs", "be", "down")
MSG_CHARS = ("addr", "label", "no", "fid")
FRAME_FIELDS = ("chn", "len", "err", "lvl", "end_bit", "end_sample", "soh_sample")


def _byte(v):
    """a c_char field as its byte value (ctypes reads it as b"" when it is NUL), anything else as a number"""
    return (v[0] if v else 0) if isinstance(v, bytes) else v


def last_step_outputs(dec, raw, start_sample, nch, call_samples, repair, bitlog, K):
    """the arrays of the module docstring.  raw: the record bytes the host received in the last pass and the drain behind it;
    start_sample: 12.5 kHz samples per channel before that pass (records that end before it belong to the pass before)."""
    import numpy as np
    rec = K.Msg if repair else K.Frame
    buf = b"".join(raw)
    n = len(buf) // C.sizeof(rec)
    arr = (rec * n).from_buffer_copy(buf) if n else []
    rows = sorted((r for r in arr if r.end_sample >= start_sample), key=lambda r: (int(r.chn), int(r.end_bit)))
    if repair:
        fields = np.array([[float(_byte(getattr(r, f))) for f in MSG_FIELDS] for r in rows], dtype=np.float64).reshape(-1, len(MSG_FIELDS))
        # (a c_char array reads as bytes up to its first NUL: padded back to the field's width)
        heads = [b"".join(getattr(r, f).ljust(getattr(rec, f).size, b"\0") for f in MSG_CHARS) for r in rows]
        texts = [bytes(r.txt[: max(0, min(int(r.txt_len), len(r.txt)))]) for r in rows]
    else:
        fields = np.array([[float(getattr(r, f)) for f in FRAME_FIELDS] for r in rows], dtype=np.float64).reshape(-1, len(FRAME_FIELDS))
        heads = [bytes(r.crc) for r in rows]
        texts = [bytes(r.txt[: max(0, min(int(r.len), len(r.txt)))]) for r in rows]
    return dict(fields=fields, heads=heads, texts=texts, per_channel=_per_channel(dec, nch, call_samples, bitlog))


def _per_channel(dec, nch, call_samples, bitlog):
    import numpy as np
    chans = np.arange(nch) if nch <= DUMP_CHANNELS else np.sort(np.random.default_rng(0xD0).choice(nch, DUMP_CHANNELS, replace=False))
    dm = np.stack([dec.dm(int(c), call_samples) for c in chans]).astype(np.float32)
    vo, lvl = [], []
    for c in (chans if bitlog else []):          # (--bitlog 0: the demodulator keeps no per-bit records)
        v, l_ = dec.bits(int(c))
        vo.append(v)
        lvl.append(l_)
    b = max([len(v) for v in vo] + [0])
    bits_vo = np.zeros((len(vo), b), dtype=np.float32)
    bits_lvl = np.zeros((len(vo), b), dtype=np.float32)
    for i, (v, l_) in enumerate(zip(vo, lvl)):
        bits_vo[i, : len(v)] = v
        bits_lvl[i, : len(l_)] = l_
    return dict(dm=dm, dm_channels=chans.astype(np.float64), bits_vo=bits_vo, bits_lvl=bits_lvl,
                bits_count=np.array([len(v) for v in vo], dtype=np.float64))


def write_outputs(d, out_dir):
    """writes the arrays of last_step_outputs() as <out_dir>/<name>.npy; returns {name: shape}"""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    per = d["per_channel"]
    fields, heads, texts = d["fields"], d["heads"], d["texts"]
    width = max([len(h) for h in heads] + [0]) + max([len(t) for t in texts] + [0])
    chars = np.zeros((len(texts), width), dtype=np.float32)
    for i, (h, t) in enumerate(zip(heads, texts)):
        b = np.frombuffer(h + t, dtype=np.uint8)
        chars[i, : b.size] = b
    fixed = sum(a.nbytes for a in per.values())
    row_bytes = fields.shape[1] * 8 + width * 4
    if row_bytes and fixed + len(texts) * row_bytes > MAX_BYTES:
        keep = max(0, (MAX_BYTES - fixed) // row_bytes)
        idx = np.sort(np.random.default_rng(0xD1).choice(len(texts), keep, replace=False))
        fields, chars = fields[idx], chars[idx]
    arrays = dict(msg_fields=fields, msg_chars=chars, **per)
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64) and np.all(np.isfinite(a)), name
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return {name: list(a.shape) for name, a in arrays.items()}
