"""The rules of the per-channel statistics table (acg_chan_stats, include/acarsdec_amd.h; csrc/stats.hip, the outcome byte of
csrc/blk.hip) restated in Python over RAW blocks: what the reference prints under -v for a block (blk_thread, acars.c:120-209)
and which of outputmsg()'s filters drops it first (output.c:537-540,650).  The two resets only the framing sees (acars.c:313,
336) are modelled too (framing_events) and pinned to the reference's lines, though the table does not count them: counting them
inside the demodulator was not free (profiles/LEDGER.md, "Per-channel reception statistics").  Plain module like the other models: tests/test_stats_model.py pins it to the
unmodified reference program's own stderr (tests/golden/stats_golden.json), tests/test_gpu_stats.py holds the device to it.

It wraps what the suite already has: repair_corpus.model_blk (the repair), label_model.keep (the three filter predicates) and
test_lean_framing_model.decode_acars (the framing machine).

`mutate` names a deliberately WRONG model (tests only: shows that the fixtures would notice a miscount):
  "last_filter"     a block several filters would drop is charged to the LAST of them instead of the first;
  "fixed_needs_crc" `fixed` is counted only when the CRC was bad (the reference prints it for every block with parity errors
                    whose search succeeded, acars.c:178 -- also when the CRC was clean);
  "del_after_repair" the DEL flag is taken from the last byte AFTER the repair (a repaired terminator then hides the rule).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import label_model as LM                                               # noqa: E402
import repair_corpus as RC                                             # noqa: E402
from test_lean_framing_model import St, decode_acars, TXT, ETX, ETB, DLE, MAXPERR     # noqa: E402

BLOCK_FIELDS = ("blocks", "too_short", "parity_many", "parity_blocks", "parity_errs", "crc_errors", "unfixable", "fixed",
                "parity_problem", "kept", "miss_txt_end")
FILTER_FIELDS = ("uplink_dropped", "label_dropped", "empty_dropped", "delivered")
FRAMING_FIELDS = ("txt_parity_resets", "too_long")                    # the reference's two framing lines: modelled, not in the table
COUNTERS = BLOCK_FIELDS + FILTER_FIELDS                                # the table's 32-bit counters, in the record's order


def new_row():
    r = dict.fromkeys(COUNTERS + FRAMING_FIELDS, 0)
    r["last_end_sample"] = -1
    r["ratios"] = []                                                   # MskLvlSum / MskBitCount of the kept blocks (where known)
    return r


def block_outcome(raw, mutate=None):
    """acars.c:120-209 on a raw block (len, text, crc0, crc1): dict(reason, pn (the k of "parity error(s): k", 0 = no line),
    crc_err, fixed, del_rule, txt (what outputmsg() receives | None))"""
    ln, txt = raw[0], bytes(raw[1])
    m = RC.model_blk(*raw)
    # acars.c:319-332: a block queued by ETX / ETB ends in it AS RECEIVED, a block queued by the DEL rule never does
    del_rule = ln > 0 and txt[ln - 1] not in (RC.ETXP, RC.ETBP)
    if mutate == "del_after_repair" and m["kept"]:
        del_rule = m["txt"][ln - 1] not in (RC.ETXP & 0x7F, RC.ETBP & 0x7F)
    out = dict(reason=None, pn=0, crc_err=False, fixed=False, del_rule=del_rule, txt=None)
    if ln < 13:
        out["reason"] = "too_short"
        return out
    t = bytearray(txt[:ln])
    t[12] = (t[12] & (RC.ETXP | RC.STXP)) | (RC.ETXP & RC.STXP)
    pn = sum(1 for b in t if RC.popc(b) & 1 == 0)
    if pn > RC.MAXPERR:
        out["reason"] = "parity_many"
        return out
    out["pn"], crc = pn, m["crc"]
    out["crc_err"] = crc != 0
    if m["kept"]:
        out["reason"], out["txt"] = "kept", m["txt"]
        searched = True
    else:
        # dropped behind the CRC: by a search that found nothing (acars.c:171-187) or by the second parity check (acars.c:202)
        found = bool(RC.prerr_candidates(ln, crc, m["pr"])) if pn else (bool(RC.dberr_candidates(ln, crc)) if crc else True)
        out["reason"] = "parity_problem" if found else "unfixable"
        searched = found
    ran = pn > 0 or crc != 0                                           # a search ran (acars.c:170, 182) ...
    if mutate == "fixed_needs_crc":
        ran = crc != 0
    out["fixed"] = searched and ran                                    # ... and succeeded: "errors fixed" (acars.c:178, 190)
    return out


def split(txt):
    """outputmsg()'s field split (output.c:486-568, the build without libacars) of a processed block: (down, label, text)"""
    ln = len(txt)
    label = bytes([txt[9], 0x64 if txt[10] == 0x7F else txt[10]])
    down = 0x30 <= txt[11] <= 0x39
    k, tl = 13, 0
    if txt[12] != 0x03:
        if down:
            for _ in range(4):
                if k < ln - 1:
                    k += 1
            for _ in range(6):
                if k < ln - 1:
                    k += 1
        tl = max(ln - k - 1, 0)
    return down, label, bytes(txt[k:k + tl])


def first_filter(txt, flt, mutate=None):
    """which of -A, -b, -e (in the reference's order: output.c:537, 539, 650) drops the processed block, or None.  flt:
    dict(downlink_only, skip_empty, labels) as label_model.keep takes them"""
    if not flt:
        return None
    down, label, body = split(txt)
    hits = []
    if flt.get("downlink_only") and not LM.keep(down, label, body, len(body), downlink_only=True):
        hits.append("uplink_dropped")
    if flt.get("labels") and not LM.keep(down, label, body, len(body), labels=flt["labels"]):
        hits.append("label_dropped")
    if flt.get("skip_empty") and not LM.keep(down, label, body, len(body), skip_empty=True):
        hits.append("empty_dropped")
    if not hits:
        return None
    return hits[-1] if mutate == "last_filter" else hits[0]


def count_block(row, raw, flt=None, entry="msgs", end_sample=None, ratio=None, mutate=None):
    """one consumed block into a channel's row.  entry: "msgs" (a message entry point: the filter fields move) or "frames"."""
    o = block_outcome(raw, mutate)
    row["blocks"] += 1
    row["miss_txt_end"] += o["del_rule"]
    if o["reason"] in ("too_short", "parity_many"):
        row[o["reason"]] += 1
        return o
    if o["pn"]:
        row["parity_blocks"] += 1
        row["parity_errs"] += o["pn"]
    row["crc_errors"] += o["crc_err"]
    row["fixed"] += o["fixed"]
    row[o["reason"]] += 1
    if o["reason"] != "kept":
        return o
    if end_sample is not None:
        row["last_end_sample"] = max(row["last_end_sample"], int(end_sample))
    if ratio is not None:
        row["ratios"].append(ratio)
    hit = first_filter(o["txt"], flt, mutate) if entry == "msgs" else None
    row[hit or "delivered"] += 1
    return o


def framing_events(frame, tail=RC.TAIL, st=None):
    """the framing machine (msk.c:53-63, acars.c:246-375) over a transmission's bits: (txt_parity_resets, too_long, blocks put
    [(len, text, crc0, crc1)]).  The two resets are told apart by the state the machine is in when the byte arrives."""
    from acarsdec_amd import synth as S
    st = st or St()
    bits = S.frame_bits(frame, tail=tail)
    par = lng = 0
    for i in range(len(bits)):
        b = int(bits[i]) ^ (st.S >> 1 & 1)
        st.outbits = ((st.outbits >> 1) & 0x7F) | (0x80 if b else 0)
        st.nbits -= 1
        if st.nbits <= 0:
            if st.astate == TXT:
                r = st.outbits & 0xFF
                if RC.popc(r) & 1 == 0 and st.berr + 1 > MAXPERR + 1:                     # acars.c:310
                    par += 1
                elif r not in (ETX, ETB) and not (st.blen + 1 > 20 and r == DLE) and st.blen + 1 > 240:   # acars.c:334
                    lng += 1
            decode_acars(st, i)
    return par, lng, [(b[1], b[5], b[3], b[4]) for b in st.blocks]


def check_identities(row, msgs_only=True):
    assert row["blocks"] == row["too_short"] + row["parity_many"] + row["unfixable"] + row["parity_problem"] + row["kept"], row
    if msgs_only:
        assert row["kept"] == row["uplink_dropped"] + row["label_dropped"] + row["empty_dropped"] + row["delivered"], row


def corpus_rows(items, flt=None, entry="msgs", mutate=None, framing=True):
    """{channel: row} of repair_corpus items: every transmission's queued block (item.want_raw) through count_block, its bits
    through framing_events"""
    rows = {}
    for it in items:
        row = rows.setdefault(it.chn, new_row())
        if it.want_raw is not None:
            count_block(row, it.want_raw, flt, entry, mutate=mutate)
        if framing:
            par, lng, _ = framing_events(it.frame)
            row["txt_parity_resets"] += par
            row["too_long"] += lng
    return rows


# ------------------------------------------------------------------------------------ the recording of tests/golden/stats_golden.json
NS = 7 * RC.CALL                                                       # samples per channel: the corpus's five calls and > 1 s of bare carrier
PCM_SCALE = 32767                                                      # int16 = rint(envelope * PCM_SCALE); a 12.5 kHz front end reads it / 32768


def to_pcm(x):
    import numpy as np
    return np.rint(np.clip(np.asarray(x, dtype=np.float64), 0.0, 1.0) * PCM_SCALE).astype(np.int16)


def corpus_pcm(items, channels):
    """int16 [len(channels), NS]: the corpus audio of the given channels, bare carrier behind it"""
    import numpy as np
    x = np.full((len(channels), NS), RC.CARRIER, dtype=np.float32)
    x[:, :RC.NSAMP] = RC.audio(items, channels)
    return to_pcm(x)


def extra_pcm(frames, phases):
    """int16 [len(frames), NS]: one crafted transmission per channel, RC.LEAD samples of carrier in front of it"""
    import numpy as np
    from acarsdec_amd import synth as S
    x = np.full((len(frames), NS), RC.CARRIER, dtype=np.float32)
    for r, (fr, ph) in enumerate(zip(frames, phases)):
        a = S.envelope(S.msk_audio(S.frame_bits(bytes(fr), tail=RC.TAIL), phase0=float(ph)))
        x[r, RC.LEAD:RC.LEAD + len(a)] = a
    return to_pcm(x)


def golden_pcm(g, items=None):
    """(pcm int16 [rows, NS] in the order of g["rows"], its SHA-256) of a stats_golden.json"""
    import hashlib
    import numpy as np
    if items is None:
        items, _ = RC.corpus(g["seed"])
    chans = [r["chn"] for r in g["rows"] if r["chn"] is not None]
    ext = [r for r in g["rows"] if r["chn"] is None]
    pcm = np.concatenate([corpus_pcm(items, chans), extra_pcm([bytes.fromhex(r["frame"]) for r in ext], [r["phase"] for r in ext])])
    return pcm, hashlib.sha256(np.ascontiguousarray(pcm).tobytes()).hexdigest()


def golden_model_rows(g, items=None, mutate=None, flt=None, entry="msgs"):
    """the model's row for every row of the golden, in its order"""
    if items is None:
        items, _ = RC.corpus(g["seed"])
    by = RC.by_channel(items)
    out = []
    for r in g["rows"]:
        if r["chn"] is not None:
            out.append(corpus_rows(by[r["chn"]], flt, entry, mutate)[r["chn"]])
            continue
        row = new_row()
        par, lng, blocks = framing_events(bytes.fromhex(r["frame"]))
        row["txt_parity_resets"], row["too_long"] = par, lng
        for raw in blocks:
            count_block(row, raw, flt, entry, mutate=mutate)
        out.append(row)
    return out
