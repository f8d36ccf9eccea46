"""Golden fixture for the per-channel statistics (acg_chan_stats): what the UNMODIFIED reference program says under -v about
channels of the block-repair corpus (tests/repair_corpus.py), counted per channel.

  * Channels are picked with the model (tests/stats_model.py) so that every block-level counter the reference can reach, "miss txt
    end" and the framing's "too many parity errors" are reached on at least two channels.  ("parity check problem", acars.c:203,
    cannot be reached: a search that succeeds leaves every byte with odd parity.)  Channels holding a block whose search reads
    syndrome row 242 are left out: the real blk_thread reads past its table there.
  * Crafted channels on top, one transmission each: a text of more than 240 bytes without a terminator ("too long", acars.c:336),
    and two blocks with three parity errors and a CLEAN CRC that fixprerr repairs all the same -- three wrong text bits and one
    wrong CRC bit that together are a code word -- the only way "errors fixed" is printed without "crc error" (acars.c:178).
  * The audio goes out as 12.5 kHz PCM16 WAV files of at most 16 channels (MAXNBCHANNELS), more than a second of bare carrier
    behind the last transmission (deinitAcars drops what is still queued at the end of the file), through
    oracle/_ref/acarsdec_cpu -v -o 0 -f <wav>; the lines on stderr are counted per channel.  Two threads share stderr, so
    only counts are kept, never order.  "too many parity errors: k" (blk_thread) and "too many parity errors" (decodeAcars) are
    different counters; for "parity error(s): k" the sum of k is kept as well.
  * Asserted here: "put message" == "get message" on every channel (else the tail was too short), the model agrees with every
    count, no class is empty.

The two framing lines ("too many parity errors" without a count, "too long") are kept although the table does not count them:
tests/stats_model.py models them and tests/test_stats_model.py holds that model to these counts.

The audio is not committed: the file holds the channel list, the corpus seed, the crafted transmissions and the SHA-256 of the PCM
that was fed (a test regenerates it).  A crafted transmission's carrier phase is drawn again until the reference's counts are the
model's -- also when its block thread merely had not finished at the end of the file -- so a re-run may settle on another phase (and
hash) with the same counts.  Run in the build container only:

    python tests/golden/make_stats_golden.py

Output (derived data, no reference source):
  stats_golden.json   {"seed", "nsamp", "pcm_scale", "pcm_sha256", "rows": [{"chn" | null, "what", "frame" (hex), "phase",
                       "counts": {line class: n}}]}
"""
import json
import os
import re
import subprocess
import sys
import tempfile
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from acarsdec_amd import synth as S  # noqa: E402
import repair_corpus as RC  # noqa: E402
import stats_model as SM  # noqa: E402

MAXNBCHANNELS = 16
TARGETS = ("too_short", "parity_many", "parity_blocks", "crc_errors", "unfixable", "fixed", "kept", "miss_txt_end", "txt_parity_resets")
LINES = [("blocks", r"get message #(\d+)"), ("put", r"put message #(\d+)"), ("too_short", r"#(\d+) too short"),
         ("parity_many", r"#(\d+) too many parity errors: (\d+)"), ("txt_parity_resets", r"#(\d+) too many parity errors"),
         ("parity_blocks", r"#(\d+) parity error\(s\): (\d+)"), ("crc_errors", r"#(\d+) crc error"),
         ("unfixable", r"#(\d+) not able to fix errors"), ("fixed", r"#(\d+) errors fixed"),
         ("parity_problem", r"#(\d+) parity check problem"), ("miss_txt_end", r"#(\d+) miss txt end"), ("too_long", r"#(\d+) too long")]
CLASSES = tuple(k for k, _ in LINES) + ("parity_errs",)


def pick_channels(items):
    rows = SM.corpus_rows(items)
    bad = {it.chn for it in items if RC.reads_row_242(it)}
    picked = []
    for k in TARGETS:
        have = [c for c in picked if rows[c][k]]
        for c in sorted(rows):
            if len(have) >= 2:
                break
            if c not in bad and c not in picked and rows[c][k]:
                picked.append(c)
                have.append(c)
        assert len(have) >= 2, k
    return sorted(picked)


def clean_crc_repairs(rng, n=2):
    """n transmissions whose block has three parity errors and a clean CRC that fixprerr repairs: (len, flips, crcflips) with
    damage syndrome 0 -- three text bits in three bytes and one CRC bit that form a code word"""
    out = []
    while len(out) < n:
        ln = int(rng.integers(40, 120))
        pos = [(i, b) for i in range(ln - 1) if i != 12 for b in range(8)]
        syn = {p: RC.SYND[p[1] + 8 * (ln - p[0] + 1)] for p in pos}
        pairs = {}
        for a in range(len(pos)):
            for b in range(a + 1, len(pos)):
                if pos[a][0] != pos[b][0]:
                    pairs.setdefault(syn[pos[a]] ^ syn[pos[b]], (pos[a], pos[b]))
        found = None
        for p in (pos[int(j)] for j in rng.permutation(len(pos))):
            for x in range(16):
                q = pairs.get(syn[p] ^ RC.SYND[x])
                if q and p[0] not in (q[0][0], q[1][0]):
                    found = (sorted([p, q[0], q[1]]), x)
                    break
            if found:
                break
        if not found:
            continue
        three, x = found
        flips, crcflips = [(i, 1 << b) for i, b in three], [(1 - (x >> 3), 1 << (x & 7))]
        assert RC.damage_syndrome(ln, flips, crcflips) == 0
        try:
            out.append(RC.make_item(rng, ln, "p3-clean-crc", flips, crcflips))
        except AssertionError:
            continue
    return out


def crafted(rng):
    """[(what, frame bytes)]"""
    head = bytes(S.odd_parity(b) for b in (ord("+"), ord("*"), S.SYN, S.SYN, S.SOH))
    long_text = head + bytes(S.odd_parity(b) for b in S.random_text(rng, 250, 250))
    out = [("a text of 250 bytes without a terminator", long_text)]
    for it in clean_crc_repairs(rng):
        o = SM.block_outcome(it.want_raw)
        assert o["pn"] == 3 and not o["crc_err"] and o["reason"] == "kept" and o["fixed"]
        out.append(("three parity errors, clean CRC, repaired", it.frame))
    return out


def run_reference(pcm):
    """the -v lines of one WAV file, counted: [per file channel: {class: n}]"""
    exe = os.path.join(ROOT, "oracle", "_ref", "acarsdec_cpu")
    assert pcm.shape[0] <= MAXNBCHANNELS
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "stats.wav")
        with wave.open(p, "wb") as w:
            w.setnchannels(pcm.shape[0])
            w.setsampwidth(2)
            w.setframerate(12500)
            w.writeframes(np.ascontiguousarray(pcm.T).tobytes())
        r = subprocess.run([exe, "-v", "-o", "0", "-f", p], capture_output=True)
    counts = [dict.fromkeys(CLASSES, 0) for _ in range(pcm.shape[0])]
    for ln in r.stderr.decode("latin1").split("\n"):
        for k, pat in LINES:
            m = re.fullmatch(pat, ln.strip())
            if m:
                c = counts[int(m.group(1)) - 1]
                c[k] += 1
                if k == "parity_blocks":
                    c["parity_errs"] += int(m.group(2))
                break
        else:
            assert not ln.startswith("#"), ln                         # a per-channel line this maker does not know
    return counts


def agrees(counts, row):
    return all(counts[k] == row[k] for k in CLASSES if k != "put") and counts["put"] == counts["blocks"]


if __name__ == "__main__":
    items, _ = RC.corpus()
    rng = np.random.default_rng(RC.SEED + 7)
    rows = []
    chans = pick_channels(items)
    model = SM.corpus_rows(items)
    for c0 in range(0, len(chans), MAXNBCHANNELS):
        part = chans[c0:c0 + MAXNBCHANNELS]
        for c, cnt in zip(part, run_reference(SM.corpus_pcm(items, part))):
            assert cnt["put"] == cnt["blocks"], (c, cnt)               # (else: the tail was too short)
            assert agrees(cnt, model[c]), (c, cnt, model[c])
            rows.append(dict(chn=c, what="corpus", frame=None, phase=None, counts=cnt))
    for what, frame in crafted(rng):
        par, lng, blocks = SM.framing_events(frame)
        want = SM.new_row()
        want["txt_parity_resets"], want["too_long"] = par, lng
        for raw in blocks:
            SM.count_block(want, raw)
        for _ in range(32):                                            # (the reference's loop does not lock onto every carrier phase)
            phase = float(rng.uniform(0, 2 * np.pi))
            cnt = run_reference(SM.extra_pcm([frame], [phase]))[0]
            if agrees(cnt, want):
                break
        else:
            raise AssertionError("never decoded as the model says: %s %r %r" % (what, cnt, want))
        rows.append(dict(chn=None, what=what, frame=frame.hex(), phase=phase, counts=cnt))
    g = dict(seed=RC.SEED, nsamp=SM.NS, pcm_scale=SM.PCM_SCALE, rows=rows)
    pcm, g["pcm_sha256"] = SM.golden_pcm(g, items)
    # the whole recording once more, in files of 16 channels as a test would lay it out: the counts must not depend on the file
    again = []
    for c0 in range(0, len(rows), MAXNBCHANNELS):
        again += run_reference(pcm[c0:c0 + MAXNBCHANNELS])
    assert again == [r["counts"] for r in rows]
    total = {k: sum(r["counts"][k] for r in rows) for k in CLASSES}
    for k in CLASSES:
        assert k == "parity_problem" or total[k] >= 2 or (k == "too_long" and total[k] >= 1), (k, total)
    assert sum(1 for r in rows if r["counts"]["fixed"] and not r["counts"]["crc_errors"]) >= 2
    with open(os.path.join(HERE, "stats_golden.json"), "w") as f:
        json.dump(g, f, indent=0)
    print("%d channels (%d crafted); totals %s" % (len(rows), sum(r["chn"] is None for r in rows), total))
