"""The statistics table's rules (tests/stats_model.py) against the reference's own words, CPU legs:

  * tests/golden/stats_golden.json -- the -v lines of the UNMODIFIED reference program on channels of the repair corpus and three
    crafted transmissions, counted per channel (tests/golden/make_stats_golden.py): the model gives every count, after the audio
    has been regenerated and its hash checked;
  * tests/golden/msgjson_golden.json -- the lines the reference prints under every filter variant: the model's `delivered` per
    channel is the number of lines, its `kept` the unfiltered variant's, and what it charges to -A / -b / -e is what each
    filter drops when it is the first to see the block;
  * the framing's two resets (not in the table) are the reference's lines as well;
  * three deliberately wrong models are caught by those fixtures;
  * the Python helpers that read a table (dB, the scan report)."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
import label_model as LM
import repair_corpus as RC
import stats_model as SM


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "stats_golden.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def msgjson():
    with open(os.path.join(GOLDEN, "msgjson_golden.json")) as f:
        return json.load(f)


GOLDEN_FIELDS = tuple(k for k in SM.BLOCK_FIELDS if k != "kept") + SM.FRAMING_FIELDS


def as_counts(row):
    return {k: row[k] for k in GOLDEN_FIELDS}


def test_golden_recording_regenerates_bit_for_bit(golden):
    pcm, sha = SM.golden_pcm(golden)
    assert pcm.shape == (len(golden["rows"]), golden["nsamp"]) and pcm.dtype == np.int16
    assert sha == golden["pcm_sha256"]


def test_golden_reaches_every_counter_the_reference_can_reach(golden):
    rows = [r["counts"] for r in golden["rows"]]
    for k in GOLDEN_FIELDS:
        n = sum(1 for r in rows if r[k])
        assert n >= 2 or k == "parity_problem" and n == 0 or k == "too_long" and n == 1, k
    assert all(r["put"] == r["blocks"] for r in rows)                  # nothing was still queued when the file ended
    assert sum(1 for r in rows if r["fixed"] and not r["crc_errors"]) >= 2
    items, _ = RC.corpus(golden["seed"])
    bad = {it.chn for it in items if RC.reads_row_242(it)}
    assert not bad & {r["chn"] for r in golden["rows"]}


def test_model_counts_what_the_reference_prints(golden):
    rows = SM.golden_model_rows(golden)
    for g, m in zip(golden["rows"], rows):
        assert as_counts(m) == {k: g["counts"][k] for k in GOLDEN_FIELDS}, (g["chn"], g["what"])
        SM.check_identities(m)
        # kept is no line of its own: what was taken off the queue and not dropped reached outputmsg()
        c = g["counts"]
        assert m["kept"] == c["blocks"] - c["too_short"] - c["parity_many"] - c["unfixable"] - c["parity_problem"]
        assert m["delivered"] == m["kept"]


def variant_filter(g, name):
    return dict(downlink_only="A" in name, skip_empty="e" in name, labels=LM.parse_label_filter(g["label_list"]) if "b" in name else ())


def msgjson_rows(g, name, mutate=None):
    rows = [SM.new_row() for _ in range(g["nch"])]
    flt = variant_filter(g, name) if name != "none" else None
    for t in g["sent"]:
        SM.count_block(rows[t["chn"]], RC.block_of(bytes.fromhex(t["frame"])), flt, mutate=mutate)
    return rows


def lines_per_channel(g, name):
    n = [0] * g["nch"]
    for ln in g["variants"][name]["lines"]:
        n[json.loads(ln)["channel"]] += 1
    return n


def test_filter_fields_match_the_references_lines_under_every_variant(msgjson):
    none = lines_per_channel(msgjson, "none")
    for name in msgjson["variants"]:
        rows = msgjson_rows(msgjson, name)
        assert [r["delivered"] for r in rows] == lines_per_channel(msgjson, name), name
        assert [r["kept"] for r in rows] == none, name
        for r in rows:
            SM.check_identities(r)
    # a filter that is the first to see a block drops what it drops when it is alone: -A in "A" and "Aeb", -b in "b", -e in "e"
    alone = {k: [a - b for a, b in zip(none, lines_per_channel(msgjson, k))] for k in ("A", "b", "e")}
    assert [r["uplink_dropped"] for r in msgjson_rows(msgjson, "A")] == alone["A"]
    assert [r["label_dropped"] for r in msgjson_rows(msgjson, "b")] == alone["b"]
    assert [r["empty_dropped"] for r in msgjson_rows(msgjson, "e")] == alone["e"]
    assert [r["uplink_dropped"] for r in msgjson_rows(msgjson, "Aeb")] == alone["A"] and sum(alone["A"]) >= 5


def test_wrong_model_that_charges_the_last_filter_is_caught(msgjson):
    none, a = lines_per_channel(msgjson, "none"), lines_per_channel(msgjson, "A")
    rows = msgjson_rows(msgjson, "Aeb", mutate="last_filter")
    assert [r["delivered"] for r in rows] == lines_per_channel(msgjson, "Aeb")          # (the total does not tell) ...
    assert [r["uplink_dropped"] for r in rows] != [x - y for x, y in zip(none, a)]      # ... what -A drops on its own does


def test_wrong_model_that_wants_a_crc_error_for_fixed_is_caught(golden):
    rows = SM.golden_model_rows(golden, mutate="fixed_needs_crc")
    bad = [g["what"] for g, m in zip(golden["rows"], rows) if m["fixed"] != g["counts"]["fixed"]]
    assert len(bad) >= 2 and set(bad) == {"three parity errors, clean CRC, repaired"}


def test_wrong_model_that_takes_the_del_flag_after_the_repair_is_caught(golden):
    rows = SM.golden_model_rows(golden, mutate="del_after_repair")
    assert any(m["miss_txt_end"] != g["counts"]["miss_txt_end"] for g, m in zip(golden["rows"], rows))


def test_level_db_and_scan_report_read_a_table():
    from acarsdec_amd import _capi as K
    from acarsdec_amd import decoder as D
    import math
    st = np.zeros(4, dtype=K.CHAN_STATS_DTYPE)
    assert st.dtype.itemsize == 88
    st["lvl_min"], st["lvl_max"] = [0.0, 1.0, 3.5e-3, 250.0], [0.0, 10.0, 3.5e-3, 1e4]
    lo, hi = D.stats_level_db(st)
    assert lo.dtype == np.float32 and lo[0] == -np.inf and hi[0] == -np.inf and lo[1] == 0 and hi[1] == 10 and hi[3] == 40
    assert lo[2] == np.float32(10 * math.log10(3.5e-3))               # acars.c:351: double arithmetic narrowed to float
    st["delivered"], st["kept"], st["blocks"] = [3, 9, 3, 0], [4, 9, 5, 0], [6, 9, 5, 2]
    rep = D.scan_report(st, [131525000, 131725000, 131825000, 131550000])
    assert rep == [(131725000, 9, 9, 9), (131825000, 3, 5, 5), (131525000, 3, 4, 6), (131550000, 0, 0, 2)]
