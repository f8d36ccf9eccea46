"""The block repair on long blocks and order-sensitive fixes, CPU legs (tests/repair_corpus.py has the corpus and the Python
model; tests/test_gpu_repair.py runs the same corpus on the device):

  * the oracle's demodulator queues exactly the crafted blocks, so the categories below really reach the repair;
  * orc_blk_process == the Python restatement of acars.c:39-90 + 123-207, block for block (kept / dropped, err, text), nothing
    left out -- 241-byte blocks that read syndrome row 242 included (the oracle has that row by the table's recurrence);
  * the real blk_thread on the same audio == the oracle, drops included; left out of this leg only: the blocks whose search
    reads row 242, where the reference reads past its table (all of them 241 bytes long, under 3 % of the corpus);
  * the corpus holds what it is meant to hold, counted from what was queued and delivered.

Counts of the committed seed (`pytest -s` on this file prints them; python -m tests.repair_corpus the generator's side):
  1722 transmissions on 1024 channels; 1696 blocks queued, 1603 delivered, 93 dropped (11 of them shorter than 13 bytes); 26
  transmissions queue nothing (8 x ETX at byte 12 damaged, 18 x five parity errors); clean at every length 13 .. 241; one parity
  error at 240 + 130 indices, all eight bits; byte 12: 30 errors that vanish, 10 that are flagged; two / three parity errors:
  slot 0 35 / 42, one per slot 80 / 23, same lane 17 / 14, across a slot boundary 28 / 28, first and last byte 15 / 15; four: 18,
  dropped; two bits in a byte: 238 indices of a 240-byte block, 19 of a 241-byte block, 72 at slot boundaries of other lengths;
  the 16 CRC bits; parity + CRC bit 31 / 27; unrepairable 26 / 26 / 26, 18 of them accepted through a false candidate; 78 blocks
  ended by DEL; order-sensitive: fixprerr 66 blocks with >= 2 candidates (34 deliver another text than was sent, 30 with the first
  two in different 64-groups, 36 in the same group), fixdberr 58 (28, 58, 0: the code has no such pair inside 64 bytes); left out
  of the blk_thread leg: 23 blocks of 241 bytes (1.3 %).
"""
import collections
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from oracle import oracle as O
import repair_corpus as RC


def test_model_table_is_the_references_and_the_oracles():
    """the model's syndrome table: the reference's 1936 entries (syndrom.h:52-295, tests/golden/syndrom_table.npy) continued by
    their own recurrence to the 243 rows a 241-byte block needs; the oracle's table is the same 243 rows"""
    ref = np.load(os.path.join(GOLDEN, "syndrom_table.npy"))
    assert ref.size == 8 * 242 and [int(v) for v in ref] == RC.SYND[: 8 * 242]
    assert len(RC.SYND) == 8 * 243 == 8 * (241 + 2)
    assert [int(v) for v in O.syndrome_table(8 * 243)] == RC.SYND
    # two wrong bits in each of two text bytes with remainder 0: only at these byte distances, so never inside a 64-byte group
    far = {d for d in range(1, 241) if set(RC._PAIR_SY[2].tolist()) & set(RC._PAIR_SY[2 + d].tolist())}
    assert far == {142, 144, 208}
    # the defining property of a row: the remainder of one set bit with k bytes behind it
    for k in (0, 1, 2, 130, 241, 242):
        for bit in (0, 3, 7):
            assert O.crc_ccitt(bytes([1 << bit]) + bytes(k)) == RC.SYND[bit + 8 * k]


@functools.lru_cache(maxsize=1)
def oracle_run():
    """per item: (raw block as the oracle's demodulator queued it | None, oracle frame, processed frame | None)"""
    items, _ = RC.corpus()
    x = RC.audio(items)
    chans = RC.by_channel(items)
    res, stray = {}, []
    for c in range(RC.NCH):
        ch = O.Channel(c, max_frames=16)
        ch.demod(x[c])
        frames = ch.frames
        its = chans.get(c, [])
        # a block belongs to the slot its last bit fell into
        per = collections.defaultdict(list)
        for f in frames:
            per[int(f.end_sample) // RC.PERIOD].append(f)
        for it in its:
            fs = per.pop(it.slot, [])
            if len(fs) > 1:
                stray.append((c, it.slot, len(fs)))
            f = fs[0] if fs else None
            res[id(it)] = (RC.raw_tuple(f) if f is not None else None, f, O.blk_process(f) if f is not None else None)
        stray += [(c, s, len(v)) for s, v in per.items()]
    return items, res, stray


def test_oracle_queues_the_crafted_blocks():
    items, res, stray = oracle_run()
    assert not stray, stray[:5]
    wrong = [(it.tag, it.chn, it.slot) for it in items if res[id(it)][0] != it.want_raw]
    assert not wrong, (len(wrong), wrong[:8])
    for it in items:                                       # (and the framing model's block is the crafted one wherever damage is plain)
        if it.direct:
            assert it.want_raw == RC.block_of(it.frame)
    # the GPU leg needs passes with more blocks than waves: one wave per 8 channels, at least 128
    calls = collections.Counter(int(f.end_sample) // RC.CALL for _, f, _ in res.values() if f is not None)
    assert sum(1 for n in calls.values() if n > 2 * max(128, RC.NCH // 8)) >= 3, calls


def model_of(raw):
    return RC.model_blk(*raw)


def test_oracle_repair_is_the_python_model_on_every_block():
    items, res, _ = oracle_run()
    n = 0
    for it in items:
        raw, f, o = res[id(it)]
        if raw is None:
            continue
        m = model_of(raw)
        n += 1
        assert (o is not None) == m["kept"], (it.tag, raw[0])
        if o is not None:
            assert (int(o.err), bytes(o.txt[: o.len]), int(o.len), bytes(o.crc)) == (m["err"], m["txt"], raw[0], bytes(raw[2:])), (it.tag, raw[0])
        # the model took the first candidate of the full list, in the reference's order
        facts = RC.order_facts(raw, m)
        if facts:
            assert (facts[1] > 0) == m["kept"]
    assert n == sum(1 for it in items if it.want_raw is not None)       # nothing left out


def test_corpus_holds_what_it_is_meant_to_hold(capsys):
    items, res, _ = oracle_run()
    cats = collections.Counter()
    order = {"pr": [0, 0, 0, 0], "db": [0, 0, 0, 0]}
    left_out, queued, zoo = [], 0, collections.Counter()
    for it in items:
        raw, f, o = res[id(it)]
        out = (int(o.err), bytes(o.txt[: o.len])) if o is not None else None
        cs = RC.categorize(it, raw, out)
        cats.update(cs)
        if raw is None:
            continue
        queued += 1
        cats["delivered" if o is not None else "dropped"] += 1
        m = model_of(raw)
        if 242 in m["rows"]:
            left_out.append(raw[0])
        facts = RC.order_facts(raw, m)
        if facts and facts[1] >= 2 and "unrepairable-accepted" not in cs and "unrepairable-dropped" not in cs:
            order[facts[0]][0] += 1
            order[facts[0]][1] += "delivered-other-text" in cs
            order[facts[0]][2] += facts[2]
            order[facts[0]][3] += facts[3]
        if o is not None and raw[0] >= 100:
            s = O.msg_split(o)
            zoo["down" if s.down not in (b"\x00", 0) else "up"] += 1
            zoo["nak" if s.ack == b"!" else "ack"] += 1
            zoo["del-label"] += bytes(o.txt[10:11]) == b"\x7f"
            zoo["dots>1"] += bytes(o.txt[1:3]) == b".."
            zoo["etb"] += bytes(o.txt[o.len - 1:o.len]) == b"\x17"
    with capsys.disabled():
        print("\n%d transmissions, %d queued, left out of the blk_thread leg: %d" % (len(items), queued, len(left_out)))
        print(sorted((k, v) for k, v in cats.items() if ":" not in k or k.startswith("nothing")))
        print("order-sensitive [>= 2 candidates, other text delivered, first two in different groups, in the same group]:", order, "zoo:", dict(zoo))
    have = lambda fmt, rng: [i for i in rng if fmt % i not in cats]
    assert not have("clean-delivered:%d", range(13, 242))
    assert not have("p1@241:%d", range(240)) and not have("p1@130:%d", range(130)) and not have("p1-bit:%d", range(8))
    assert cats["byte12-vanishes-delivered"] >= 12 and cats["p1-byte12"] >= 4
    assert cats["nothing-queued:etx12"] == 8
    assert cats["nothing-queued:p5"] == sum(1 for it in items if it.tag == "p5") >= 12     # five parity errors: the framing resets
    assert cats["short"] >= 10
    for n in (2, 3):
        for k in ("slot0", "one-per-slot", "same-lane", "across-boundary", "first-and-last"):
            assert cats["p%d-%s" % (n, k)] >= 5, (n, k)
        assert cats["p%d-repaired" % n] >= 30
    assert cats["p4-dropped"] >= 12
    assert not have("db@240:%d", [i for i in range(239) if i != 12])
    assert sum(1 for k in cats if k.startswith("db@241:")) >= 15 and cats["db-boundary"] >= 20
    assert not have("crc-bit:%d", range(16))
    assert cats["p1+crc-bit"] >= 12 and cats["p2+crc-bit"] >= 12 and cats["p1+crc-bit-repaired"] >= 1
    for k in ("2x2", "3+1", "crc2"):
        assert cats["unrepairable-" + k] >= 20, k
    assert cats["unrepairable-accepted"] >= 10 and cats["unrepairable-dropped"] >= 30
    for k in ("pr", "db"):
        assert order[k][0] >= 30 and order[k][1] >= 10 and order[k][2] >= 10, (k, order[k])
    # competing candidates inside one 64-group (what tells find-first from find-last in a ballot): two per entry of the table of
    # code words that allow it, injected bit first and second; fixdberr has none by the code's structure (see same_group_table)
    assert order["pr"][3] >= 2 * len(RC.same_group_table()) >= 30 and order["db"][3] == 0
    assert cats["ended-by-del"] >= 16 and cats["etb"] >= 24 and cats["end-moved"] >= 2
    assert min(zoo[k] for k in ("down", "up", "nak", "ack", "dots>1", "etb")) >= 10 and zoo["del-label"] >= 5, zoo
    # what the leg against the real blk_thread leaves out: only 241-byte blocks, under 3 % of the corpus
    assert left_out and set(left_out) == {241} and len(left_out) <= 0.03 * len(items), len(left_out)


@pytest.mark.parametrize("fault", ["db_from_64", "last_hit", "slot0"])
def test_corpus_notices_what_a_wave_wide_search_could_get_wrong(fault):
    """the faults a 64-candidates-at-a-time search could have (fixdberr starting at its second group, find-last for find-first,
    the slot of a write-back forced to 0), applied to the Python model: the oracle disagrees on this corpus.  The slot fault is
    invisible on short blocks with random damage of the kind the other tests use, which is why this corpus exists"""
    items, res, _ = oracle_run()

    def disagreements(blocks):
        n = 0
        for raw, o in blocks:
            m = RC.model_blk(*raw, mutate=fault)
            n += (o is not None) != m["kept"] or (o is not None and bytes(o.txt[: o.len]) != m["txt"])
        return n
    assert disagreements([(raw, o) for raw, _, o in res.values() if raw is not None]) >= 5
    if fault != "slot0":
        return
    from acarsdec_amd import synth as S
    rng = np.random.default_rng(31337)
    kinds = [None, "p1", "p2", "p3", "db", "crc", "p4", "p1crc"]
    short = []
    for c in range(16):
        a, _ = S.channel_audio(rng, 48 * 1024, gap=(1200, 2500), text_len=(15, 50), corrupt=kinds[c % 8:] + kinds[:c % 8])
        ch = O.Channel(c, max_frames=512)
        ch.demod(S.envelope(a, noise=0.002, rng=rng))
        short += [(RC.raw_tuple(f), O.blk_process(f)) for f in ch.frames]
    assert len(short) >= 40
    assert disagreements(short) == 0


REF_CHILD = r'''
import sys, json
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
from oracle import oracle as O
import repair_corpus as RC
items, _ = RC.corpus()
# the transmissions whose block makes the search read syndrome row 242 are not played to the reference at all
left = [it for it in items if it.want_raw is not None and 242 in RC.model_blk(*it.want_raw)["rows"]]
items = [it for it in items if it.want_raw is None or 242 not in RC.model_blk(*it.want_raw)["rows"]]
ref = O.Ref()
G = 8
res = dict(nraw=0, nout=0, nitems=len(items), left_out=[it.want_raw[0] for it in left], raw_diff=[], out_diff=[])
def tup(f): return [int(f.len), int(f.err), bytes(f.crc).hex(), bytes(f.txt[:f.len]).hex(), float(f.lvl).hex()]
for c0 in range(0, RC.NCH, G):
    x = RC.audio(items, range(c0, c0 + G))
    ref.init_file(G)
    och = [O.Channel(r, max_frames=16) for r in range(G)]
    for r in range(G):
        for s in range(0, RC.NSAMP, 4096):
            ref.demod(r, x[r, s:s + 4096])
        och[r].demod(x[r])
    ref.drain()
    rraw = sorted([int(f.chn)] + tup(f) for f in ref.raw_frames())
    oraw = sorted([r] + tup(f) for r in range(G) for f in och[r].frames)
    if rraw != oraw: res["raw_diff"].append(c0)
    assert not any(242 in RC.model_blk(*RC.raw_tuple(f))["rows"] for r in range(G) for f in och[r].frames)
    mine = sorted([r] + tup(o) for r in range(G) for o in (O.blk_process(f) for f in och[r].frames) if o is not None)
    theirs = sorted([int(f.chn)] + tup(f) for f in ref.out_frames())
    if mine != theirs: res["out_diff"].append(c0)
    res["nraw"] += len(rraw); res["nout"] += len(theirs)
print(json.dumps(res))
'''


@pytest.mark.skipif(not O.ref_available(), reason="oracle/_ref not built (no reference tree)")
def test_real_blk_thread_delivers_what_the_oracle_delivers():
    """the UNMODIFIED blk_thread (acars.c:93-215) on the corpus audio: what it queues and what reaches outputmsg() is what the
    oracle queues and delivers, drops included -- except the blocks whose search reads syndrome row 242"""
    r = subprocess.run([sys.executable, "-c", REF_CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    items, mine, _ = oracle_run()
    assert not res["raw_diff"] and not res["out_diff"], res
    assert res["left_out"] and set(res["left_out"]) == {241} and len(res["left_out"]) <= 0.03 * len(items)
    assert res["nitems"] + len(res["left_out"]) == len(items)
    kept = [(raw, o) for raw, _, o in mine.values() if raw is not None and 242 not in RC.model_blk(*raw)["rows"]]
    assert res["nraw"] == len(kept) and res["nout"] == sum(1 for _, o in kept if o is not None) >= 1000
