"""The premises of tests/test_gpu_reasm_pressure.py, proven with the model alone (tests/reasm_table_model.py, tests/reasm_model.py):
the key words and the hash restatement, same_home() finds what it says, and for every scenario the homes, the entries that bar a
claim plus the new keys of each call, distinct (end_sample, chn) and blocks shorter than BLOCK_SAMPLES.  Premises, not measurements:
a scenario that misses one gets other numbers, never a weaker premise.  No GPU."""
import collections
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reasm_cases as RC  # noqa: E402
import reasm_model as RM  # noqa: E402
import reasm_table_model as T  # noqa: E402


def common_premises(sc):
    """what every scenario keeps: distinct (end_sample, chn), blocks shorter than BLOCK_SAMPLES, the reclaiming model and the plain
    one agree (so reasm_model.run is the expectation whatever slot an expired entry lost)"""
    assert sum(sc.batches) == len(sc.msgs)
    assert len({(m.end_sample, m.chn) for m in sc.msgs}) == len(sc.msgs)
    assert all(0 < m.end_sample - m.soh_sample < RC.BLOCK_SAMPLES for m in sc.msgs)
    assert T.expect(sc.msgs, sc.batches, sc.lost) == T.expect(sc.msgs, sc.batches, sc.lost, reclaim=True)


# ---- key words, hash, same_home ----------------------------------------------------------------------------------------------------
def test_key_words_are_c_strings_with_the_label_split_over_both():
    k0, k1 = T.key_words(b"N123AB", b"H1", b"M01", True)
    assert k0 == int.from_bytes(b"N123AB", "little") | ord("H") << 56 and k1 == ord("1") | int.from_bytes(b"M01", "little") << 8 | 1 << 63
    assert T.key_words(b"N123AB\0", b"H1\0", b"M01A", True) == (k0, k1)                  # the 8th, 3rd and 4th byte do not count
    assert T.key_words(b"N1\0XYZW", b"H1", b"M\0Z", True) == T.key_words(b"N1", b"H1", b"M", True)   # nothing behind a NUL does
    assert T.key_words(b"ABCDEFGH", b"H1", b"", False) == (int.from_bytes(b"ABCDEFG", "little") | ord("H") << 56, ord("1") | 1 << 63)
    assert T.key_words(b"N123AB", b"H1", b"M01", False)[1] == ord("1") | 1 << 63          # an uplink's key holds no msn
    assert T.key_words(b"", b"", b"", True) == (0, 1 << 63)
    assert T.key_words(b"N123AB", b"\0Z", b"M01", True) == T.key_words(b"N123AB", b"", b"M01", True)
    # the words of a record are those of its fields, and two keys of the model are equal exactly when their words are
    msgs = RC.one_field_keys()
    for m in msgs:
        assert T.key_words_of(m) == T.key_words(RM.raw(m, "addr", 7), RM.raw(m, "label", 2), RM.raw(m, "no", 3), RM._c(m.down) != 0)
    assert len({T.key_words_of(m) for m in msgs}) == len({RM.key_of(m) for m in msgs}) == 11
    assert len({(T.key_words_of(m), RM.key_of(m)) for m in msgs}) == 11


def test_hash_mixes_both_words():
    assert T.rs_hash(0, 0) == 0
    base = T.key_words(b"S00000", b"H1", b"K00", True)
    for w in (0, 1):
        flips = []
        for b in range(63):
            k = list(base)
            k[w] ^= 1 << b
            flips.append(bin(T.rs_hash(*base) ^ T.rs_hash(*k)).count("1"))
        assert min(flips) >= 5 and 14 <= sum(flips) / 63.0 <= 18, (w, flips)


@pytest.mark.parametrize("cap", [128, 256])
def test_home_is_spread_evenly(cap):
    """100 000 enumerated keys over cap homes: every home's count within 5 standard deviations of a Poisson count of the mean, so
    same_home() finds about 100 000 / cap keys per prefix character for ANY home"""
    count = collections.Counter(x & (cap - 1) for x in T._hashes(ord("S")))
    mean = 100000.0 / cap
    assert len(count) == cap
    lo, hi = min(count.values()), max(count.values())
    print("cap %d: %d .. %d per home, mean %.1f" % (cap, lo, hi, mean))
    assert mean - 5 * mean ** 0.5 <= lo and hi <= mean + 5 * mean ** 0.5


@pytest.mark.parametrize("cap", [128, 256, 1024])
def test_same_home_returns_keys_of_that_home_of_both_kinds(cap):
    for h in (0, cap // 2 - 12, cap - 5):
        S = T.same_home(cap, h, 129)
        assert len({(k.addr, k.label, k.msn) for k in S}) == 129 and all(T.home(T.words(k), cap) == h for k in S)
        assert 20 <= sum(k.up for k in S) <= 50                                          # every fourth, roughly
        assert all(not k.up for k in T.same_home(cap, h, 40, kinds="down")) and all(k.up for k in T.same_home(cap, h, 20, kinds="up"))
        # as the record carries them, and as the model keys them
        for n, k in enumerate(S[:12]):
            m = T.block(k, 0, False, 5000, n, b"x")
            assert T.home(T.key_words_of(m), cap) == h
            assert RM.key_of(m) == (k.addr, k.label, k.msn) and RM.creates(m)
            assert T.key_words_of(T.block(k, 1, True, 9000, n, b"")) == T.key_words_of(m)
    with pytest.raises(ValueError):
        T.same_home(cap, 1, 100000, b"S")


def test_no_slot_status_is_the_walk_without_an_entry():
    k, u = T.make_key(ord("S"), 0), T.make_key(ord("S"), 3)
    assert not k.up and u.up
    assert T.no_slot_status(T.block(k, 0, False, 5000, 0, b"x")) == RM.UNKNOWN and T.no_slot_status(T.block(u, 4, False, 5000, 0, b"x")) == RM.UNKNOWN
    assert T.no_slot_status(T.block(k, 1, False, 5000, 0, b"x")) == RM.OUT_OF_SEQUENCE
    assert T.no_slot_status(T.block(k, 0, True, 5000, 0, b"x")) == T.no_slot_status(T.block(u, 1, True, 5000, 0, b"x")) == RM.SKIPPED
    # where the block creates nothing it is what the model says of a block without an entry
    for m in (T.block(k, 1, False, 5000, 0, b"x"), T.block(k, 0, True, 5000, 0, b"x"), T.block(u, 1, True, 5000, 0, b"x")):
        assert RM.Table().add(m) == T.no_slot_status(m) and not RM.creates(m)


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
def test_expiry_takeover_turns_on_one_sample():
    sc = T.expiry_takeover()
    assert T.expiry_takeover() is sc                                                      # computed once, shared
    common_premises(sc)
    n = sc.note
    one = lambda name: sc.msgs[n[name][0]]
    old = sc.keys["old"]
    assert sc.cap == 128 == T.RS_PROBE                                                    # one window: homes do not matter here
    assert sum(k.up for k in old) == 28 and len({(k.addr, k.label, k.msn) for k in old}) == 128
    fill = [sc.msgs[i] for i in n["fill"]]
    assert len({m.soh_sample for m in fill}) == 128
    first = {RM.key_of(m): m.soh_sample for m in fill}
    up_first = min(first[(k.addr, k.label, k.msn)] for k in old if k.up)
    down_first = min(first[(k.addr, k.label, k.msn)] for k in old if not k.up)
    # the lone final blocks stand exactly at first + time-out + 2 s and one sample behind it, and are no creating events
    assert one("up_at").soh_sample == up_first + T.S90 + T.S2 and one("up_past").soh_sample == one("up_at").soh_sample + 1
    assert one("down_at").soh_sample == down_first + T.S660 + T.S2 and one("down_past").soh_sample == one("down_at").soh_sample + 1
    for name in ("up_at", "up_past", "up_all", "down_at", "down_past", "all"):
        m = one(name)
        assert not RM.creates(m) and RM._c(m.bs) != RM.ETX and RM._c(m.bid) != 0 and RM.Table().add(m) == RM.SKIPPED
    # G after each call is the largest SOH so far, and moves only with those blocks: every other record of the steps lies below
    G, at, moved = None, 0, []
    for b, size in enumerate(sc.batches):
        top = max(m.soh_sample for m in sc.msgs[at:at + size])
        if G is None or top > G:
            G = top
            moved.append(b)
        at += size
    names = {i: name for name, idx in n.items() for i in idx}
    starts = [sum(sc.batches[:b]) for b in moved]
    assert [names[s] for s in starts] == ["fill", "up_at", "up_past", "up_all", "down_at", "down_past", "all", "last_done", "old_b", "old_c"]
    # the table as a claim sees it, call by call
    occ = T.occupancy(sc.msgs, sc.batches, sc.lost)
    call_of = {}
    at = 0
    for b, size in enumerate(sc.batches):
        for i in range(at, at + size):
            call_of[i] = b
        at += size
    by = lambda name: occ[call_of[n[name][0]]]
    for tag in ("up", "down"):
        assert by(tag + "_full") == by(tag + "_still") == by(tag + "_fullagain") == (128, 0, 1)      # nothing to take: UNKNOWN
        assert by(tag + "_takes") == (127, 1, 0)                                         # exactly one slot became claimable
        assert by(tag + "_done") == (128, 0, 0) and by(tag + "_idle") == (127, 1, 0)
    assert by("fillers") == (101, 27, 0) and by("last") == (0, 127, 0) and by("old_b") == (0, 28, 0)
    assert all(live + new <= 128 for live, new, _ in occ) and all(live == 128 for live, _, gone in occ if gone)
    assert sorted(sc.lost) == sorted(n[t + s][0] for t in ("up", "down") for s in ("_full", "_still", "_fullagain"))
    # what the model says of it
    status, done, dropped = T.expect(sc.msgs, sc.batches, sc.lost)
    assert dropped == 6 and all(status[i] == RM.UNKNOWN for i in sc.lost)
    for name in ("fill", "fillers", "last", "up_takes", "down_takes", "up_idle", "down_idle"):
        assert all(status[i] == RM.IN_PROGRESS for i in n[name]), name
    assert all(status[i] == RM.COMPLETE for i in n["last_done"] + n["up_done"] + n["down_done"])
    up_keys = {(k.addr, k.label, k.msn) for k in old if k.up}
    for i in n["old_b"]:
        assert status[i] == (RM.IN_PROGRESS if RM.key_of(sc.msgs[i]) in up_keys else RM.OUT_OF_SEQUENCE)
    for i in n["old_c"]:
        assert status[i] == (RM.COMPLETE if RM.key_of(sc.msgs[i]) in up_keys else RM.OUT_OF_SEQUENCE)
    assert len(done) == 2 + 127 + 28
    # the restarted uplink chains hold their B and C blocks only; the seam: rows of every length mod 4 change hands
    text_of = {i: RM.msg_text(m) for i, m in enumerate(sc.msgs)}
    b_of = {RM.key_of(sc.msgs[i]): text_of[i] for i in n["old_b"]}
    c_of = {RM.key_of(sc.msgs[i]): text_of[i] for i in n["old_c"]}
    assert sorted(d[-1] for d in done[-28:]) == sorted(b_of[k] + c_of[k] for k in up_keys)
    assert {len(text_of[i]) for i in n["fill"]} == {1, 2, 3, 5} and {len(d[-1]) % 4 for d in done} == {0, 1, 2, 3}


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [100, 256 - 5], ids=["middle", "wraps"])
def test_probe_window_is_full_with_half_the_table_free(h):
    sc = T.probe_window(h)
    common_premises(sc)
    S, n = sc.keys["S"], sc.note
    assert sc.cap == 256 and len({(k.addr, k.label, k.msn) for k in S}) == 129 and all(T.home(T.words(k), 256) == h for k in S)
    assert {k.up for k in S[:128]} == {False, True}
    assert (h + T.RS_PROBE - 1 >= 256) == (h == 251)                                      # the window runs round the table's end, or not
    assert T.home(T.words(sc.keys["plus"]), 256) == (h + 1) % 256 and T.home(T.words(sc.keys["minus"]), 256) == h - 1
    assert all(T.home(T.key_words_of(sc.msgs[i]), 256) == h for i in n["fill"] + n["129th"] + n["finals"] + n["129th_again"])
    # 128 claims for the 128 slots of one window in one pass; then the window holds 128 live entries and the table 128 free slots
    occ = T.occupancy(sc.msgs, sc.batches, sc.lost)
    assert occ == [(0, 128, 0), (128, 0, 1), (128, 2, 0), (130, 0, 0), (2, 1, 0), (3, 0, 0)]
    status, done, dropped = T.expect(sc.msgs, sc.batches, sc.lost)
    assert dropped == 1 and sc.lost == n["129th"] and status[n["129th"][0]] == RM.UNKNOWN
    assert all(status[i] == RM.IN_PROGRESS for i in n["fill"] + n["neighbours"] + n["129th_again"])
    assert all(status[i] == RM.COMPLETE for i in n["finals"] + n["rest"]) and len(done) == 131
    # left in, the 129th would be in progress from its first block on: the two expectations differ
    assert T.expect(sc.msgs, sc.batches, [])[0][n["129th"][0]] == RM.IN_PROGRESS


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------
def test_racing_claims_have_28_slots_for_40():
    sc = T.racing_claims()
    common_premises(sc)
    n = sc.note
    assert sc.cap == 128 and sc.batches == [100, 40, 140] and sc.lost == []
    new = sc.keys["new"]
    assert len(new) == 40 and not any(k.up for k in new) and {k.up for k in sc.keys["old"]} == {False, True}
    assert len({(k.addr, k.label, k.msn) for k in new + sc.keys["old"]}) == 140
    assert T.occupancy(sc.msgs, sc.batches, [])[:2] == [(0, 100, 0), (100, 40, 0)]         # 28 free slots, 40 claims
    # whichever 12 lose: their first blocks are UNKNOWN, their final blocks OUT_OF_SEQUENCE, everybody else completes
    rng = __import__("random").Random(5)
    for _ in range(3):
        losers = rng.sample(n["new"], 12)
        status, done, dropped = T.expect(sc.msgs, sc.batches, losers)
        gone = {RM.key_of(sc.msgs[i]) for i in losers}
        assert dropped == 12 and [status[i] for i in n["new"]].count(RM.IN_PROGRESS) == 28
        assert all(status[i] == (RM.OUT_OF_SEQUENCE if RM.key_of(sc.msgs[i]) in gone else RM.COMPLETE) for i in n["finals"])
        assert len(done) == 128 and T.occupancy(sc.msgs, sc.batches, losers)[1] == (100, 28, 12)
        ends = [(d[3], d[0]) for d in done]
        assert ends == sorted(ends)


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------
def test_large_index_traffic_straddles_2_32_in_one_call():
    msgs, batches = T.large_index_traffic()
    assert len(msgs) == 20000 and max(batches) <= 2000 and sum(batches) == len(msgs)
    assert sorted(bytes(m) for m in msgs) == sorted(bytes(m) for m in RC.random_traffic())
    cross = T.straddles(msgs, batches, T.OFFSETS[0])
    assert len(cross) == 1 and batches[cross[0]] > 1
    assert all(0 < m.end_sample + T.OFFSETS[1] < 1 << 43 for m in msgs) and min(m.end_sample for m in msgs) + T.OFFSETS[1] >= 1 << 42
    assert not T.straddles(msgs, batches, 0)
    # the model does not care where the samples are counted from, with t0 moved back to match
    plain = RM.run(msgs, batches, t0_us=T.T0_US)
    for off in T.OFFSETS:
        (sec, usec), us = T.t0_before(off)
        assert sec * 10**6 + usec == us == T.T0_US - 80 * off and 0 <= usec < 10**6 and sec > 10**9
        sh = RM.run(T.shifted(msgs, off), batches, t0_us=us)
        assert sh[0] == plain[0] and RC.completed_tuples(sh[1]) == T.shifted_done(RC.completed_tuples(plain[1]), off)
    # and nobody can be dropped in these calls either
    assert max(RM.run(msgs, batches, t0_us=T.T0_US, reclaim=True)[2]) <= T.RS_PROBE - 1
