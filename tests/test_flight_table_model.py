"""The conditions on the inputs of tests/test_gpu_flight_pressure.py, proven with the list walk alone (tests/flight_table_model.py,
tests/flight_model.py): the hash restatement spreads and same_home() finds what it says, every traffic meets the condition its
GPU test rests on (nobody can be dropped / exactly these are dropped, so many live, taken over, returned), and expect_without()
with nothing dropped is the plain list walk.  Conditions, not measurements: a traffic that misses one gets another seed or
another rate, never a weaker condition."""
import collections

import pytest

import flight_model as FM
import flight_table_model as T

CAP = T.CAP


def entry(b):
    from acarsdec_amd import _capi as K
    return K.Flight.from_buffer_copy(b)


def by_addr(snap):
    return {b[:8]: entry(b) for b in snap}


def plain_walk(batches):
    walk, snaps = FM.ListWalk(T.MDLY), []
    for evs in batches:
        for e in FM.batch_order(evs):
            walk.add(e)
        snaps.append([FM.flight_bytes(f) for f in walk.entries()])
    return walk, snaps


# ---- key, hash, same_home ----------------------------------------------------------------------------------------------------
def test_key_is_seven_bytes_cut_at_the_first_nul():
    assert T.key_of(b"HOT1") == T.key_of(b"HOT1\0\0\0\0") == T.key_of(b"HOT1\0XYZ") == int.from_bytes(b"HOT1", "little") | 1 << 63
    assert T.key_of(b"ABCDEFGH") == T.key_of(b"ABCDEFG") == int.from_bytes(b"ABCDEFG", "little") | 1 << 63
    assert T.key_of(b"") == 1 << 63 and T.key_of(b"S00001") != T.key_of(b"S00010")
    # the finaliser is a bijection of 64-bit words with 0 as its fixed point; one bit in, about half the bits out
    assert T.fl_hash(0) == 0
    flips = [bin(T.fl_hash(T.key_of(b"S00000")) ^ T.fl_hash(T.key_of(b"S00000") ^ (1 << b))).count("1") for b in range(48)]
    assert min(flips) >= 6 and 14 <= sum(flips) / 48.0 <= 18, flips


@pytest.mark.parametrize("cap", [256, 1024])
def test_home_is_spread_evenly(cap):
    """100 000 enumerated addresses over cap homes: every home's count within 5 standard deviations of a Poisson count of the
    mean (5 sigma: about 6e-7 per home), so same_home() finds about 100 000 / cap addresses per prefix character for ANY home"""
    count = collections.Counter(x & (cap - 1) for x in T._hashes(ord("S")))
    mean = 100000.0 / cap
    assert len(count) == cap
    lo, hi = min(count.values()), max(count.values())
    print("cap %d: %d .. %d per home, mean %.1f" % (cap, lo, hi, mean))
    assert mean - 5 * mean ** 0.5 <= lo and hi <= mean + 5 * mean ** 0.5
    assert all(T.home(b"S%05d" % i, cap) == x & (cap - 1) for i, x in list(enumerate(T._hashes(ord("S"))))[::997])


@pytest.mark.parametrize("cap", [256, 1024])
def test_same_home_returns_addresses_of_that_home(cap):
    for h in (0, cap // 2 - 12, cap - 3):
        S = T.same_home(cap, h, 140, b"ST")
        assert len(S) == len(set(S)) == 140 and all(len(a) == 6 for a in S)
        assert all(T.home(a, cap) == h for a in S)
        assert all(T.home(a + b"\0\0", cap) == h for a in S[:5])             # as the record carries it: char[8], NUL padded
    with pytest.raises(ValueError):
        T.same_home(cap, 1, 100000, b"S")


# ---- (a) ---------------------------------------------------------------------------------------------------------------------
def test_aged_traffic_can_drop_nobody_and_turns_the_table_over():
    tr = T.aged_traffic()
    snaps, routes, drops = T.aged_expected()
    assert T.aged_traffic() is tr and T.aged_expected()[0] is snaps                # shared, computed once
    evs = [e for b in tr.batches for e in b]
    addrs = {e.addr for e in evs}
    live = T.live_before(tr.batches, T.MDLY)
    srt = sorted(live[len(live) // 20:])
    print("%d events, %d aircraft, %d batches of %d .. %d; live before a batch: median %d, 1%% %d, max %d; %d routes" %
          (len(evs), len(addrs), len(tr.sizes), min(tr.sizes), max(tr.sizes), srt[len(srt) // 2], srt[len(srt) // 100], srt[-1], len(routes)))
    # nobody can be dropped, whatever the claim order, in a table of 128 slots or more
    assert T.claimable_everywhere(tr.batches, T.MDLY, T.FL_PROBE)
    assert not T.claimable_everywhere(tr.batches, T.MDLY, T.FL_PROBE // 2)           # (the condition does bind)
    assert drops == 0
    # the size of it: 20 generations of a 1024-slot table, 80 of a 256-slot one
    assert len(addrs) == T.AGED_AIRCRAFT + 1 and len(addrs) >= 20 * 256 and 55000 <= len(evs) <= 65000
    assert min(tr.sizes) == 1 and max(tr.sizes) <= 400 and sum(tr.sizes) == len(evs) and len(tr.sizes) >= 300
    assert sum(s >= 60 for s in tr.sizes) >= 100                                     # passes with many segments, not only small ones
    # the table is under pressure all the time: 60 .. 100 live entries, roughly
    assert 60 <= srt[len(srt) // 2] <= 100 and srt[len(srt) // 100] >= 45 and srt[-1] <= T.FL_PROBE - 2
    assert len(routes) > 1000
    # every insertion but the first few hundred is a take-over in a 256-slot table: far more aircraft than slots
    assert len(addrs) - 256 > 19000


def test_aged_traffic_hot_aircraft_and_returns():
    tr = T.aged_traffic()
    snaps = T.aged_expected()[0]
    walk, plain = plain_walk(tr.batches[:200])
    assert plain == snaps[:200]
    evs = [e for b in tr.batches for e in b]
    hot = [e for e in evs if e.addr == T.addr8(T.HOT)]
    # heard in every second of the traffic
    secs = {e.sec for e in hot}
    assert secs >= set(range(min(e.sec for e in evs) + 1, max(e.sec for e in evs)))
    # one entry throughout: its ts is its first message's, its count at the end is all of them
    first = min(hot, key=lambda e: (e.end, e.chn))
    for k, snap in enumerate(snaps):
        mine = [b for b in snap if b[:8] == T.addr8(T.HOT)]
        assert len(mine) == 1, k
    for snap in (snaps[0], snaps[len(snaps) // 2], snaps[-1]):
        f = by_addr(snap)[T.addr8(T.HOT)]
        assert (f.ts_sample, f.ts_sec, f.ts_usec) == (first.soh, first.sec, first.usec)
    assert by_addr(snaps[-1])[T.addr8(T.HOT)].nbm == len(hot) and len(hot) > 15000
    # the returns: every one of them comes back more than mdly + 1 s after it was last heard -> a new entry, AGED_RETURNS times
    last, gaps = {}, {}
    for e in evs:
        if e.addr in last and e.sec - last[e.addr] > T.MDLY + 1:
            assert e.addr not in gaps
            gaps[e.addr] = e.sec - last[e.addr]
        last[e.addr] = max(e.sec, last.get(e.addr, e.sec))
    assert set(gaps) == {T.addr8(a) for a in tr.returned} and len(gaps) == T.AGED_RETURNS >= 300
    # half of them within seconds (their slot probably still carries their key), half after thousands of other aircraft
    assert sum(g <= 8 for g in gaps.values()) == sum(g >= 99 for g in gaps.values()) == T.AGED_RETURNS // 2


def test_expect_without_nothing_dropped_is_the_list_walk():
    for tr in (T.window_traffic(500, True), T.contended_traffic(), T.overfull_traffic()):
        walk, plain = plain_walk(tr.batches)
        snaps, routes, drops = T.expect_without(dict(mdly=T.MDLY), tr.batches, [()] * len(tr.batches))
        assert snaps == plain and routes == [FM.route_bytes(r) for r in walk.routes] and drops == 0
        assert len(routes) >= 10


# ---- (b), (c) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,full", [(500, True), (CAP - 3, False)], ids=["middle", "wraps"])
def test_window_traffic_fills_one_window_and_expires_it(h, full):
    tr = T.window_traffic(h, full)
    S, st, o = tr.S, tr.step, tr.others
    a8 = T.addr8
    assert len(set(S)) == 131 and all(T.home(a, CAP) == h for a in S)
    assert (h + T.FL_PROBE - 1 >= CAP) == (not full)                                 # the window wraps round the table's end, or not
    assert T.home(o["clock"], CAP) == (h + 512) % CAP
    assert all(s == 1 for s in tr.sizes[:128]) and st["fill"] == 127
    snaps, routes, drops = T.expect_without(dict(mdly=T.MDLY), tr.batches, tr.gone)
    assert drops == 2 and len(routes) >= 10
    # all 128 stay live while the window fills, so S[i] sits in slot h + i and S[128] has nowhere to go
    assert [len(s) for s in snaps[:128]] == list(range(1, 129))
    assert {b[:8] for b in snaps[st["fill"]]} == {a8(a) for a in S[:128]}
    assert snaps[st["alone"]] == snaps[st["fill"]]
    w3, before = by_addr(snaps[st["with3"]]), by_addr(snaps[st["fill"]])
    assert set(w3) == set(before) and w3[a8(S[3])].nbm == 2 and snaps[st["with3"]][0][:8] == a8(S[3])
    assert [bytes(w3[k]) for k in w3 if k != a8(S[3])] == [bytes(before[k]) for k in before if k != a8(S[3])]
    if full:
        assert T.home(o["plus64"], CAP) == h + 64 and T.home(o["minus1"], CAP) == h - 1
        assert len(snaps[st["plus64"]]) == 129 and len(snaps[st["minus1"]]) == 130
    # S[7] is heard every second and stays; from the third second on S[0 .. 6], before it on its probe path, have expired
    keep = range(st["keep"] - 8, st["keep"] + 1)
    assert [by_addr(snaps[b])[a8(S[7])].nbm for b in keep] == list(range(2, 11))
    there = [a8(S[0]) in by_addr(snaps[b]) for b in keep]               # S[0]: last heard 0.7 s before the fill ended
    assert there[0] and not any(there[2:])
    assert all(by_addr(snaps[b])[a8(S[7])].ts_sample == by_addr(snaps[st["fill"]])[a8(S[7])].ts_sample for b in keep)
    # 10 s on everything else has expired
    assert [b[:8] for b in snaps[st["clock"]]] == [a8(o["clock"]), a8(S[7])]
    back = by_addr(snaps[st["back"]])
    assert set(back) == {a8(o["clock"]), a8(S[128]), a8(S[5]), a8(S[7])}
    e5 = [e for e in tr.batches[st["back"]] if e.addr == a8(S[5])][0]
    assert back[a8(S[5])].nbm == 1 and (back[a8(S[5])].ts_sample, back[a8(S[5])].ts_sec) == (e5.soh, e5.sec)
    assert back[a8(S[128])].nbm == 1
    if full:
        s0, s5 = by_addr(snaps[st["s0"]]), by_addr(snaps[st["s5"]])
        assert s0[a8(S[0])].nbm == 1 and s0[a8(S[0])].ts_sample == tr.batches[st["s0"]][0].soh and len(s0) == 5
        assert s5[a8(S[5])].nbm == 2 and s5[a8(S[5])].ts_sample == e5.soh and len(s5) == 5
        assert st["s5"] == len(tr.sizes) - 1
    # and left in, S[128] would be in the list from its first message on: the two expectations differ
    plain = plain_walk(tr.batches)[1]
    assert plain[st["alone"]] != snaps[st["alone"]] and len(plain[st["alone"]]) == 129


# ---- (d), (e) ----------------------------------------------------------------------------------------------------------------
def test_contended_traffic_fills_the_window_exactly():
    tr = T.contended_traffic()
    S, h, a8 = tr.S, 400, T.addr8
    assert len(set(S)) == 140 and all(T.home(a, CAP) == h for a in S) and h + T.FL_PROBE <= CAP
    assert len(tr.sizes) == 30 and all(s == 1 for s in tr.sizes[:28])
    snaps, routes, drops = T.expect_without(dict(mdly=T.MDLY), tr.batches, tr.gone)
    assert T.live_before(tr.batches, T.MDLY)[28:] == [28, 128]
    big = collections.Counter(e.addr for e in tr.batches[28])
    new = [a8(a) for a in S[28:128]]
    assert set(big) == {a8(a) for a in S[:128]} and all(2 <= big[a] <= 5 for a in new)
    # the 128 of them are all alive after the batch, every message counted
    after = by_addr(snaps[28])
    assert set(after) == set(big) and sum(f.nbm for f in after.values()) == 28 + tr.sizes[28]
    # the last batch: five more of that home (the window holds 128 live entries: none of them can fit) and 40 from elsewhere
    last = collections.Counter(e.addr for e in tr.batches[29])
    assert set(last) == {a8(a) for a in S[128:133]} | {a8(a) for a in tr.others} and len(tr.others) == len(set(tr.others)) == 40
    homes = [T.home(a, CAP) for a in tr.others]
    assert len(set(homes)) == 40 and all(h + T.FL_PROBE <= x and x + T.FL_PROBE <= CAP + h for x in homes)
    assert drops == 5 and set(by_addr(snaps[29])) == set(big) | {a8(a) for a in tr.others}
    assert any(last[a8(a)] > 1 for a in S[128:133])                                  # (dropped once per call, not per message)
    assert len(routes) >= 20


def test_overfull_traffic_has_eight_slots_for_twenty():
    tr = T.overfull_traffic()
    S, a8 = tr.S, T.addr8
    assert all(T.home(a, CAP) == 700 for a in S) and 700 + T.FL_PROBE <= CAP
    assert len(tr.sizes) == 121 and all(s == 1 for s in tr.sizes[:120])
    assert T.live_before(tr.batches, T.MDLY)[120] == 120
    big = collections.Counter(e.addr for e in tr.batches[120])
    new = {a8(a) for a in S[120:140]}
    assert new <= set(big) <= {a8(a) for a in S} and all(3 <= big[a] <= 5 for a in new)
    walk, plain = plain_walk(tr.batches)
    assert len(plain[120]) == 140                                                     # nobody expires: with room, all 140 would be there
    assert len({r["addr"] for r in walk.routes} & new) >= 8                           # routes that a drop must keep out of the queue
