"""The flight table (flight.hip, THE TABLE) in the regime its slot rules exist for: every slot a tombstone and every insertion a
take-over, one probe window filled to its last slot -- in the middle of the table and round its end --, a hundred claims racing
for a hundred slots, and more claims than slots.  Everything goes through acg_selftest_flights with mdly = 2 and the records
shuffled inside each batch; every snapshot, the route list and `dropped` are held to the list walk (tests/flight_model.py) minus
what a call had to drop (tests/flight_table_model.py, whose conditions tests/test_flight_table_model.py proves without a GPU).
GPU box only."""
import ctypes as C

import numpy as np
import pytest

import flight_model as FM
import flight_table_model as T
from test_gpu_flights import T0

pytestmark = pytest.mark.gpu

CAP = T.CAP


@pytest.fixture(scope="module")
def D():
    from acarsdec_amd import decoder
    from acarsdec_amd import _capi as K
    assert K.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return decoder


def run(D, tr, cap, seed, nbatch=None):
    """the first nbatch batches of tr through acg_selftest_flights on a fresh table of `cap` slots:
    ([the entries' bytes after every batch], [the routes' bytes], dropped)"""
    from acarsdec_amd import _capi as K
    sizes = tr.sizes[:nbatch]
    recs = tr.shuffled(np.random.default_rng(seed), nbatch)
    f = D.make_msg_filter(**T.filter_kw())
    cfg = K.FlightConfig(T0[0], T0[1], T.MDLY, cap)
    snap_cap, route_cap = min(cap, 256) * len(sizes), sum(sizes)
    snaps, routes = (K.Flight * snap_cap)(), (K.Route * route_cap)()
    snap_n, nroutes, dropped = (C.c_int * len(sizes))(), C.c_int(0), C.c_int(0)
    rc = K.load().acg_selftest_flights(recs, (C.c_int * len(sizes))(*sizes), len(sizes), C.byref(cfg), C.byref(f), snaps, snap_cap, snap_n,
                                       routes, route_cap, C.byref(nroutes), C.byref(dropped))
    assert rc == K.OK, rc
    blob, out, at = bytes(snaps), [], 0
    for b in range(len(sizes)):
        out.append([blob[120 * i:120 * i + 120] for i in range(at, at + snap_n[b])])
        at += snap_n[b]
    return out, [bytes(routes[i]) for i in range(nroutes.value)], dropped.value


def same(got, want):
    """every snapshot, the route list and the drop count; on a mismatch the first batch and row that differ"""
    assert [len(s) for s in got[0]] == [len(s) for s in want[0]][:len(got[0])], \
        next((b, len(g), len(w)) for b, (g, w) in enumerate(zip(got[0], want[0])) if len(g) != len(w))
    for b, (g, w) in enumerate(zip(got[0], want[0])):
        assert g == w, (b, next(i for i in range(len(w)) if g[i] != w[i]))
    assert got[1] == want[1]
    assert got[2] == want[2]


def entry(b):
    from acarsdec_amd import _capi as K
    return K.Flight.from_buffer_copy(b)


def by_addr(snap):
    out = {b[:8]: b for b in snap}
    assert len(out) == len(snap), "two entries share an address"
    return out


# ---- (a) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [128, 256, 1024])
def test_a_table_many_times_older_than_its_size(D, cap):
    """20 001 aircraft in 62 054 events (470 batches of 1 .. 261) through a table of 128 (the probe window is the table), 256 and
    1024 slots (the window is a part of it): 156, 78 and 19.5 times as many aircraft as slots, so all but the first few hundred
    insertions take an expired slot over, while 46 .. 79 entries are live and one aircraft, heard every second, must stay ONE
    entry in the middle of the churn; 500 aircraft come back after they expired, half within seconds, half after thousands of
    others.  live + aircraft of the batch <= 127 in every batch, so no claim order can drop anybody (the model's docstring):
    dropped == 0, and every snapshot and the routes are the plain list walk's."""
    tr, want = T.aged_traffic(), T.aged_expected()
    addrs = {e.addr for b in tr.batches for e in b}
    assert len(addrs) >= 20 * min(cap, 256) + 1 and len(tr.returned) >= 300 and want[2] == 0      # the premise
    got = run(D, tr, cap, 31 + cap)
    assert got[2] == 0
    same(got, want)
    hot = T.addr8(T.HOT)
    first = min((e for b in tr.batches for e in b if e.addr == hot), key=lambda e: (e.end, e.chn))
    for b, snap in enumerate(got[0]):
        mine = [x for x in snap if x[:8] == hot]
        assert len(mine) == 1, b
        if b % 50 == 0 or b == len(got[0]) - 1:
            f = entry(mine[0])
            assert (f.ts_sample, f.ts_sec, f.ts_usec) == (first.soh, first.sec, first.usec), b
    assert entry(by_addr(got[0][-1])[hot]).nbm == sum(e.addr == hot for b in tr.batches for e in b)


# ---- (b), (c) ----------------------------------------------------------------------------------------------------------------
def window(D, h, full):
    tr = T.window_traffic(h, full)
    want = T.expect_without(dict(mdly=T.MDLY), tr.batches, tr.gone)
    st, S, a8 = tr.step, tr.S, T.addr8
    got = run(D, tr, CAP, 5 + h)
    same(got, want)
    # `dropped` step by step: the same batches up to each step, on a fresh table (one aircraft per batch: nothing races)
    steps = ["fill", "alone", "with3"] + (["plus64", "minus1"] if full else []) + ["keep", "clock", "back"] + (["s0", "s5"] if full else [])
    counts = {}
    for name in steps:
        part = run(D, tr, CAP, 5 + h, st[name] + 1)
        assert part[0] == got[0][:st[name] + 1], name
        counts[name] = part[2]
    assert counts == dict(dict.fromkeys(steps, 2), fill=0, alone=1), counts
    # and what each step is there for, on the device's own bytes
    assert len(got[0][st["fill"]]) == 128 and got[0][st["alone"]] == got[0][st["fill"]]
    w3 = by_addr(got[0][st["with3"]])
    assert a8(S[128]) not in w3 and entry(w3[a8(S[3])]).nbm == 2
    for b in range(st["keep"] - 8, st["clock"] + 1):                      # S[7], live behind the expired keys of S[0 .. 6]: one entry
        assert entry(by_addr(got[0][b])[a8(S[7])]).nbm == min(b - st["keep"] + 10, 10), b
    assert len(got[0][st["clock"]]) == 2
    back = by_addr(got[0][st["back"]])
    assert set(back) == {a8(S[128]), a8(S[5]), a8(S[7]), a8(tr.others["clock"])}
    e5 = [e for e in tr.batches[st["back"]] if e.addr == a8(S[5])][0]
    f5 = entry(back[a8(S[5])])
    assert f5.nbm == 1 and (f5.ts_sample, f5.ts_sec, f5.ts_usec) == (e5.soh, e5.sec, e5.usec)
    return tr, got


def test_one_probe_window_filled_one_aircraft_at_a_time(D):
    """131 aircraft whose home is slot 500 of 1024 (flight_table_model.home() restates the hash: if it drifts, nobody is dropped
    here and the test fails).  S[0 .. 127] go in one per batch and stay live: the 128th still fits (a probe loop one short
    drops it).  S[128] finds 128 live slots: dropped, once per call, the snapshot unchanged; S[3] in the same call is updated.
    Home + 64 reaches 64 slots past the crowd and fits, home - 1 fits.  S[7] is then heard once a second and stays ONE live
    entry BEHIND the keys of S[0 .. 6] as they expire (a lookup that stops at an expired key makes a second S[7]).  10 s on
    everything else is expired: S[128] takes a tombstone this pass did not mark, S[5] restarts in its own, S[0] (its tombstone
    taken) comes back as a fresh entry, and S[5] is found again where it is."""
    tr, got = window(D, 500, True)
    st, S, a8 = tr.step, tr.S, T.addr8
    assert len(got[0][st["plus64"]]) == 129 and len(got[0][st["minus1"]]) == 130
    assert got[0][st["minus1"]][0][:8] == a8(tr.others["minus1"]) and got[0][st["minus1"]][1][:8] == a8(tr.others["plus64"])
    s0, s5 = by_addr(got[0][st["s0"]]), by_addr(got[0][st["s5"]])
    assert entry(s0[a8(S[0])]).nbm == 1 and entry(s0[a8(S[0])]).ts_sample == tr.batches[st["s0"]][0].soh
    assert len(s5) == 5 and entry(s5[a8(S[5])]).nbm == 2


def test_a_probe_window_that_wraps_round_the_end_of_the_table(D):
    """the same with home slot 1021: the window is slots 1021 .. 1023, 0 .. 124"""
    window(D, CAP - 3, False)


# ---- (d) ---------------------------------------------------------------------------------------------------------------------
def test_contended_claims(D):
    """28 live aircraft of home slot 400, then ONE call with 100 new ones of that home (2 .. 5 messages each) and messages of the
    28: a hundred waves claim the hundred free slots of one window at the same time.  All 128 are there once, with the list
    walk's bytes and every message counted -- a claim that ignores `touch`, or a compare-and-swap loser that keeps the slot it
    lost, puts two aircraft into one slot and loses one of them; a claim that skips a free slot drops the last.  The next call
    brings 5 more of that home and 40 aircraft from elsewhere.  Which of several new aircraft of one call get the last slots is
    unspecified; here the window holds 128 live entries before the call starts, so NONE of the five can fit
    whatever the order: the dropped are determined, and so is every byte of the snapshot."""
    tr = T.contended_traffic()
    want = T.expect_without(dict(mdly=T.MDLY), tr.batches, tr.gone)
    S, a8 = tr.S, T.addr8
    part = run(D, tr, CAP, 91, 29)
    assert part[2] == 0
    assert part[0] == want[0][:29]
    after = by_addr(part[0][28])                                          # (no two entries share an address)
    assert set(after) == {a8(a) for a in S[:128]} and len(part[0][28]) == 128
    assert sum(entry(b).nbm for b in after.values()) == sum(tr.sizes[:29])
    got = run(D, tr, CAP, 92)
    assert got[2] == 5
    same(got, want)
    # as test_table_state_handling: whoever is present carries its complete entry, and the present are the 128 and the 40
    last = by_addr(got[0][29])
    assert set(last) == {a8(a) for a in S[:128]} | {a8(a) for a in tr.others}
    whole = by_addr(T.expect_without(dict(mdly=T.MDLY), tr.batches, [()] * 30)[0][29])
    assert all(last[a] == whole[a] for a in last) and len(whole) == len(last) + 5


# ---- (e) ---------------------------------------------------------------------------------------------------------------------
def test_more_new_aircraft_than_free_slots_in_one_call(D):
    """120 live aircraft of home slot 700, then ONE call with 20 new ones of that home: 8 slots for 20 claims.  Exactly 12 are
    dropped; 128 of the home are present; who is present has its complete entry (all its messages of the call, or none); and
    the route queue holds the routes of the present, in order, and none of a dropped aircraft.  WHO gets the 8 slots is
    unspecified and not asserted."""
    tr = T.overfull_traffic()
    S, a8 = tr.S, T.addr8
    whole = T.expect_without(dict(mdly=T.MDLY), tr.batches, [()] * 121)
    part = run(D, tr, CAP, 93, 120)
    assert part[2] == 0 and part[0] == whole[0][:120]
    got = run(D, tr, CAP, 94)
    assert got[2] == 12
    assert got[0][:120] == whole[0][:120]
    present = by_addr(got[0][120])
    assert len(present) == 128 and set(present) <= {a8(a) for a in S} and set(present) >= {a8(a) for a in S[:120]}
    # complete, and in the list walk's order: the list walk with the absent left out
    gone = [a for a in S[120:] if a8(a) not in present]
    assert len(gone) == 12
    want = T.expect_without(dict(mdly=T.MDLY), tr.batches, [()] * 120 + [gone])
    assert all(present[a] == by_addr(whole[0][120])[a] for a in present)
    route_addr = lambda r: r[41:49]
    assert all(route_addr(r) in present for r in got[1])
    assert any(route_addr(r) in {a8(a) for a in gone} for r in whole[1]), "no dropped aircraft would have had a route"
    same(got, want)
