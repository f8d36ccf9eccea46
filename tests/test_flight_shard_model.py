"""One flight table for the channels of several contexts, on the model alone (tests/flight_model.py): the rule that export and
import of flight events rely on.  Channels are sharded `c mod N`; a ROUND is what every context consumes between two imports.
Merging the shards' events of a round by (end_sample, chn) gives back the single context's pass, so the list walk over the merged
stream is the list walk over the unsharded one -- table, routes, expiry.  Applying the shards one after the other inside a round
does NOT: the round contract of include/acarsdec_amd.h is needed, not a convenience."""
import functools

import numpy as np
import pytest

import flight_model as FM

T0 = (1700000000, 250000)
MDLY = 2
NCH = 64
AIRPORTS = [b"KJFK", b"EGLL", b"LFPG", b"EDDF", b"KBOS", b"LEMD"]


@functools.lru_cache(maxsize=None)
def traffic():
    """20 000 events over 64 channels in time order (distinct end samples), a quarter from one aircraft, the rest from 400; about
    10 ms apart with a silence of 2 .. 5 s now and then, so that with mdly = 2 entries expire inside rounds and between them;
    cut into rounds of 1 .. 500.  ([the events of each round], all events)"""
    rng = np.random.default_rng(20261020)
    n = 20000
    gaps = np.where(rng.random(n) < 0.004, rng.uniform(2.0, 5.0, n), rng.exponential(0.01, n))
    end = 30000 + np.cumsum(np.rint(gaps * 12500).astype(np.int64) + 1)
    evs = []
    for i in range(n):
        addr = b"HOT1" if rng.random() < 0.25 else b"N%05d" % int(rng.integers(0, 400))
        fid = b"" if rng.random() < 0.1 else b"XY%04d" % int(rng.integers(0, 40))
        soh = int(end[i]) - int(rng.integers(600, 10200))
        fields = tuple(AIRPORTS[int(rng.integers(0, 6))] if rng.random() < 0.2 else b"\0" * 4 for _ in range(7))
        sec, usec = FM.tv(T0[0], T0[1], soh)
        evs.append(FM.Event(addr, fid, int(rng.integers(0, NCH)), soh, int(end[i]), sec, usec, fields, rng.random() < 0.8))
    rounds, at = [], 0
    while at < n:
        s = min(int(rng.integers(1, 501)), n - at)
        rounds.append(evs[at:at + s])
        at += s
    return rounds, evs


def walk_rounds(rounds_in_order):
    """the list walk over rounds whose events are already in the order they are applied in:
    ([the entries after every round], routes, entries made anew after an expiry)"""
    walk, snaps = FM.ListWalk(MDLY), []
    for evs in rounds_in_order:
        for e in evs:
            walk.add(e)
        snaps.append([FM.flight_bytes(f) for f in walk.entries()])
    return snaps, [FM.route_bytes(r) for r in walk.routes], walk.recreated


@functools.lru_cache(maxsize=None)
def unsharded():
    rounds, _ = traffic()
    return walk_rounds([FM.batch_order(r) for r in rounds])


@pytest.mark.parametrize("N", [2, 3, 4])
def test_events_merged_per_round_give_the_single_context_walk(N):
    rounds, evs = traffic()
    assert len(evs) == 20000 and len({(e.end, e.chn) for e in evs}) == len(evs) and max(len(r) for r in rounds) <= 500
    merged = []
    for r in rounds:
        shards = [[e for e in r if e.chn % N == k] for k in range(N)]                # what each context extracts ...
        assert sum(len(s) for s in shards) == len(r)
        merged.append(FM.batch_order([e for s in shards[::-1] for e in s]))          # ... arrives in any order, the pass sorts it
    want = unsharded()
    got = walk_rounds(merged)
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2]
    assert want[2] > 100 and len(want[1]) > 100 and max(len(s) for s in want[0]) > 50    # expiry, routes and a table worth the name


@pytest.mark.parametrize("N", [2, 3, 4])
def test_shard_after_shard_inside_a_round_is_a_different_table(N):
    """the owner's events first, then each peer's, each in its own (end_sample, chn) order: not the single context's walk"""
    rounds, _ = traffic()
    per_shard = [[e for k in range(N) for e in FM.batch_order([e for e in r if e.chn % N == k])] for r in rounds]
    want = unsharded()
    got = walk_rounds(per_shard)
    assert got[0] != want[0]
    assert sum(g != w for g, w in zip(got[0], want[0])) > len(rounds) // 2           # not a corner case: most rounds differ
