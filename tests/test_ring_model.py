"""tests/ring_model.py (the block ring's host protocol: which sequence numbers a collect / drain hands out, what it declares lost
and what it returns) beside a brute-force ring: an array of `cap` slots into which every issued call writes its sequence numbers,
all writes done before each claim.  No GPU.  tests/test_gpu_ring_laps.py holds the library to the same model."""
import random

import pytest

import ring_model as RM

NEAR_WRAP = (1 << 32) - 1


def random_schedule(rng):
    cap = rng.choice((8, 16, 32, 64))
    start = rng.choice((0, rng.randrange(1 << 32), (NEAR_WRAP - rng.randrange(3 * cap)) & RM.MASK, NEAR_WRAP))
    steps = []
    for _ in range(rng.randrange(5, 60)):
        r = rng.random()
        if r < 0.55:
            steps.append(("process", rng.randrange(cap // 2 + 1)))
        elif r < 0.9:
            steps.append(("collect", rng.randrange(4), rng.choice((0, 1, 3, rng.randrange(cap + 1), 4 * cap))))
        else:
            steps.append(("drain", rng.choice((1, 5, rng.randrange(1, cap + 1), 4 * cap))))
    return cap, start, steps


def play(ring, brute, steps, seen, on_claim=None):
    """runs the steps on model and brute-force ring; returns (handed out, whether live - consumed ever exceeded cap)"""
    handed, lapped = 0, False
    for st in steps:
        if st[0] == "process":
            ring.process(st[1])
            brute.process(st[1])
            lapped |= RM.sdiff(ring.live(), ring.consumed) > ring.cap
            assert ring.live() == brute.count
            continue
        rc, lost, first, take = ring.collect(st[1], st[2]) if st[0] == "collect" else ring.drain(st[1])
        assert (rc == RM.EOVERFLOW) == (lost > 0) and 0 <= take <= max(0, st[-1]) and take <= ring.cap
        if on_claim:
            on_claim(st, rc, lost, first, take)
        want = RM.seq_range(first, take)
        assert brute.read(first, take) == want, (st, first, take)          # every claimed slot still holds its own block
        assert not (seen & set(want))                                       # nothing is handed out twice
        seen |= set(want)
        handed += take
    return handed, lapped


def test_random_schedules_claim_only_live_slots_and_account_for_every_block():
    rng = random.Random(20261020)
    laps = clean = wraps = behind = 0
    for _ in range(4000):
        cap, start, steps = random_schedule(rng)
        ring, brute, seen = RM.Ring(cap, start), RM.BruteRing(cap, start), set()
        handed, lapped = play(ring, brute, steps, seen)
        while True:                                                         # the final drain, through a small buffer
            rc, lost, first, take = ring.drain(7)
            want = RM.seq_range(first, take)
            assert brute.read(first, take) == want and not (seen & set(want))
            seen |= set(want)
            handed += take
            if rc == RM.OK:
                break
        produced = sum(s[1] for s in steps if s[0] == "process")
        assert handed + ring.lost_total == produced and ring.consumed == brute.count
        if not lapped:
            assert ring.lost_total == 0
        laps += ring.lost_total > 0
        clean += not lapped
        wraps += start + produced > RM.MASK and start != 0
    assert laps >= 500 and clean >= 500 and wraps >= 300               # the schedules reach what they are meant to reach


def test_return_codes_after_a_lap():
    """the loss is reported once; the calls after it say EAGAIN until a last OK"""
    ring = RM.Ring(32)
    for _ in range(9):
        ring.process(13)                                                    # 117 blocks: 3 * cap + cap / 2 <= 117
    rcs = []
    while True:
        rc, lost, first, take = ring.drain(5)
        rcs.append(rc)
        assert (lost, first, take) == ((85, 85, 5) if len(rcs) == 1 else (0, 85 + 5 * (len(rcs) - 1), min(5, 117 - first)))
        if rc == RM.OK:
            break
    assert rcs == [RM.EOVERFLOW] + [RM.EAGAIN] * 5 + [RM.OK]
    assert ring.collect(1, 5) == (RM.OK, 0, 117, 0) and ring.drain(5) == (RM.OK, 0, 117, 0)


def test_a_mark_behind_the_consumer_claims_nothing():
    ring = RM.Ring(16, NEAR_WRAP - 3)
    ring.process(6)
    ring.process(2)
    assert ring.drain(100) == (RM.OK, 0, NEAR_WRAP - 3, 8)                  # (across the wrap)
    assert ring.collect(1, 100) == (RM.OK, 0, 4, 0) and ring.collect(5, 100) == (RM.OK, 0, 4, 0)


# ---- the designed schedules of the GPU tests, on the parent's rule ------------------------------------------------------------------
def designed_adds(seed, cap, ncalls=40):
    rng = random.Random(seed)
    return [rng.randrange(cap // 8, cap // 3) for _ in range(ncalls)]


def steps_with_counts(adds, steps):
    """the schedule's steps in play()'s form: a process step carries its block count, a drain_all is a run of drains"""
    out = []
    for st in steps:
        if st[0] == "process":
            out.append(("process", adds[st[1]]))
        elif st[0] == "drain_all":
            out += [("drain", st[1])] * 4
        elif st[0] == "collect":
            out.append(st)
    return out


DESIGNED = {
    "B": lambda adds, cap: RM.schedule_b(adds, cap, lag=1),
    "C": lambda adds, cap: RM.schedule_c(adds, cap, small=3, lag=1),
    "D": lambda adds, cap: RM.schedule_b(adds, cap, lag=2),
    "G": lambda adds, cap: RM.schedule_b(adds, cap, lag=1, sync=False),     # (a sync is no step of the model: G is B and C to it)
}


@pytest.mark.parametrize("name", sorted(DESIGNED))
@pytest.mark.parametrize("start", [0, NEAR_WRAP - 20])
def test_parents_rule_hands_out_an_overwritten_slot_on_the_designed_schedules(name, start):
    """`lost` computed from the collect's own mark instead of the live count (ParentRing): on schedules B, C, D and G a claim
    returns slots that the newest call has overwritten, says OK or EAGAIN while doing so, and later hands the same blocks out
    again.  The model's rule passes the same schedules.  So the GPU tests of these schedules can fail."""
    cap = 32
    for seed in range(20):
        adds = designed_adds(seed, cap)
        steps = steps_with_counts(adds, DESIGNED[name](adds, cap))
        ring, brute, seen = RM.Ring(cap, start), RM.BruteRing(cap, start), set()
        rcs = []
        play(ring, brute, steps, seen, on_claim=lambda st, rc, *r: rcs.append(rc))
        assert RM.EOVERFLOW in rcs and ring.consumed == brute.count        # the schedule does lap, and the model survives it
        parent, brute = RM.ParentRing(cap, start), RM.BruteRing(cap, start)
        stale, twice, seen = [], 0, set()
        for st in steps:
            if st[0] == "process":
                parent.process(st[1])
                brute.process(st[1])
                continue
            rc, lost, first, take = parent.collect(st[1], st[2]) if st[0] == "collect" else parent.drain(st[1])
            have = brute.read(first, take)
            if have != RM.seq_range(first, take):
                stale.append((rc, lost))
            twice += len(seen & set(have))
            seen |= set(have)
        assert stale and stale[0][0] in (RM.OK, RM.EAGAIN) and stale[0][1] == 0, (name, seed)   # silently
        assert twice > 0, (name, seed)                                      # ... and the new blocks arrive twice
