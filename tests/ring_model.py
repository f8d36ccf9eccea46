"""A model of the block ring's HOST protocol (acarsdec_amd/csrc/results.cpp: ring_upto, ring_claim, ring_result), plain Python,
written from the contract in include/acarsdec_amd.h (ACG_EOVERFLOW, acg_collect_frames) and importing nothing from the project.

State: `cap` (the ring's length, a power of two), `consumed` (the sequence number of the oldest block not yet handed out) and
cnt[k], the queue length after process call k; `start` stands for cnt[-1].  All counters are 32-bit and wrap.

With N calls issued, a claim through a buffer of `max` records does this:

    live    = cnt[N-1]
    upto    = live                for a drain
            = cnt[N-1-lag]        for a collect (N <= lag: the collect claims nothing)
    lost    = max(0, live - cap - consumed);   consumed += lost
    pending = max(0, upto - consumed)          a signed difference: a mark may lie behind the consumer
    take    = min(pending, max)
    rc      = EOVERFLOW if lost else EAGAIN if take < pending else OK
    hands out the sequence numbers [consumed, consumed + take);   consumed += take

`lost` comes from `live`, not from `upto`: every issued call writes into the ring whether or not the host has waited for it, so
what the newest call overwrote is gone for a collect that ends at an older mark too.  ParentRing restates the rule this replaced
(`lost` from `upto`); tests/test_ring_model.py shows on a brute-force ring where it hands out an overwritten slot."""

OK, EOVERFLOW, EAGAIN = 0, -5, -7
MASK = 0xFFFFFFFF


def sdiff(a, b):
    """a - b of two wrapping 32-bit counters as a signed difference"""
    d = (a - b) & MASK
    return d - (1 << 32) if d >> 31 else d


class Ring:
    def __init__(self, cap, start=0):
        assert cap >= 2 and cap & (cap - 1) == 0
        self.cap = cap
        self.start = start & MASK
        self.consumed = self.start
        self.cnt = []
        self.lost_total = 0

    def process(self, nblocks):
        """one process call that queues nblocks blocks"""
        assert nblocks >= 0
        self.cnt.append((self.live() + nblocks) & MASK)

    def live(self):
        return self.cnt[-1] if self.cnt else self.start

    def lost_from(self, upto):
        """how many of the oldest blocks a claim that ends at `upto` declares lost"""
        return max(0, sdiff(self.live(), self.consumed) - self.cap)

    def _claim(self, upto, max_recs):
        lost = self.lost_from(upto)
        self.consumed = (self.consumed + lost) & MASK
        self.lost_total += lost
        pending = max(0, sdiff(upto, self.consumed))
        take = min(pending, max(0, max_recs))
        rc = EOVERFLOW if lost else EAGAIN if take < pending else OK
        first = self.consumed
        self.consumed = (self.consumed + take) & MASK
        return rc, lost, first, take

    def collect(self, lag, max_recs):
        """(rc, lost, first, take): the sequence numbers first .. first + take - 1 (mod 2^32) are handed out"""
        n = len(self.cnt)
        if n <= lag:
            return OK, 0, self.consumed, 0
        return self._claim(self.cnt[n - 1 - lag], max_recs)

    def drain(self, max_recs):
        return self._claim(self.live(), max_recs)


class ParentRing(Ring):
    """the rule before the fix: the lap is judged against the mark the claim ends at, and a collect whose mark lies behind the
    consumer claims nothing"""

    def lost_from(self, upto):
        return max(0, sdiff(upto, self.consumed) - self.cap)


class BruteRing:
    """cap slots; every issued call writes its sequence numbers at once (all writes are done before each claim)"""

    def __init__(self, cap, start=0):
        self.cap = cap
        self.slot = [None] * cap
        self.count = start & MASK

    def process(self, nblocks):
        for _ in range(nblocks):
            self.slot[self.count & (self.cap - 1)] = self.count
            self.count = (self.count + 1) & MASK

    def read(self, first, take):
        """what the slots of [first, first + take) hold now"""
        return [self.slot[(first + i) & (self.cap - 1)] for i in range(take)]


def seq_range(first, take):
    return [(first + i) & MASK for i in range(take)]


# ---- the designed schedules of tests/test_gpu_ring_laps.py, as lists of steps over a given production per call -------------------
# a step is ("process", k) | ("sync",) | ("collect", lag, max): ONE C call | ("drain_all", max): drain calls until one says OK
def first_silent_lap(adds, cap, lag):
    """the first K (calls issued) with cnt[K-1-lag] - consumed <= cap < cnt[K-1] - consumed for a host that has consumed nothing,
    or None"""
    cnt, tot = [], 0
    for a in adds:
        tot += a
        cnt.append(tot)
    for K in range(lag + 1, len(cnt) + 1):
        if cnt[K - 1 - lag] <= cap < cnt[K - 1]:
            return K
    return None


def schedule_a(adds, small=5, ncalls=None):
    """no collect over the first ncalls calls (default: all), then a drain through a buffer of `small` records until it says OK"""
    return [("process", k) for k in range(len(adds) if ncalls is None else ncalls)] + [("drain_all", small)]


def schedule_b(adds, cap, lag=1, sync=True, tail=3):
    """no collect until the silent lap; sync; collect(lag); one more call; collect(lag); drain; `tail` more calls and a drain"""
    K = first_silent_lap(adds, cap, lag)
    assert K is not None and K + tail < len(adds), "the traffic never laps a collect silently"
    steps = [("process", k) for k in range(K)]
    if sync:
        steps.append(("sync",))
    steps += [("collect", lag, 1 << 20), ("process", K)]
    if sync:
        steps.append(("sync",))
    steps += [("collect", lag, 1 << 20), ("drain_all", 1 << 20)]
    steps += [("process", k) for k in range(K + 1, K + 1 + tail)] + [("drain_all", 1 << 20)]
    return steps


def schedule_c(adds, cap, small=3, lag=1, sync=True, ncalls=None):
    """collect(lag) through a buffer of `small` records after every call: the remainder goes stale until the newest call laps it;
    then (sync and) collect again, and a drain"""
    steps = []
    for k in range(len(adds) if ncalls is None else ncalls):
        steps.append(("process", k))
        steps.append(("collect", lag, small))
    if sync:
        steps.append(("sync",))
    steps += [("collect", lag, small), ("drain_all", 1 << 20)]
    return steps
