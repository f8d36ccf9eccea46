"""The device block repair (csrc/blk.hip blk_repair_kernel) on the crafted corpus of tests/repair_corpus.py: blocks of every
length 13 .. 241, damage at chosen positions (every byte index, slot boundaries, same lane / different slot, byte 12), blocks
whose search has several acceptable candidates (found by mining: the reference takes the first of its loop order, the kernel
"the first hit of the first 64-group"), unrepairable blocks, blocks the framing drops.  tests/test_repair_corpus.py pins the
oracle used here to a Python restatement and to the real blk_thread on the same audio (CPU).

1024 channels, calls of 8 x 1024 samples, every transmission ending inside one of three calls: those repair passes see 400 - 600
blocks with 128 waves, so every wave takes several blocks with its prefetch in flight.  All comparisons are exact."""
import collections
import functools

import pytest

import repair_corpus as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def D():
    from acarsdec_amd import decoder
    from acarsdec_amd import _capi as K
    assert K.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return decoder


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@functools.lru_cache(maxsize=1)
def expected():
    """(audio [NCH, NSAMP], per channel: [(raw oracle frame, processed frame | None)] in the order the blocks were queued)"""
    from oracle import oracle as O
    items, _ = RC.corpus()
    x = RC.audio(items)
    per = []
    for c in range(RC.NCH):
        ch = O.Channel(c, max_frames=16)
        ch.demod(x[c])
        per.append([(f, O.blk_process(f)) for f in ch.frames])
    return x, per


def stamp(f):
    return (int(f.end_bit), int(f.end_sample))


def play(dec, x, after_call):
    out = []
    for k in range(0, RC.NSAMP, RC.CALL):
        dec.demod_msk(x[:, k:k + RC.CALL])
        out += after_call()
    return out


def by_chn(records, key):
    out = collections.defaultdict(list)
    for r in sorted(records, key=lambda r: (int(r.chn), int(r.end_bit))):
        out[int(r.chn)].append(key(r))
    return [out.get(c, []) for c in range(RC.NCH)]


@functools.lru_cache(maxsize=1)
def device_raw_keys():
    """(chn, end_bit, end_sample) + block of everything the device's framing queues (repair off): one run, used twice"""
    from acarsdec_amd import decoder as D
    x, _ = expected()
    dec = D.Decoder(RC.NCH, decim=8, ntaps=8, max_blocks=8, repair=False, bitlog=False)
    got = play(dec, x, dec.drain_frames)
    dec.close()
    return by_chn(got, lambda f: D.frame_tuple(f) + stamp(f))


def test_passes_see_more_blocks_than_they_have_waves():
    """the condition on the input that makes the run below a test of the per-wave loop and its prefetch: at least three calls
    queue more than twice as many blocks as their repair pass has waves (one wave per 8 channels, at least 128)"""
    _, per = expected()
    calls = collections.Counter(int(f.end_sample) // RC.CALL for blocks in per for f, _ in blocks)
    assert sum(1 for n in calls.values() if n > 2 * max(128, RC.NCH // 8)) >= 3, calls


def test_framing_queues_the_oracles_raw_blocks(O):
    """repair off: a framing fault would show here, a repair fault only below"""
    _, per = expected()
    want = [[O.frame_tuple(f) + stamp(f) for f, _ in blocks] for blocks in per]
    got = device_raw_keys()
    assert sum(map(len, want)) >= 1600
    for c in range(RC.NCH):
        assert got[c] == want[c], c


def test_repair_delivers_the_oracles_blocks_and_drops_the_oracles_drops(D, O):
    x, per = expected()
    dec = D.Decoder(RC.NCH, decim=8, ntaps=8, max_blocks=8, repair=True, bitlog=False)
    got = by_chn(play(dec, x, dec.drain_frames), lambda f: D.frame_tuple(f) + stamp(f))
    dec.close()
    want = [[O.frame_tuple(o) + stamp(o) for _, o in blocks if o is not None] for blocks in per]
    assert sum(map(len, want)) >= 1500
    bad = [c for c in range(RC.NCH) if got[c] != want[c]]
    assert not bad, (len(bad), bad[:5], got[bad[0]], want[bad[0]])
    # the dropped blocks: what the framing queued (the run without repair) minus what was delivered
    raw = device_raw_keys()
    dropped = {(t[0],) + t[-2:] for c in range(RC.NCH) for t in raw[c]} - {(t[0],) + t[-2:] for c in range(RC.NCH) for t in got[c]}
    want_dropped = {(c,) + stamp(f) for c in range(RC.NCH) for f, o in per[c] if o is None}
    assert dropped == want_dropped and len(dropped) >= 80


def test_message_records_of_the_corpus_match_the_oracles_split(D, O):
    """the same through the message sink, collected one call behind: records == msg_split(blk_process(raw))"""
    x, per = expected()
    dec = D.Decoder(RC.NCH, decim=8, ntaps=8, max_blocks=8, repair=True, bitlog=False, max_lag=1)
    got = play(dec, x, lambda: dec.collect_msgs(lag=1))
    got += dec.drain_msgs()
    dec.close()
    got = by_chn(got, lambda m: O.msg_tuple(m) + stamp(m))
    want = []
    for blocks in per:
        rows = []
        for _, o in blocks:
            if o is not None:
                rows.append(O.msg_tuple(O.msg_split(o)) + stamp(o))
        want.append(rows)
    assert sum(map(len, want)) >= 1500
    bad = [c for c in range(RC.NCH) if got[c] != want[c]]
    assert not bad, (len(bad), bad[:5], got[bad[0]], want[bad[0]])
