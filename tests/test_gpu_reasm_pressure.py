"""The reassembly table's slots under load (reasm.hip: reasm_heads_kernel's lookup, reasm_claim, the walk's seam) through the lab
entry acg_selftest_reasm: the take-over of an expired but still live entry at its edge, the probe bound inside a larger table,
claims racing in one pass, and sample indices above 2^32.  The inputs and the premises they rest on are
tests/reasm_table_model.py's, proven on the CPU by tests/test_reasm_table_model.py; every expectation is tests/reasm_model.py's over
the same calls without the blocks of the keys that found no slot, and exact."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reasm_cases as RC  # noqa: E402
import reasm_model as RM  # noqa: E402
import reasm_table_model as T  # noqa: E402
from test_gpu_reasm import done_tuple  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    from acarsdec_amd import _capi
    assert _capi.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return _capi


def device_run(K, msgs, batches, max_msgs, t0=T.T0):
    """msgs through acg_selftest_reasm in calls of `batches` records: (statuses, completed tuples, dropped)"""
    L = K.load(lab=True)
    n = len(msgs)
    assert sum(batches) == n
    arr = RC.pack(msgs)
    b = (C.c_int * len(batches))(*batches)
    cfg = K.ReasmConfig(t0[0], t0[1], max_msgs, 0)
    status = (C.c_ubyte * n)()
    done = (K.ReasmMsg * n)()
    cap = n * 242 + 16
    text = C.create_string_buffer(cap)
    nd, dr = C.c_int(0), C.c_int(-1)
    rc = L.acg_selftest_reasm(arr, b, len(batches), C.byref(cfg), None, status, done, n, text, cap, C.byref(nd), C.byref(dr), None)
    assert rc == K.OK, rc
    out, at = [], 0
    for i in range(nd.value):
        r = done[i]
        assert r.text_off == at
        out.append(done_tuple(r, text.raw[at:at + r.text_len]))
        at += r.text_len
    return list(status[:n]), out, dr.value


def same(status, want, msgs):
    bad = [i for i in range(len(want)) if status[i] != want[i]]
    assert not bad, (len(bad), [(i, RM.key_of(msgs[i]), RM.NAMES[status[i]], RM.NAMES[want[i]]) for i in bad[:10]])


def test_expiry_take_over_at_its_edge(K):
    """128 live entries in 128 slots.  A new key finds no slot while G <= first + time-out + 2 s of the earliest entry, and exactly
    one when G lies one sample behind that -- at 90 s for the earliest uplink entry, at 660 s for the earliest downlink entry; then
    every slot changes hands at once.  The chains begun in taken-over slots complete with their own 1 - 10 bytes: nothing of the
    previous tenant's row or of its last incomplete dword."""
    sc = T.expiry_takeover()
    want, want_done, want_dropped = T.expect(sc.msgs, sc.batches, sc.lost)
    status, done, dropped = device_run(K, sc.msgs, sc.batches, max_msgs=128)
    n = sc.note
    print("expiry take-over: dropped %d; at the edges %s" % (dropped, {name: RM.NAMES[status[n[name][0]]] for name in n if name[:2] in ("up", "do")}))
    for tag in ("up", "down"):
        assert status[n[tag + "_at"][0]] == status[n[tag + "_past"][0]] == RM.SKIPPED
        assert [status[n[tag + s][0]] for s in ("_full", "_still", "_takes", "_fullagain")] == [RM.UNKNOWN, RM.UNKNOWN, RM.IN_PROGRESS, RM.UNKNOWN]
        assert status[n[tag + "_done"][0]] == RM.COMPLETE and status[n[tag + "_idle"][0]] == RM.IN_PROGRESS
    assert [status[i] for i in n["fillers"] + n["last"]] == [RM.IN_PROGRESS] * (27 + 127)
    same(status, want, sc.msgs)
    assert dropped == want_dropped == 6
    assert done == want_done and len(done) == 2 + 127 + 28


@pytest.mark.parametrize("h", [100, 256 - 5], ids=["middle", "wraps"])
def test_probe_window_inside_a_larger_table(K, h):
    """128 keys of one home fill their window in ONE pass of a 256-slot table; the 129th finds no slot with 128 free; keys of the
    homes next to it do; the 128 final blocks in one pass find every entry, the window's last slot included; the 129th fits then"""
    sc = T.probe_window(h)
    want, want_done, want_dropped = T.expect(sc.msgs, sc.batches, sc.lost)
    status, done, dropped = device_run(K, sc.msgs, sc.batches, max_msgs=256)
    n = sc.note
    print("window at %d: fill %s, 129th %s, dropped %d" % (h, {RM.NAMES[status[i]] for i in n["fill"]}, RM.NAMES[status[n["129th"][0]]], dropped))
    assert [status[i] for i in n["fill"]] == [RM.IN_PROGRESS] * 128
    assert status[n["129th"][0]] == RM.UNKNOWN and dropped == want_dropped == 1
    assert [status[i] for i in n["neighbours"]] == [RM.IN_PROGRESS] * 2
    assert [status[i] for i in n["finals"]] == [RM.COMPLETE] * 128
    assert status[n["129th_again"][0]] == RM.IN_PROGRESS
    same(status, want, sc.msgs)
    assert done == want_done and len(done) == 131


def test_claims_racing_in_one_pass(K):
    """100 live chains and ONE pass with 40 new keys: 28 slots for 40 claims.  Which keys win is the race's; exactly 28 first
    blocks are IN_PROGRESS and 12 UNKNOWN, dropped == 12, and with those 12 left out everything is the model's: the winners and
    the 100 complete with their own text in (end_sample, chn) order, the losers' final blocks are OUT_OF_SEQUENCE"""
    sc = T.racing_claims()
    status, done, dropped = device_run(K, sc.msgs, sc.batches, max_msgs=128)
    n = sc.note
    first = [status[i] for i in n["new"]]
    print("racing claims: %d in progress, %d unknown, dropped %d" % (first.count(RM.IN_PROGRESS), first.count(RM.UNKNOWN), dropped))
    assert first.count(RM.IN_PROGRESS) == 28 and first.count(RM.UNKNOWN) == 12 and dropped == 12
    losers = [i for i in n["new"] if status[i] == RM.UNKNOWN]
    gone = {RM.key_of(sc.msgs[i]) for i in losers}
    want, want_done, want_dropped = T.expect(sc.msgs, sc.batches, losers)
    same(status, want, sc.msgs)
    assert want_dropped == 12
    assert [status[i] for i in n["old"]] == [RM.IN_PROGRESS] * 100
    assert all(status[i] == (RM.OUT_OF_SEQUENCE if RM.key_of(sc.msgs[i]) in gone else RM.COMPLETE) for i in n["finals"])
    assert done == want_done and len(done) == 128
    assert {(d[7], d[8], d[9]) for d in done} == {RM.key_of(sc.msgs[i]) for i in n["old"] + n["new"]} - gone
    ends = [(d[3], d[0]) for d in done]
    assert ends == sorted(ends)


@pytest.fixture(scope="module")
def unshifted(K):
    msgs, batches = T.large_index_traffic()
    want = RM.run(msgs, batches, t0_us=T.T0_US)
    got = device_run(K, msgs, batches, max_msgs=256)
    same(got[0], want[0], msgs)
    assert got[1] == RC.completed_tuples(want[1]) and got[2] == 0
    return got


@pytest.mark.parametrize("off", T.OFFSETS, ids=["2^32-1e6", "2^42"])
def test_statuses_and_records_at_large_sample_indices(K, unshifted, off):
    """the random traffic with end_sample and soh_sample moved up by 2^32 - 10^6 (one call straddles 2^32) and by 2^42 (the time
    key's 43 bits are all in use), t0 moved back to match: the statuses of the unshifted run, its completed records with the three
    sample stamps shifted"""
    msgs, batches = T.large_index_traffic()
    if off == T.OFFSETS[0]:
        assert len(T.straddles(msgs, batches, off)) == 1                                  # the premise: one call holds both sides
    t0, _ = T.t0_before(off)
    status, done, dropped = device_run(K, T.shifted(msgs, off), batches, max_msgs=256, t0=t0)
    same(status, unshifted[0], msgs)
    assert done == T.shifted_done(unshifted[1], off) and dropped == 0
    assert len(done) > 1000 and max(d[3] for d in done) >= (1 << 32) + 10**6
