"""The reassembly table's specification (tests/reasm_model.py) on hand-written chains with every status reached, the proof that the
device's slot reclaiming is unobservable, the conditions the random GPU traffic keeps, the kernels' budget read from the code
object, and the ABI.  No GPU."""
import os
import re
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reasm_cases as RC  # noqa: E402
import reasm_model as RM  # noqa: E402
from acarsdec_amd import _capi as K  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_status_values_are_libacars_in_libacars_order():
    assert RM.NAMES == ("unknown", "complete", "in progress", "skipped", "duplicate", "out of sequence", "invalid args", "overflow")
    assert (K.REASM_UNKNOWN, K.REASM_COMPLETE, K.REASM_IN_PROGRESS, K.REASM_SKIPPED, K.REASM_DUPLICATE, K.REASM_OUT_OF_SEQUENCE,
            K.REASM_ARGS_INVALID, K.REASM_OVERFLOW) == tuple(range(8))
    hdr = open(os.path.join(ROOT, "include", "acarsdec_amd.h")).read()
    for v, n in enumerate(("UNKNOWN", "COMPLETE", "IN_PROGRESS", "SKIPPED", "DUPLICATE", "OUT_OF_SEQUENCE", "ARGS_INVALID", "OVERFLOW")):
        assert re.search(r"#define ACG_REASM_%s\s+%d\b" % (n, v), hdr), n


def test_hand_written_chains_reach_every_status():
    msgs, want = RC.hand_chains()
    got, done, _ = RM.run(msgs, [len(msgs)])
    assert got == want
    assert set(want) >= {RM.COMPLETE, RM.IN_PROGRESS, RM.SKIPPED, RM.DUPLICATE, RM.OUT_OF_SEQUENCE}
    # the completed messages: the 3-block downlink without the repeated block's text twice, the three uplinks, the seam chain
    assert [(c.addr, c.msn, c.nfrag, c.down) for c in done] == [(b"N123AB", b"M01", 3, 1), (b"UP2", b"", 3, 0), (b"UPX", b"", 4, 0), (b"UPW", b"", 2, 0),
                                                                  (b"N123AB", b"M06", 5, 1)]
    assert done[0].text == RM.msg_text(msgs[0]) + RM.msg_text(msgs[1]) + RM.msg_text(msgs[3])
    assert done[0].first_soh_sample == msgs[0].soh_sample and done[0].soh_sample == msgs[3].soh_sample and done[0].chn == msgs[3].chn
    assert done[4].text == b"abcdef" + RC.text_of(3, 242) + b"xyz"
    # cut into calls anywhere: the same (the table is resident, the order rule holds per call)
    for cut in range(1, len(msgs)):
        g2, d2, _ = RM.run(msgs, [cut, len(msgs) - cut])
        assert g2 == want and RC.completed_tuples(d2) == RC.completed_tuples(done)


def test_overflow_at_exactly_max_text_plus_one():
    for max_text in (16, 256, 3584):
        msgs, want = RC.overflow_chain(max_text)
        got, done, _ = RM.run(msgs, [len(msgs)], max_text=max_text)
        assert got == want and RM.OVERFLOW in got
        assert len(done) == 1 and len(done[0].text) == max_text


def test_time_out_boundaries_and_whose_time_out_it_is():
    msgs, want = RC.timeout_chains()
    got, done, _ = RM.run(msgs, [len(msgs)], t0_us=1700000000 * 10**6 + 999999)
    assert got == want
    assert sorted(c.addr for c in done) == [b"TU1", b"TX2"]
    tu = [c for c in done if c.addr == b"TU1"][0]
    assert tu.nfrag == 2 and tu.text == b"t6t7"                      # E and F: the chain restarted one sample past 90 s


def test_keys_that_differ_in_one_character_stay_apart():
    msgs = RC.one_field_keys()
    got, done, _ = RM.run(msgs, [len(msgs)])
    assert set(got) == {RM.IN_PROGRESS, RM.COMPLETE} and len(done) == 11 and all(c.nfrag == 4 for c in done)
    assert len({(c.addr, c.label, c.msn) for c in done}) == 11


@pytest.fixture(scope="module")
def traffic():
    msgs = RC.random_traffic()
    return msgs, RC.random_batches(len(msgs), seed=5)


def test_random_traffic_reaches_what_it_is_for(traffic):
    msgs, batches = traffic
    got, done, _ = RM.run(msgs, batches)
    count = {s: got.count(s) for s in set(got)}
    print("random traffic:", {RM.NAMES[s]: c for s, c in count.items()}, "completed", len(done), "calls", len(batches))
    assert len(msgs) == 20000 and 250 <= len({RM.key_of(m) for m in msgs if RM.creates(m)}) <= 300
    for s in (RM.COMPLETE, RM.IN_PROGRESS, RM.SKIPPED, RM.DUPLICATE, RM.OUT_OF_SEQUENCE):
        assert count.get(s, 0) >= 100, RM.NAMES[s]
    assert 2 <= min(c.nfrag for c in done) and max(c.nfrag for c in done) == 16 and any(not c.down for c in done)
    assert min(batches) == 1 and max(batches) == 2000
    # time-outs happen: some chain restarts although its key still has an entry
    t = RM.Table()
    expired = 0
    for i in RM.call_order(msgs):
        m = msgs[i]
        e = t.table.get(RM.key_of(m))
        if RM._c(m.bs) != RM.ETX and RM._c(m.bid) != 0 and e is not None and 80 * m.soh_sample > e.first_us + e.timeout_us:
            expired += 1
        t.add(m)
    assert expired >= 20, expired


def test_slot_reclaiming_is_unobservable(traffic):
    """The device lets a new key take over the slot of an entry that expired more than 2 s before G, the largest tv of the earlier
    calls.  In a call's order tv runs backwards by less than a block (0.87 s), and every tv of a later call is larger than G minus
    that: whoever would find the entry finds it expired and deletes it.  So a table that throws such entries away at the start of
    every call gives the same statuses and the same completed messages -- on the random traffic, under several cuts into calls."""
    msgs, batches = traffic
    assert all(0 < m.end_sample - m.soh_sample < RC.BLOCK_SAMPLES for m in msgs)
    for b in (batches, RC.random_batches(len(msgs), seed=6), [1] * 3000 + [len(msgs) - 3000], [len(msgs)]):
        plain = RM.run(msgs, b)
        lazy = RM.run(msgs, b, reclaim=True)
        assert plain[0] == lazy[0] and RC.completed_tuples(plain[1]) == RC.completed_tuples(lazy[1])
    # (and the rule is not vacuous: entries are thrown away)
    t = RM.Table(reclaim=True)
    gone, at = 0, 0
    for n in batches:
        before = len(t.table)
        t.begin_call()
        gone += before - len(t.table)
        for i in RM.call_order(msgs[at:at + n]):
            t.add(msgs[at + i])
        at += n
    assert gone >= 20, gone


def test_random_traffic_can_drop_nobody(traffic):
    """live + new keys of the call <= FL_PROBE - 1 in every call: whatever order the claims come in, a key that looks for a slot
    finds one within its 128, in a table of 256 as of 1024 entries.  `live` counts what the device cannot take over: the entries
    of the reclaiming model."""
    msgs, batches = traffic
    for b in (batches, RC.random_batches(len(msgs), seed=6)):
        _, _, load = RM.run(msgs, b, reclaim=True)
        print("occupancy: max", max(load))
        assert max(load) <= RC.FL_PROBE - 1 and max(load) >= 40


# DESIGN.md 4 states these: VGPRs and LDS bytes per kernel of reasm.hip as the product builds it
BUDGET = {"extract": (30, 0), "gather": (9, 0), "heads": (18, 0), "walk": (72, 1024), "finish": (4, 0)}


def test_reasm_kernels_use_no_scratch_and_keep_their_budget():
    from acarsdec_amd import _build as B
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    assert hipcc, "hipcc"
    csrc = os.path.join(ROOT, "acarsdec_amd", "csrc")
    flags = {name: (f, prod) for name, f, prod in B.UNITS}
    assert flags["reasm.hip"] == (["-O3", "--offload-compress"], True)
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include")] +
                       flags["reasm.hip"][0] + ["-S", "-o", "-", os.path.join(csrc, "reasm.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = [n.split("reasm_")[1].split("_kernel")[0] for n in re.findall(r"^\s*\.amdhsa_kernel (\S+)", r.stdout, flags=re.M)]
    scratch = [int(v) for v in re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", r.stdout)]
    vgpr = [int(v) for v in re.findall(r"\.amdhsa_next_free_vgpr (\d+)", r.stdout)]
    lds = [int(v) for v in re.findall(r"\.amdhsa_group_segment_fixed_size (\d+)", r.stdout)]
    print("reasm.hip kernels:", list(zip(names, vgpr, lds, scratch)))
    assert sorted(names) == sorted(BUDGET) and len(scratch) == len(BUDGET) and not any(scratch), (names, scratch)
    assert "scratch_" not in r.stdout
    assert {n: (v, l) for n, v, l in zip(names, vgpr, lds)} == BUDGET
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for n, (v, l) in BUDGET.items():
        assert re.search(r"\| `reasm_%s_kernel` \| %d \| %d \|" % (n, v, l), design), n


def test_abi_exports_the_reassembly_entry_points():
    names = ("acg_reasm_enable", "acg_drain_msgs_reasm", "acg_collect_msgs_reasm", "acg_drain_reassembled", "acg_reasm_status_name")
    hdr = open(os.path.join(ROOT, "include", "acarsdec_amd.h")).read()
    lab = open(os.path.join(ROOT, "include", "acarsdec_amd_lab.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", K.LIB_PATH], capture_output=True, text=True).stdout
    out_lab = subprocess.run(["nm", "-D", "--defined-only", K.LAB_PATH], capture_output=True, text=True).stdout
    for n in names:
        assert n in K.SYMBOLS and re.search(r"\b%s\(" % n, hdr) and re.search(r" T %s$" % n, out, flags=re.M) and re.search(r" T %s$" % n, out_lab, flags=re.M), n
    assert "acg_selftest_reasm" in K.LAB_SYMBOLS and re.search(r"\bacg_selftest_reasm\(", lab) and "acg_selftest_reasm" not in hdr
    assert re.search(r" T acg_selftest_reasm$", out, flags=re.M) and re.search(r" T acg_selftest_reasm$", out_lab, flags=re.M)
    L = K.load()
    assert [L.acg_reasm_status_name(i) for i in range(8)] == [n.encode() for n in RM.NAMES]
    assert L.acg_reasm_status_name(-1) == b"unknown" and L.acg_reasm_status_name(8) == b"unknown"
    # the product library exports the lab entry and answers ACG_ESTATE: it is compiled into the lab library only
    cfg = K.ReasmConfig(0, 0, 0, 0)
    import ctypes as C
    nd, dr = C.c_int(0), C.c_int(0)
    assert L.acg_selftest_reasm(None, None, 0, C.byref(cfg), None, None, None, 0, None, 0, C.byref(nd), C.byref(dr), None) == K.ESTATE
    assert L.acg_reasm_enable(None, C.byref(cfg)) == K.EINVAL
    for bad in (K.ReasmConfig(0, 1000000, 0, 0), K.ReasmConfig(0, 0, -1, 0), K.ReasmConfig(0, 0, 0, 24), K.ReasmConfig(0, 0, 0, 65552),
                K.ReasmConfig(0, 0, (1 << 20) + 1, 0)):
        assert K.load(lab=True).acg_selftest_reasm(None, None, 0, C.byref(bad), None, None, None, 0, None, 0, C.byref(nd), C.byref(dr), None) == K.EINVAL
