"""The inputs of tests/test_gpu_msk_exact.py (tests/msk_exact_inputs.py), checked on the oracle alone: the premise under which the
device must equal the oracle bit for bit holds at every sample that file feeds, and the inputs reach what they are there for.
No GPU."""
import os
import re

import numpy as np

import msk_exact_inputs as X
from conftest import ROOT

STATE_FIELDS = ("MskPhi", "MskDf", "MskClk", "MskLvlSum", "MskBitCount", "MskS", "idx", "outbits", "nbits", "Acarsstate", "blk_len",
                "blk_err", "nbit_total", "nsamp_total", "soh_sample")


def same_state(a, b):
    return all(getattr(a, k) == getattr(b, k) for k in STATE_FIELDS) and bytes(a.inb) == bytes(b.inb) and bytes(a.blk_txt) == bytes(b.blk_txt)


def test_model_header_is_the_device_function():
    """tests/sincos_model.h restates msk_common.h's sincos_tab: every constant of the device's text is in the header's, and the
    table is the product's own (host_setup.c), 128 entries as on the device"""
    dev = open(os.path.join(ROOT, "acarsdec_amd", "csrc", "msk_common.h")).read()
    dev = dev[dev.index("void sincos_tab("):dev.index("// n0 / d and n1 / d")]
    hdr = open(os.path.join(ROOT, "tests", "sincos_model.h")).read()
    pat = r"-?\d\.\d{10,}e[-+]\d+(?: [*/] 32\.0)?"
    consts = set(re.findall(pat, dev))
    assert len(consts) == 8 and consts == set(re.findall(pat, hdr)), consts ^ set(re.findall(pat, hdr))
    assert "tab[128][2]" in hdr and "acg_host_sincos_table(&tab[0][0])" in hdr and "q & 127" in hdr
    assert "ACG_SINCOS_N 128" in open(os.path.join(ROOT, "acarsdec_amd", "csrc", "host_setup.c")).read()
    # and the comparison can tell the two apart: one ulp below 2 pi the series' sine is off in its tenth digit (the remainder
    # is what the two-term constant leaves of 2 pi), and this sample's product falls to the other side of a float rounding
    # (met with SEED 20261019 on a planted channel)
    assert X.products_differing([6.283185307179585], [np.float32(0.6715259)]) == (1, 0)
    assert X.products_differing([6.283185307179585, 1.0], [np.float32(0.5), np.float32(0.6715259)]) == (0, -1)


def test_walk_is_the_run():
    """the oracle stepped one sample at a time (where the phases of the premise come from) is the oracle run call by call: the same
    state at the end of every call of both schedules, at every cut point and behind every planted call"""
    w = X.oracle_walk(X.EVEN)
    for sched in (X.EVEN, X.RAGGED):
        for end, row in zip(np.cumsum(sched), X.oracle_run(sched)):
            for ch, s in enumerate(row):
                assert s.c.MskPhi == w.phi[ch, end - 1] and s.c.Acarsstate == w.astate[ch, end - 1], (sched, end, ch)
    assert all(same_state(s.c, w.last[ch]) for ch, s in enumerate(X.oracle_run(X.EVEN)[-1]))
    for t in X.cut_points():
        state, calls = X.oracle_cut(t)
        for ch in range(X.NCH):
            assert state[ch].c.MskPhi == w.phi[ch, t - 1] and state[ch].c.nsamp_total == t
            for n in X.SHORT:
                if t + n <= sum(X.EVEN):
                    assert calls[n][ch].c.MskPhi == w.phi[ch, t + n - 1]
                    assert len(calls[n][ch].vo) == w.nbit[ch, t + n - 1] - w.nbit[ch, t - 1]
    wp = X.oracle_walk(X.PLANT_CALLS, planted=True)
    assert all(same_state(s.c, wp.last[ch]) for ch, s in enumerate(X.oracle_run(X.PLANT_CALLS, planted=True)[-1]))


def test_premise_no_mixer_product_differs_from_cexp():
    """At every (phase, sample) pair the oracle visits on the inputs of the GPU file -- every sample of both schedules and of the
    calls behind the cut points (one trajectory: the first sum(EVEN) + 128 samples of a free run), and every sample of the planted
    calls -- the device's sin/cos model gives the two float products of glibc's cexp.  0 differ.  Should a change of the inputs
    ever break this: another SEED in msk_exact_inputs.py, never another number here."""
    x = X.tracks()
    total = 0
    for sched, planted in (([X.NSAMP], False), (X.PLANT_CALLS, True)):
        w = X.oracle_walk(sched, planted)
        n = sum(sched)
        bad, first = X.products_differing(w.phi, x[:, :n])
        ch, i = divmod(first, n) if first >= 0 else (-1, -1)
        assert bad == 0, "%d products differ; the first on channel %d, sample %d, phase %r (planted: %s)" % (bad, ch, i, w.phi[ch, i], planted)
        total += 2 * w.phi.size
    assert total == 2 * X.NCH * (X.NSAMP + sum(X.PLANT_CALLS))
    # the free walk is the trajectory of the schedules
    assert np.array_equal(X.oracle_walk([X.NSAMP]).phi[:, :sum(X.EVEN)], X.oracle_walk(X.EVEN).phi)
    # the planted run is where the phase goes negative (df = -1), outside the range the table reduction was written for
    wp = X.oracle_walk(X.PLANT_CALLS, True)
    assert wp.phi.min() < -2 * np.pi and X.oracle_walk(X.EVEN).phi.min() >= 0 and wp.phi.max() < X.TWO_PI


def test_inputs_do_their_job():
    x = X.tracks()
    assert x.shape == (X.NCH, X.NSAMP) and x.dtype == np.float32 and np.isfinite(x).all()
    run, w = X.oracle_run(X.EVEN), X.oracle_walk(X.EVEN)
    assert {ch % X.NKINDS for ch in range(X.NCH)} == set(range(X.NKINDS))
    enters = lambda ch, a, b: int(np.sum((w.astate[ch, :-1] == a) & (w.astate[ch, 1:] == b)))
    for ch in range(X.NCH):
        k = ch % X.NKINDS
        nblocks = sum(len(row[ch].blocks) for row in run)
        if k in X.PASSING:
            # every kind whose frames are meant to come out: at least 3 blocks within sum(EVEN) samples
            assert nblocks >= 3, (ch, X.KIND_NAMES[k], nblocks)
        elif k == 2:
            # six parity errors: the block is dropped at the fifth (acars.c:312), three times at least, and none comes out
            assert nblocks == 0 and enters(ch, X.TXT, X.WSYN) >= 3, (ch, nblocks)
        elif k == 3:
            # a frame of a 230-byte text is 21000 samples: it never ends here, the channel stays in TXT with a long text
            assert nblocks == 0 and run[-1][ch].c.Acarsstate == X.TXT and run[-1][ch].c.blk_len > 80, ch
        else:
            assert nblocks == 0 and not (w.astate[ch] >= X.SOH1).any(), ch
        if k in X.FRAMED:
            # bit periods of five and of six samples
            at = np.flatnonzero(np.diff(np.concatenate([[0], w.nbit[ch]])))
            assert {5, 6} <= set(np.diff(at).tolist()), (ch, np.bincount(np.diff(at)))
    # both ways a block ends: the second CRC byte (acars.c:348) and DEL behind a lost terminator (acars.c:323)
    assert sum(enters(ch, X.CRC2, X.END) for ch in range(X.NCH)) >= 20 and sum(enters(ch, X.TXT, X.END) for ch in range(X.NCH)) >= 6
    # both polarities, among the bits that completed a block
    pol = {int(w.pol[ch, i + 1]) for ch in range(X.NCH) for i in np.flatnonzero((w.astate[ch, :-1] != X.END) & (w.astate[ch, 1:] == X.END))}
    assert pol == {0, 2}, pol
    # the drifting track carries channel 0's bits (the same blocks come out) and its bits fall on other samples
    at = lambda ch: np.flatnonzero(np.diff(np.concatenate([[0], w.nbit[ch]])))
    text = lambda ch: [(f.len, bytes(f.txt[: f.len]), bytes(f.crc)) for row in run for f in row[ch].blocks]
    assert text(12) == text(0) and len(text(0)) >= 3
    assert not np.array_equal(np.diff(at(12))[:1500], np.diff(at(0))[:1500])
    # the scaled and quantised tracks are not channel 0 again
    for ch in (9, 10, 11):
        assert not np.array_equal(x[ch], x[0]) and text(ch) == text(0)
    assert max(len(f.txt[: f.len]) for row in run for s in row for f in s.blocks) <= 40


def test_cut_points_hit_every_framing_state_but_crc2():
    """the public state (acg_chan_state) does not carry the held first CRC byte, so a decoder cannot be brought to CRC2: no cut
    lies there, on any channel; every other state is met by some channel at some cut"""
    cuts, w = X.cut_points(), X.oracle_walk(X.EVEN)
    assert set(np.cumsum(X.EVEN).tolist()) <= set(cuts) and len(cuts) <= 12
    seen = set()
    for t in cuts:
        state, _ = X.oracle_cut(t)
        here = {int(s.c.Acarsstate) for s in state}
        assert X.CRC2 not in here, t
        assert here == set(w.astate[:, t - 1].tolist())
        seen |= here
    assert seen == {X.WSYN, X.SYN2, X.SOH1, X.TXT, X.CRC1, X.END}, seen
    # a channel planted in TXT or CRC1 brings a text and a distance back to its SOH
    assert any(s.c.Acarsstate == X.CRC1 and len(s.text) > 13 and s.soh_back > 0 for t in cuts for s in X.oracle_cut(t)[0])


def test_oracle_soft_bits_are_finite_everywhere():
    rows = [X.oracle_run(X.EVEN), X.oracle_run(X.RAGGED), X.oracle_run(X.PLANT_CALLS, planted=True)]
    rows += [list(X.oracle_cut(t)[1].values()) for t in X.cut_points()]
    nbits = 0
    for run in rows:
        for row in run:
            for s in row:
                assert np.isfinite(s.vo).all() and np.isfinite(s.lvl).all() and (s.lvl >= 0).all()
                assert all(np.isfinite(v) for v in (s.c.MskPhi, s.c.MskDf, s.c.MskClk, s.c.MskLvlSum))
                nbits += len(s.vo)
    assert nbits > 50000
    # the plants do what they are there for: under df = -1 the clock never fires in the call (that df = +3 fires on
    # the first sample, plants() itself asserts)
    run = X.oracle_run(X.PLANT_CALLS, planted=True)
    p = X.plants()
    kinds = set()
    for i, row in enumerate(run):
        for ch in range(0, X.NCH, 2):
            j = p.index(X.plant_for(i, ch))
            kinds.add((j, ch))
            if j == 12:
                assert len(row[ch].vo) == 0, (i, ch)
    assert len(p) == 14 and len(kinds) == 14 * len(range(0, X.NCH, 2))          # every plant on every planted channel
