"""Inputs of the bit-exact demodulator tests (tests/test_msk_exact_inputs.py on the CPU, tests/test_gpu_msk_exact.py on the GPU): the
tracks, the call schedules, the planted loop states, the oracle's run over them, and the one premise under which the device has to
equal the oracle bit for bit.

The premise.  The device's mixer takes sin/cos from a table and a short series (msk_common.h sincos_tab, <= 2.1 ulp), the oracle
calls glibc's cexp; what either keeps is (float)(in * cos p), (float)(in * -sin p) (msk.c:90).  Everything else in the loop is
the same IEEE operation on both sides.  So the inputs here are CHOSEN such that at every (phase, sample) pair the oracle visits,
the model of the device's sin/cos (tests/sincos_model.h, the device's operations on the CPU) gives the same two float products
as cexp: products_differing() counts the pairs where it does not, and tests/test_msk_exact_inputs.py asserts that the count is 0
over every run the GPU file makes.  If a change of the tracks or of SEED ever makes that count non-zero, choose another SEED: the
GPU test has no share of cases it may skip, and the assertion `== 0` stays.

Sizes.  The schedules are 9536 and 9256 samples: at 1200 bit/s that is 915 bits, so the texts are short (a frame of a 10-byte text
is about 1600 samples), and the kind with texts of 230-250 bytes never finishes a frame here -- it is a channel that stays in TXT
with a long text under assembly."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

NCH = 21
SEED = 20261021                                       # (20261019: one product differs, at a planted phase of 2 pi - 1 ulp; 20261020: a cut in CRC2)
EVEN = [32, 64, 96, 128, 1024, 8192]
RAGGED = [1, 7, 1000, 53, 4099, 4096]                 # no multiples of 32: the kernels' scalar-refill shape
SHORT = [32, 64, 96, 128]                             # the calls behind a planted state
PLANT_CALLS = SHORT * 4                               # every plant in front of each of 16 short calls
NSAMP = sum(EVEN) + max(SHORT)                        # a planted call may start at the end of the last EVEN call
NKINDS = 13
# kinds (channel % 13) that carry frames; PASSING: whose frames are meant to come out as blocks
FRAMED = (0, 1, 2, 3, 7, 8, 9, 10, 11, 12)
PASSING = (0, 1, 7, 8, 9, 10, 11, 12)
KIND_NAMES = ["plain", "inverted", "six parity errors", "texts of 230-250 bytes", "noise", "silence", "constant", "terminator lost",
              "repairable corruption in noise, inverted", "plain * 2^-20", "plain * 4", "plain as int16 / 32768", "plain at 12500 (1 + 2e-4) Hz"]

TWO_PI = 2.0 * 3.14159265358979323846
K_VCO = 1800.0 / 12500 * 2.0 * 3.14159265358979323846
K_3PI2 = 3 * 3.14159265358979323846 / 2.0
WSYN, SYN2, SOH1, TXT, CRC1, CRC2, END = range(7)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


# ---- tracks -----------------------------------------------------------------------------------------------------------------------
def tracks():
    """[NCH, NSAMP] float32 envelopes at 12.5 kHz, read-only, the same array for every caller.  Kinds by channel % 13: the nine of
    test_gpu_lean_order.py -- plain frames; the same inverted (~SYN: the other polarity); six parity errors in the text (the block
    is dropped at MAXPERR + 2, acars.c:312); texts of 230-250 bytes; noise; silence; a constant; the terminator lost (the block
    ends at DEL, acars.c:323); repairable corruption in noise, inverted -- with the pre-key growing by a bit from frame to frame,
    and four made from channel 0's audio: scaled by 2^-20 (the 1e-8 of msk.c:111 counts), scaled by 4, quantised to int16 / 32768
    (what pcm.hip delivers), and the same bits sampled at 12500 (1 + 2e-4) Hz, so that the pattern of five- and six-sample bit
    periods drifts against channel 0's.  No NaN, no Inf."""
    if "x" in _cache:
        return _cache["x"]
    from acarsdec_amd import synth as S
    rng = np.random.default_rng(SEED)
    x = np.zeros((NCH, NSAMP), dtype=np.float32)

    def audio(frames, gap, lead, phases, gaps=None, rate=S.INTRATE):
        parts = [np.zeros(lead)]
        for i, fr in enumerate(frames):
            parts.append(S.msk_audio(S.frame_bits(fr, prekey=32 + (i + len(frames)) % 8), phase0=phases[i], rate=rate))
            parts.append(np.zeros(gaps[i] if gaps is not None else int(rng.integers(*gap))))
        a = np.concatenate(parts)
        return a[:NSAMP] if len(a) >= NSAMP else np.concatenate([a, np.zeros(NSAMP - len(a))])

    text_len = {0: (1, 16), 1: (1, 16), 2: (12, 24), 3: (230, 250), 7: (6, 18), 8: (4, 16)}
    plain = None
    for c in range(NCH):
        k = c % NKINDS
        if k in (0, 1, 2, 3, 7, 8):
            frames = []
            for i in range(3 if k == 3 else 8):
                fr = bytearray(S.acars_frame(text=S.random_text(rng, *text_len[k])))
                if k == 2:
                    assert len(fr) > 32
                    for j in rng.choice(np.arange(20, len(fr) - 6), size=6, replace=False):
                        fr[int(j)] ^= 1 << int(rng.integers(0, 7))
                if k == 7:
                    fr[len(fr) - 4] = S.odd_parity(0x41 + int(rng.integers(0, 26)))
                if k == 8 and len(fr) > 24:
                    fr = bytearray(S.corrupt_frame(bytes(fr), rng, ["p1", "p2", "p3", "p4", "db", "crc"][i % 6]))
                frames.append(bytes(fr))
            lead = int(rng.integers(0, 40))
            phases = [float(rng.uniform(0, 2 * np.pi)) for _ in frames]
            gaps = [int(rng.integers(40, 200)) for _ in frames]
            a = audio(frames, None, lead, phases, gaps)
            if c == 0:
                plain = (frames, lead, phases, gaps)
            x[c] = S.envelope(-a if k in (1, 8) else a, noise=0.02 if k == 8 else 0.0, rng=rng)
        elif k == 4:
            x[c] = rng.normal(0.5, 0.2, size=NSAMP).astype(np.float32)
        elif k == 5:
            x[c] = 0.0
        elif k == 6:
            x[c] = 0.37
        elif k == 9:
            x[c] = x[0] * np.float32(2.0 ** -20)
        elif k == 10:
            x[c] = x[0] * np.float32(4.0)
        elif k == 11:
            x[c] = (np.rint(x[0].astype(np.float64) * 32768.0).astype(np.int16).astype(np.float32) / np.float32(32768.0)).astype(np.float32)
        else:
            frames, lead, phases, gaps = plain
            x[c] = S.envelope(audio(frames, None, lead, phases, gaps, rate=S.INTRATE * (1 + 2e-4)))
    assert np.isfinite(x).all()
    x.setflags(write=False)
    _cache["x"] = x
    return x


# ---- planted loop states (used by tests/test_gpu_lean_chains.py too) ----------------------------------------------------------------
def period(phi, clk, df):
    """one six-sample pass from (phi, clk, df) as the kernels compute it: [(running sum before its wrap, clock)] per sample taken"""
    s = np.float64(K_VCO) + np.float64(df)
    thr = np.float64(K_3PI2) - s / 2
    p, c, out = np.float64(phi), np.float32(clk), []
    for _ in range(6):
        p = p + s
        c = np.float32(np.float64(c) + s)
        out.append((p, c))
        if p >= TWO_PI:
            p = p - np.float64(TWO_PI)                                  # fma(-1, 2 pi, p): one rounding, as the subtraction
        if np.float64(c) >= thr:
            break
    return out


def plants():
    """[(phi, df, clk)]: for j = 1..6 the wrap exactly at step j, then the same one ulp lower, then df = -1 and df = +3"""
    if "plants" in _cache:
        return _cache["plants"]
    exact, below = [], []
    for j in range(1, 7):
        clk = -0.5 if j == 6 else 0.0
        centre = np.float64(TWO_PI) - j * np.float64(K_VCO)
        found = None
        cands = [centre]
        up = down = centre
        for _ in range(64):
            up, down = np.nextafter(up, np.inf), np.nextafter(down, -np.inf)
            cands += [up, down]
        for phi in cands:
            steps = period(phi, clk, 0.0)
            if len(steps) >= j and steps[j - 1][0] == TWO_PI and all(q[0] < TWO_PI for q in steps[:j - 1]):
                found = phi
                break
        assert found is not None, "no phase within 64 ulps whose sum number %d is 2 pi" % j
        lower = np.nextafter(found, -np.inf)
        steps = period(lower, clk, 0.0)
        assert len(steps) >= j and all(q[0] < TWO_PI for q in steps[:j]), j
        exact.append((float(found), 0.0, clk))
        below.append((float(lower), 0.0, clk))
    # five samples from clk = 0, six from clk = -0.5 (the sixth step is taken at all)
    assert len(period(exact[0][0], 0.0, 0.0)) == 5 and len(period(exact[5][0], -0.5, 0.0)) == 6
    # df = -1: the step is negative, never the six-sample pass; df = +3: the clock fires on the first sample
    assert K_VCO - 1.0 < 0 and len(period(1.0, 0.0, 3.0)) == 1
    _cache["plants"] = exact + below + [(1.0, -1.0, 0.0), (1.0, 3.0, 0.0)]
    return _cache["plants"]


def plant_for(call, ch):
    """the plant of channel `ch` in front of call number `call` of PLANT_CALLS, or None.  Even channels are planted, odd ones keep
    their lock, so that both kinds share every wave; every plant reaches every planted channel."""
    if ch % 2:
        return None
    p = plants()
    return p[(ch // 2 + call) % len(p)]


# ---- the oracle's run ---------------------------------------------------------------------------------------------------------------
def frame_key(f, stamps=True):
    """everything a block carries, exactly: (chn, len, err, crc, txt), the level's bit pattern, the three stamps"""
    k = (int(f.chn), int(f.len), int(f.err), bytes(f.crc), bytes(f.txt[: max(0, f.len)]), np.float32(f.lvl).tobytes().hex())
    return k + (int(f.end_bit), int(f.end_sample), int(f.soh_sample)) if stamps else k


class Snap:
    """one channel after one call: `c` a copy of the oracle's OrcChan (every field of the device's ChanState is in it), `text` the
    bytes under assembly (TXT and CRC1, else empty), `vo` / `lvl` the bit log of the call, `blocks` the OrcFrames it completed"""
    __slots__ = ("c", "text", "vo", "lvl", "blocks")

    @property
    def soh_back(self):
        return int(self.c.nsamp_total - self.c.soh_sample) if self.c.Acarsstate in (TXT, CRC1, CRC2) else 0


def oracle_run(schedule, planted=False, nch=NCH):
    """The oracle (oracle/acars_oracle.c through O.Channel) over tracks() in calls of the lengths `schedule`; planted: plant_for()'s
    (MskPhi, MskDf, MskClk) written into the channel in front of every call.  Returns [call][channel] -> Snap.  Cached."""
    key = (tuple(schedule), planted)
    if key not in _cache:
        from oracle import oracle as O
        x = tracks()
        total = sum(schedule)
        assert total <= NSAMP
        out = [[None] * NCH for _ in schedule]
        for ch in range(NCH):
            oc = O.Channel(ch, max_bits=total, max_frames=64)
            a0 = 0
            for i, n in enumerate(schedule):
                if planted and plant_for(i, ch) is not None:
                    oc.c.MskPhi, oc.c.MskDf, oc.c.MskClk = plant_for(i, ch)
                b0, f0 = oc.c.bitlog_n, oc.c.frames_n
                oc.demod(x[ch, a0:a0 + n])
                a0 += n
                assert oc.c.bitlog_n <= total and oc.c.frames_n <= 64
                s = Snap()
                s.c = O.OrcChan.from_buffer_copy(oc.c)
                s.text = bytes(oc.c.blk_txt[: oc.c.blk_len]) if oc.c.Acarsstate in (TXT, CRC1) else b""
                vo, lvl = oc.bits
                s.vo, s.lvl = vo[b0:], lvl[b0:]
                s.blocks = [O.OrcFrame.from_buffer_copy(f) for f in oc.frames[f0:]]
                out[i][ch] = s
        _cache[key] = out
    return [row[:nch] for row in _cache[key]]


def oracle_cut(t):
    """the oracle at sample t of a free run, and one call of each SHORT length from there: (state [channel] -> Snap,
    {n: [channel] -> Snap}).  The oracle is sequential, so its state n samples on does not depend on how the samples were cut into
    calls: the call of n samples is the 32-sample pieces up to t + n put together."""
    assert 0 < t and t + max(SHORT) <= NSAMP
    run = oracle_run([t] + [32] * (max(SHORT) // 32))
    calls = {}
    for n in SHORT:
        row = []
        for ch in range(NCH):
            parts = [run[1 + k][ch] for k in range(n // 32)]
            s = Snap()
            s.c, s.text = parts[-1].c, parts[-1].text
            s.vo, s.lvl = np.concatenate([p.vo for p in parts]), np.concatenate([p.lvl for p in parts])
            s.blocks = [f for p in parts for f in p.blocks]
            row.append(s)
        calls[n] = row
    return run[0], calls


class Walk:
    """the oracle one sample at a time: phi[ch, i] = MskPhi after sample i (the phase the mixer used on it, msk.c:83-90),
    astate[ch, i], nbit[ch, i] = bits so far, pol[ch, i] = MskS & 2, last = the final OrcChan of every channel"""
    __slots__ = ("phi", "astate", "nbit", "pol", "last")


def oracle_walk(schedule, planted=False):
    """Walk over the samples of oracle_run(schedule, planted).  Cached."""
    key = ("walk", tuple(schedule), planted)
    if key not in _cache:
        from oracle import oracle as O
        x = tracks()
        total = sum(schedule)
        w = Walk()
        w.phi = np.zeros((NCH, total))
        w.astate = np.zeros((NCH, total), dtype=np.int8)
        w.nbit = np.zeros((NCH, total), dtype=np.int32)
        w.pol = np.zeros((NCH, total), dtype=np.int8)
        w.last = []
        step = O.lib().orc_demod_msk
        starts = set(np.cumsum([0] + list(schedule[:-1])).tolist())
        call_of = {int(a): i for i, a in enumerate(np.cumsum([0] + list(schedule[:-1])))}
        for ch in range(NCH):
            oc = O.Channel(ch)
            c, ref, base = oc.c, C.byref(oc.c), x[ch].ctypes.data
            phi, ast, nb, pol = w.phi[ch], w.astate[ch], w.nbit[ch], w.pol[ch]
            for i in range(total):
                if planted and i in starts and plant_for(call_of[i], ch) is not None:
                    c.MskPhi, c.MskDf, c.MskClk = plant_for(call_of[i], ch)
                step(ref, base + 4 * i, 1)
                phi[i], ast[i], nb[i], pol[i] = c.MskPhi, c.Acarsstate, c.bitlog_n, c.MskS & 2
            w.last.append(O.OrcChan.from_buffer_copy(c))
        _cache[key] = w
    return _cache[key]


# ---- the cut points of the planted runs ---------------------------------------------------------------------------------------------
def cut_points():
    """The samples at which the GPU test brings a fresh decoder to the oracle's state: the ends of the EVEN calls, plus for every
    framing state that no channel is in at any of those the first sample (a multiple of 32 if there is one) behind which a channel
    is in it.  CRC2 is left out: the held first CRC byte is not part of the public state (acg_chan_state), so a decoder cannot be
    brought there.  tests/test_msk_exact_inputs.py asserts that the cuts hit every other state and none hits CRC2."""
    if "cuts" not in _cache:
        w = oracle_walk(EVEN)
        cuts = np.cumsum(EVEN).tolist()
        for state in (WSYN, SYN2, SOH1, TXT, CRC1, END):
            if any((w.astate[:, t - 1] == state).any() for t in cuts):
                continue
            # samples t (as a count: the state behind sample t - 1) at which some channel is in `state` and none is in CRC2
            ok = np.flatnonzero((w.astate == state).any(axis=0) & ~(w.astate == CRC2).any(axis=0)) + 1
            ok = ok[ok + max(SHORT) <= NSAMP]
            assert len(ok), "no channel is ever in framing state %d" % state
            even = ok[ok % 32 == 0]
            cuts.append(int(even[0] if len(even) else ok[0]))
        _cache["cuts"] = sorted(cuts)
    return _cache["cuts"]


# ---- the premise ------------------------------------------------------------------------------------------------------------------
def products_lib():
    """tests/sincos_products.c + host_setup.c as a shared object (gcc -O2 -ffp-contract=off), built once per process"""
    if "lib" not in _cache:
        td = tempfile.mkdtemp(prefix="sincos_products_")
        atexit.register(shutil.rmtree, td, ignore_errors=True)
        so = os.path.join(td, "libsincos_products.so")
        r = subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-o", so,
                            os.path.join(ROOT, "tests", "sincos_products.c"), os.path.join(ROOT, "acarsdec_amd", "csrc", "host_setup.c"), "-lm"],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        L = C.CDLL(so)
        L.sc_products_differ.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
        L.sc_products_differ.restype = C.c_long
        L.sc_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
        L.sc_eval.restype = None
        _cache["lib"] = L
    return _cache["lib"]


def products_differing(phi, samples):
    """(how many of the 2 n mixer products differ between the device's sin/cos model and the oracle's cexp, index of the first pair)"""
    phi = np.ascontiguousarray(phi, dtype=np.float64).reshape(-1)
    samples = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
    assert phi.size == samples.size
    first = C.c_long(-1)
    bad = products_lib().sc_products_differ(phi.ctypes.data, samples.ctypes.data, phi.size, C.byref(first))
    return int(bad), int(first.value)


def model_sincos(phi):
    """(sin, cos) of tests/sincos_model.h's sc_tab as float64 arrays"""
    phi = np.ascontiguousarray(phi, dtype=np.float64).reshape(-1)
    sn, cs = np.zeros_like(phi), np.zeros_like(phi)
    products_lib().sc_eval(phi.ctypes.data, sn.ctypes.data, cs.ctypes.data, phi.size)
    return sn, cs


def visited_phases():
    """every phase the oracle's mixer sees in the runs of the GPU file: the free run and the planted calls"""
    return np.concatenate([oracle_walk([NSAMP]).phi.reshape(-1), oracle_walk(PLANT_CALLS, planted=True).phi.reshape(-1)])
