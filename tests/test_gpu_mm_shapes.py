"""The matrix-pipe down-converters (acarsdec_amd/csrc/fir_mm.hip) held to EQUALITY with their arithmetic (tests/mm_model.py) on
every output, in every launch shape the library selects: fir_u8_mm_kernel<CPR, 1> under the CU partition, <CPR, 2> as a context
without a partition picks it (the production instantiation of wide contexts), <CPR, 2> on 8 CUs where few groups still give long
runs and ticket draws; end to end beside the demodulator; and fir_u8_mm1_kernel.  Which instantiation a launch takes and how it is
cut into runs is asked of the launcher itself (acg_lab_fir_launch_shape), so every test knows it reached the shape it names.

The 2e-7 bar of tests/test_gpu_round6.py cannot tell one rounding from two (tests/test_mm_model.py); equality can."""
import numpy as np
import pytest

import mm_model as MM

pytestmark = pytest.mark.gpu

SHAPES = [(200, 200), (160, 160), (192, 192), (200, 192), (160, 37)]
SIZES = [1, 3, 8, 11, 16, 1]                     # channels per stream: groups of 1, 3, 8, 8 + 3, 8 + 8, 1 channels
NBLK = 8                                         # callbacks a stream holds = the contexts' max_blocks
CALLS = [(0, 1), (1, 2), (3, 3), (2, 5), (1, 7), (0, 8)]      # (first callback, callbacks) of consecutive calls
SWAP_AFTER = 3                                   # the tap tables are replaced before this call
ARRANGEMENTS = ["partition", "whole", "cus8"]
ZERO_CH, RTL_EXCEPT = 11, (3, 5, 7, 11, 13)


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


@pytest.fixture(scope="module")
def S():
    from acarsdec_amd import synth
    return synth


@pytest.fixture(scope="module")
def device_cus(D):
    dec = D.Decoder(2, decim=160, nstreams=1, max_blocks=1)
    n = int(dec.launch_shape(1).device_cus)
    dec.close()
    assert n > 16
    return n


def arrange(tune, name, device_cus):
    """the switches of one arrangement, set before the context is made; one call is one launch in all of them"""
    tune("ACG_PIPE_BLOCKS", "0")
    if name == "whole":
        tune("ACG_MSK_CUS", "0")                      # no CU partition: the library itself takes <CPR, 2>
    elif name == "cus8":
        tune("ACG_MSK_CUS", str(device_cus - 8))      # the down-converter keeps 8 CUs ...
        tune("ACG_FIR_MM_STAGES", "2")                # ... and runs two tiles in flight on them
    else:
        assert name == "partition"


def shape_dict(s):
    return {f: int(getattr(s, f)) for f, _ in s._fields_}


REGIMES = {
    "an odd run length >= 3": lambda s: s["tiles_per_run"] >= 3 and s["tiles_per_run"] % 2 == 1,
    "a run length >= 16": lambda s: s["tiles_per_run"] >= 16,
    "more runs than waves (tickets carry work)": lambda s: s["runs"] > s["waves"],
    "fewer runs than the waves the launch is sized for (the grid is cut, every ticket is empty)": lambda s: s["runs"] < s["wave_slots"],
}


def frozen(a):
    a.setflags(write=False)
    return a


_CASES = {}


def case(O, M, ntaps):
    """input, tap tables, model and references of one (M, ntaps): made once, shared by the arrangements, read-only"""
    key = (M, ntaps)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(9000 * M + ntaps)
    smap = np.repeat(np.arange(len(SIZES)), SIZES)
    rng.shuffle(smap)
    nch, nout, row = int(smap.size), NBLK * 1024, 1024 * M * 2
    iq = rng.integers(0, 256, size=(len(SIZES), NBLK * row), dtype=np.uint8)
    for k in range(NBLK):                            # runs of 0 / 255 / 128 / alternating 255, 0 in every callback, across tile edges
        s, at = k % len(SIZES), k * row + (29 + 3 * k) * 2 * M
        iq[s, at: at + 6 * M] = 0
        iq[(s + 1) % 6, at: at + 6 * M] = 255
        iq[(s + 2) % 6, at + M: at + 5 * M] = 128
        iq[(s + 4) % 6, at: at + 8 * M: 2] = 255
        iq[(s + 4) % 6, at + 1: at + 8 * M: 2] = 0
    iq[0, : 4 * M] = 0
    iq[1, : 4 * M] = 255
    iq[2, : 2 * M] = 128
    taps = np.zeros((nch, ntaps, 2), dtype=np.float32)
    for c in range(nch):
        taps[c] = O.rtl_taps(131000000 + 25000 * int(rng.integers(-40, 41)), 131000000, M)[:ntaps]
    taps[3] *= np.float32(2.0 ** -9)                 # a table 2^9 below the others: its own scale
    taps[7] *= np.float32(2.0 ** -40)                # ... and one 2^40 below
    taps[5, 1::2] = 0                                # exact zeros inside a table
    taps[ZERO_CH] = 0                                # an all-zero table: +0.0
    taps[13, 17] *= np.float32(4096.0)               # one tap 2^12 above the rest: the others are cut at 2^-31 of it
    sets = [taps, taps[::-1].copy()]
    model = np.zeros((2, nch, nout), dtype=np.float32)
    for t, tp in enumerate(sets):
        for s in range(len(SIZES)):
            chs = np.flatnonzero(smap == s)
            model[t, chs] = MM.model_dm_many(iq[s], M, [tp[c] for c in chs], nout)
    # the two bars the kernels already carry, on the plain rtl tables: the model itself sits inside them
    rtl = [[c for c in range(nch) if (c if t == 0 else nch - 1 - c) not in RTL_EXCEPT] for t in range(2)]
    exact, oracle = {}, {}
    for t, tp in enumerate(sets):
        for c in rtl[t]:
            exact[t, c] = frozen(MM.exact_dm(iq[smap[c]], M, tp[c], nout))
            oracle[t, c] = frozen(O.fir_u8(iq[smap[c]], M, tp[c], nout=nout, ntaps=ntaps))
    _CASES[key] = dict(smap=frozen(smap), iq=frozen(iq), sets=[frozen(x) for x in sets], model=frozen(model), rtl=rtl, exact=exact,
                       oracle=oracle, nch=nch, row=row)
    return _CASES[key]


def check_call(cs, t, got, w0, n, chans, where):
    """got [len(chans), n] against the model bit for bit; on the rtl tables against the f64-exact value and the oracle as well.
    Returns the worst relative distance from the f64-exact value."""
    worst = 0.0
    for i, c in enumerate(chans):
        want = cs["model"][t, c, w0: w0 + n]
        bad = np.flatnonzero(got[i].view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (where, "channel", c, "outputs that differ", int(bad.size), "first", int(bad[0]),
                               float(got[i][bad[0]]), float(want[bad[0]]))
        if (t, c) in cs["exact"]:
            ex, orc = cs["exact"][t, c][w0: w0 + n], cs["oracle"][t, c][w0: w0 + n]
            err = np.abs(got[i].astype(np.float64) - ex)
            assert np.all(err <= 2e-7 * ex + 1e-9), (where, c, float((err / (ex + 1e-9)).max()))
            assert np.all(np.abs(got[i] - orc) <= 1e-5 * np.abs(orc) + 1e-6), (where, c)
            worst = max(worst, float((err / (ex + 1e-3)).max()))
    return worst


@pytest.mark.parametrize("arr", ARRANGEMENTS)
@pytest.mark.parametrize("M,ntaps", SHAPES)
def test_shared_stream_kernel_equals_the_model(D, O, tune, device_cus, M, ntaps, arr):
    """fir_u8_mm_kernel: six streams feeding 1, 3, 8, 11, 16 and 1 channels in scrambled channel order; runs of 0, 255, 128 and
    alternating 255 / 0; rtl tables, tables scaled by 2^-9 and 2^-40, one with exact zeros, an all-zero one (+0.0), one whose
    largest tap is 2^12 above the rest.  ONE context, consecutive calls of 1, 2, 3, 5, 7, 8 callbacks over different stretches of
    the streams (the run dispenser re-arms itself between launches of different shapes), the tap tables replaced on the way.
    EVERY output of every channel equals tests/mm_model.py bit for bit; on the rtl tables the 2e-7 and 1e-5 bars hold besides.
    The launcher says which instantiation ran: <CPR, 1> under the partition, <CPR, 2> without one (chosen by the library) and on
    8 CUs -- and that the two-stage launches reach the steady-state pipeline: odd runs of >= 3 tiles and a grid cut to the runs
    (no partition: 3 / 5 / 7 callbacks over 8 groups), runs of >= 16 tiles handed out by ticket (8 CUs: 8 callbacks)."""
    cs = case(O, M, ntaps)
    arrange(tune, arr, device_cus)
    nch, row = cs["nch"], cs["row"]
    dec = D.Decoder(nch, decim=M, ntaps=ntaps, nstreams=len(SIZES), max_blocks=NBLK)
    dec.set_taps(cs["sets"][0])
    dec.set_channel_streams(cs["smap"])
    shapes, worst = [], 0.0
    for k, (b0, nb) in enumerate(CALLS):
        t = int(k >= SWAP_AFTER)
        if k == SWAP_AFTER:
            dec.set_taps(cs["sets"][1])                  # the digit images must follow the tap tables
        s = shape_dict(dec.launch_shape(nb))
        shapes.append(s)
        assert s["kernel"] == 1 and s["cpr"] == M // 8 and s["chunk_blocks"] == 0 and s["units"] == 8, s
        assert s["stages"] == (1 if arr == "partition" else 2), s
        assert (s["ncu"] == 8) if arr == "cus8" else (s["ncu"] == device_cus) if arr == "whole" else (8 < s["ncu"] < device_cus), s
        assert s["runs"] == s["units"] * s["runs_per_unit"] and s["tiles_per_run"] * s["runs_per_unit"] == nb * 32, s
        dec.in_callback(np.ascontiguousarray(cs["iq"][:, b0 * row: (b0 + nb) * row]), nblocks=nb)
        got = np.stack([dec.dm(c, nb * 1024) for c in range(nch)])
        worst = max(worst, check_call(cs, t, got, b0 * 1024, nb * 1024, range(nch), (arr, "call", k, s)))
        z = got[ZERO_CH if t == 0 else nch - 1 - ZERO_CH]
        assert np.array_equal(z.view(np.uint32), np.zeros(z.size, np.uint32))           # +0.0, not -0.0
    dec.close()
    print("%s M=%d ntaps=%d: worst relative distance from the f64-exact value %.3e; tiles per run %s, runs / waves %s" % (
        arr, M, ntaps, worst, [s["tiles_per_run"] for s in shapes], [(s["runs"], s["waves"]) for s in shapes]))
    want = {"whole": (0, 3), "cus8": (1, 2), "partition": ()}[arr]
    for i in want:
        name = list(REGIMES)[i]
        assert any(REGIMES[name](s) for s in shapes), ("not reached with two tiles in flight: " + name, shapes)


@pytest.mark.parametrize("M", [160, 192, 200])
def test_two_stage_launches_reach_every_pipeline_regime(D, tune, device_cus, M):
    """The launches test_shared_stream_kernel_equals_the_model makes with two tiles in flight (no partition; 8 CUs), as the
    launcher cuts them: together they include an odd run length >= 3, a run length >= 16, a launch with more runs than waves
    and one with fewer runs than the waves it is sized for.  A regime that is not reached fails here -- the equality test would
    otherwise pass without having been where it claims."""
    smap = np.repeat(np.arange(len(SIZES)), SIZES)
    seen = []
    for arr in ("whole", "cus8"):
        arrange(tune, arr, device_cus)
        dec = D.Decoder(int(smap.size), decim=M, nstreams=len(SIZES), max_blocks=NBLK)
        dec.set_channel_streams(smap)
        for _, nb in CALLS:
            s = shape_dict(dec.launch_shape(nb))
            assert s["kernel"] == 1 and s["stages"] == 2 and s["cpr"] == M // 8 and s["chunk_blocks"] == 0, (arr, s)
            seen.append((arr, nb, s))
        dec.close()
    for name, reached in REGIMES.items():
        assert any(reached(s) for _, _, s in seen), ("not reached with two tiles in flight: " + name, seen)


@pytest.mark.parametrize("M,ntaps", [(200, 200), (160, 160), (192, 192)])
def test_odd_runs_handed_out_by_ticket(D, O, tune, device_cus, M, ntaps):
    """Two tiles in flight on 8 CUs with FOUR groups (the streams that feed 1, 3 and 11 channels): the launcher is asked which of
    7, 5 or 3 callbacks gives an odd run of >= 3 tiles with more runs than waves (7: 7-tile runs, 128 runs for 32 waves on a
    256-CU device) -- the last tile of every run goes through the first register stage alone, on runs that came from the ticket
    counter.  Every output equals the model."""
    cs = case(O, M, ntaps)
    arrange(tune, "cus8", device_cus)
    streams = [s for s, n in enumerate(SIZES) if n in (3, 11)] + [SIZES.index(1)]
    chans = [c for c in range(cs["nch"]) if cs["smap"][c] in streams]
    sub = sorted(streams)
    dec = D.Decoder(len(chans), decim=M, ntaps=ntaps, nstreams=len(sub), max_blocks=NBLK)
    dec.set_taps(cs["sets"][0][chans])
    dec.set_channel_streams([sub.index(cs["smap"][c]) for c in chans])
    tried = []
    for nb in (7, 5, 3):
        s = shape_dict(dec.launch_shape(nb))
        tried.append(s)
        if s["tiles_per_run"] >= 3 and s["tiles_per_run"] % 2 == 1 and s["runs"] > s["waves"]:
            break
    else:
        pytest.fail("no candidate gives odd runs handed out by ticket: %r" % (tried,))
    assert s["kernel"] == 1 and s["stages"] == 2 and s["units"] == 4 and s["ncu"] == 8 and s["chunk_blocks"] == 0, s
    row, b0 = cs["row"], NBLK - nb
    for rep in range(2):                                 # twice: the second launch finds the dispenser re-armed by the first
        dec.in_callback(np.ascontiguousarray(cs["iq"][sub][:, b0 * row: (b0 + nb) * row]), nblocks=nb)
        got = np.stack([dec.dm(i, nb * 1024) for i in range(len(chans))])
        check_call(cs, 0, got, b0 * 1024, nb * 1024, chans, ("4 groups", rep, s))
    dec.close()


# ---- end to end beside the demodulator ------------------------------------------------------------------------------------------
_TRAFFIC = {}


def traffic(O, S, M):
    if M in _TRAFFIC:
        return _TRAFFIC[M]
    rng = np.random.default_rng(660 + M)
    nch, nblk = 16, 6
    nout = nblk * 1024
    fr = [131.0e6 + 25000.0 * k for k in (-20, -14, -9, -6, -4, -2, 2, 3, 5, 7, 9, 12, 15, 18, 21, 24)]
    fc = 131.0e6
    env = []
    for c in range(nch):
        a, _ = S.channel_audio(rng, nout, nframes=2, gap=(800, 1500), text_len=(10, 40))
        env.append(0.5 * (1 + 0.5 * a))
    iq = S.iq_u8_from_envelopes(np.array(env), M, [f - fc for f in fr], phases=list(rng.uniform(0, 6.28, nch)), noise=0.004, rng=rng,
                                scale=0.06)
    iq = np.ascontiguousarray(iq, dtype=np.uint8).reshape(1, -1)
    taps = np.stack([O.rtl_taps(int(f), int(fc), M) for f in fr])
    model = MM.model_dm_many(iq[0], M, list(taps), nout)
    _TRAFFIC[M] = (frozen(iq), frozen(taps), frozen(model))
    return _TRAFFIC[M]


@pytest.mark.parametrize("pipe", [None, 4])
@pytest.mark.parametrize("M", [160, 192])
def test_one_dongle_sixteen_channels_without_a_partition(D, O, S, tune, M, pipe):
    """rtlMult 160 (the reference's default) and 192, one dongle, 16 channels of synthetic ACARS traffic, NO CU partition
    (ACG_MSK_CUS=0: fir_u8_mm_kernel<20, 2> / <24, 2> beside the demodulator on the same CUs), whole calls and chunks of 4
    callbacks; six callbacks handed over as [6], [1] x 6 and [3, 2, 1].  dm and blocks are identical bit for bit across the
    chunkings, dm equals the model, the blocks are the oracle demodulator's on the GPU's dm, every channel delivers a block."""
    iq, taps, model = traffic(O, S, M)
    nch, row = 16, 1024 * M * 2
    tune("ACG_MSK_CUS", "0")
    if pipe is not None:
        tune("ACG_PIPE_BLOCKS", str(pipe))

    def run(chunks):
        dec = D.Decoder(nch, decim=M, nstreams=1, max_blocks=6)
        dec.set_taps(taps)
        for nb in set(chunks):
            s = shape_dict(dec.launch_shape(min(nb, pipe or nb)))
            assert s["kernel"] == 1 and s["stages"] == 2 and s["cpr"] == M // 8 and s["chunk_blocks"] == (pipe or 0), s
        dms, b0 = [], 0
        for nb in chunks:
            dec.in_callback(np.ascontiguousarray(iq[:, b0 * row: (b0 + nb) * row]), nblocks=nb)
            dms.append(np.stack([dec.dm(c, nb * 1024) for c in range(nch)]))
            b0 += nb
        got = {}
        for f in dec.drain_frames():
            got.setdefault(int(f.chn), []).append(D.frame_tuple(f))
        dec.close()
        return got, np.concatenate(dms, axis=1)

    runs = [run(ch) for ch in ([6], [1] * 6, [3, 2, 1])]
    got, dm = runs[0]
    for g2, d2 in runs[1:]:
        assert g2 == got and np.array_equal(d2.view(np.uint32), dm.view(np.uint32))
    assert np.array_equal(dm.view(np.uint32), model.view(np.uint32)), int(np.count_nonzero(dm.view(np.uint32) != model.view(np.uint32)))
    for c in range(nch):
        ch = O.Channel(c)
        ch.demod(dm[c])                                    # the oracle's demodulator on the GPU's dm: exact
        want = [O.frame_tuple(f) for f in ch.frames]
        assert got.get(c, []) == want, c
        assert len(want) >= 1, c


# ---- one stream per channel -----------------------------------------------------------------------------------------------------
_MM1 = {}


def mm1_case(O, M):
    """37 channels, one stream each (one entry kept: 8 callbacks of 37 streams are ~100 MB)"""
    if M in _MM1:
        return _MM1[M]
    _MM1.clear()
    rng = np.random.default_rng(3700 + M)
    nch, nout, row = 37, NBLK * 1024, 1024 * M * 2
    iq = rng.integers(0, 256, size=(nch, NBLK * row), dtype=np.uint8)
    iq[0, : 4 * M] = 0
    iq[1, 3 * row + 62 * M: 3 * row + 70 * M] = 255
    iq[2, 7 * row - 4 * M: 7 * row + 4 * M] = 128
    iq[4, row: row + 8 * M: 2] = 255
    iq[4, row + 1: row + 8 * M: 2] = 0
    taps = np.zeros((nch, M, 2), dtype=np.float32)
    for c in range(nch):
        taps[c] = O.rtl_taps(131000000 + 25000 * int(rng.integers(-40, 41)), 131000000, M)
    taps[3] *= np.float32(2.0 ** -9)
    taps[5, ::2] = 0
    taps[ZERO_CH] = 0
    perm = rng.permutation(nch)
    model = np.stack([MM.model_dm(iq[perm[c]], M, taps[c], nout) for c in range(nch)])
    _MM1[M] = (frozen(iq), frozen(taps), frozen(perm), frozen(model))
    return _MM1[M]


@pytest.mark.parametrize("waves", [1, 12])
@pytest.mark.parametrize("arr", ["partition", "whole"])
@pytest.mark.parametrize("M", [160, 192, 200])
def test_one_stream_per_channel_kernel_equals_the_model(D, O, tune, device_cus, M, arr, waves):
    """fir_u8_mm1_kernel (ACG_FIR_MM1=1): its recombination is the shared-stream kernel's expression, so it is held to the same
    model.  37 channels on scrambled streams, calls of 1, 4 and 8 callbacks in one context, under the CU partition and without
    one, with 1 and 12 waves per CU (1: more runs than waves, handed out by ticket): every output equals the model."""
    iq, taps, perm, model = mm1_case(O, M)
    nch, row = 37, 1024 * M * 2
    arrange(tune, arr, device_cus)
    tune("ACG_FIR_MM1", "1")
    tune("ACG_FIR_MM1_WAVES", str(waves))
    dec = D.Decoder(nch, decim=M, nstreams=nch, max_blocks=NBLK)
    dec.set_taps(taps)
    dec.set_channel_streams(perm)
    for b0, nb in ((5, 1), (2, 4), (0, 8)):
        s = shape_dict(dec.launch_shape(nb))
        assert s["kernel"] == 2 and s["cpr"] == M // 8 and s["units"] == nch and s["chunk_blocks"] == 0, s
        assert s["wave_slots"] == s["ncu"] * waves and (arr == "partition") == (s["ncu"] < device_cus), s
        dec.in_callback(np.ascontiguousarray(iq[:, b0 * row: (b0 + nb) * row]), nblocks=nb)
        for c in range(nch):
            got, want = dec.dm(c, nb * 1024), model[c, b0 * 1024: (b0 + nb) * 1024]
            bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, (arr, waves, nb, "channel", c, int(bad.size), int(bad[0]), s)
    dec.close()
