"""msk_lean.hip keeps a segment's bit records in registers (lane g of a channel's group keeps records g, g + LPC, ...) and stores
them once behind the segment's framing, turned there if the framing found a ~SYN in front of them -- instead of one 64-lane
store per bit period and a read-modify-write of global memory for the turn.  Same values at the same places: the lean kernel
against msk.hip's kernel (ACG_MSK_NOLEAN=1, which stores every record where it is made and is not touched by this) must agree bit
for bit, after every call, on the bit log (count and every record), the text rows, the channel state and the blocks; and both
against the oracle.

Shapes: 1, 8 and 9 channels (a wave of the 8-lane kernel holds 8: one group, a full wave, a second wave that replicates), at 8 and
4 lanes per channel; calls of 32, 64, 96, 160 and 8192 samples (the dm window is refilled every 64: a launch that ends before,
at and just behind a refill, and a launch shorter than one segment, which leaves through the partial-segment store); a call of three
chunks whose launches APPEND to the call's log (ACG_PIPE_BLOCKS=1); transmissions in both polarities (the ~SYN turn reaches kept
records), blocks that run on to DEL (put_frame from the text state, right behind a segment's text byte), corrupted and over-long
blocks, noise, silence.
The `nb + SEG <= bit_cap` rule cannot be crossed through the library: bit_cap = max_len / 4 + 8 records and a call of max_len
samples makes about max_len / 5.2 bits; the rule's code is unchanged and stays covered by the kernel's clamp.

Against the oracle: bit count and blocks exact, and every soft symbol of the call-by-call runs identical to the oracle's bit for
bit (about 4e5 records; the mixer's sin/cos is the one operation that is not glibc's, and it differs about once in 1e8 products,
tests/test_gpu_parity.py test_exact_order_mode_is_bit_identical_end_to_end: none falls into these inputs).  The levels, and the
appended call, whose dm comes from the down-converter, are held to that test's standing criterion (assert_soft_close, >= 0.9999
of the soft symbols identical)."""
import numpy as np
import pytest

from test_gpu_lean import snapshot, zoo_tracks
from test_gpu_parity import assert_soft_close

pytestmark = pytest.mark.gpu

LENS = [32, 64, 96, 160, 8192, 32, 8192, 64, 8192, 96, 8192, 160, 160, 8192, 64, 32, 8192]


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


def tracks(S, nch, nsamp, seed, first_kind=0):
    """[nch, nsamp] envelopes: channel c is of kind (first_kind + c) % 9 --
    0 plain traffic, 1 every transmission in the OTHER polarity (bits complemented: found as ~SYN), 2 both polarities in turn with
    noise, 3 blocks that lose their ETX and end at DEL, 4 noise, 5 silence, 6 corrupted blocks, 7 over-long blocks, 8 short blocks
    in dense succession"""
    rng = np.random.default_rng(seed)
    zoo, zk = zoo_tracks(S, 10, nsamp, seed + 1)
    zoo_of = {3: zk.index(5), 4: zk.index(6), 5: zk.index(7), 6: zk.index(1), 7: zk.index(3), 8: zk.index(9)}
    x = np.zeros((nch, nsamp), dtype=np.float32)
    kinds = []
    for c in range(nch):
        k = (first_kind + c) % 9
        kinds.append(k)
        if k in (0, 1, 2):
            parts, n, i = [np.zeros(int(rng.integers(50, 400)))], 0, 0
            while n < nsamp:
                bits = S.frame_bits(S.acars_frame(text=S.random_text(rng, 1, 60)), prekey=int(rng.integers(16, 40)))
                if k == 1 or (k == 2 and i % 2):
                    bits = 1 - bits
                parts.append(S.msk_audio(bits, phase0=float(rng.uniform(0, 2 * np.pi))))
                parts.append(np.zeros(int(rng.integers(150, 700))))
                n += parts[-1].size + parts[-2].size
                i += 1
            x[c] = S.envelope(np.concatenate(parts)[:nsamp], noise=0.02 if k == 2 else 0.0, rng=rng)
        else:
            x[c] = zoo[zoo_of[k]]
    return x, kinds


def run_calls(D, K, x, lens, bitlog=True):
    dec = D.Decoder(x.shape[0], max_blocks=8, bitlog=bitlog)
    out, a0 = [], 0
    for n in lens:
        dec.demod_msk(x[:, a0:a0 + n])
        dec.sync()
        snap = snapshot(dec, K)
        cnt, vo, lvl = dec.bits_all()
        out.append(snap + (cnt.copy(), [(vo[c, : cnt[c]].copy(), lvl[c, : cnt[c]].copy()) for c in range(x.shape[0])]))
        a0 += n
    dec.close()
    return out


@pytest.mark.parametrize("nch,first_kind,lpc", [(1, 1, 8), (1, 3, 8), (8, 0, 8), (9, 0, 8), (9, 1, 4), (1, 2, 4)])
def test_kept_records_are_the_inline_kernels_records(D, O, S, tune, nch, first_kind, lpc):
    from acarsdec_amd import _capi as K
    x, kinds = tracks(S, nch, sum(LENS), 40 + nch + first_kind, first_kind)
    tune("ACG_MSK_LPC", str(lpc))
    lean = run_calls(D, K, x, LENS)
    tune("ACG_MSK_NOLEAN", "1")
    inline = run_calls(D, K, x, LENS)
    nbits = nframes = 0
    for i, (a, b) in enumerate(zip(lean, inline)):
        assert a[0] == b[0], "call %d (%d samples): channel state" % (i, LENS[i])
        assert a[1] == b[1], "call %d: text rows" % i
        assert a[2] == b[2], "call %d: blocks" % i
        assert np.array_equal(a[3], b[3]), "call %d: bits per channel %s / %s" % (i, a[3], b[3])
        for c in range(nch):
            for j, what in ((0, "soft symbol"), (1, "level")):
                assert np.array_equal(a[4][c][j].view(np.uint32), b[4][c][j].view(np.uint32)), "call %d channel %d (kind %d): %s" % (i, c, kinds[c], what)
        nbits += int(a[3].sum())
        nframes += len(a[2])
    assert nbits > 1000 * nch
    # ... and the oracle on the same samples, call by call
    got = {}
    ident = total = 0
    for c in range(nch):
        oc = O.Channel(c, max_bits=sum(LENS) // 4 + 8, max_frames=1024)
        a0 = 0
        for n in LENS:
            oc.demod(x[c, a0:a0 + n])
            a0 += n
        vo_o, lvl_o = oc.bits
        vo_g = np.concatenate([s[4][c][0] for s in lean])
        lvl_g = np.concatenate([s[4][c][1] for s in lean])
        assert len(vo_g) == len(vo_o), (c, kinds[c])
        if kinds[c] == 5:
            assert np.all(vo_g == 0) and np.all(lvl_g == 0)
        else:
            same = (vo_g.view(np.uint32) == vo_o.view(np.uint32)).mean()
            print("channel %d kind %d: %d records, identical to the oracle's %.6f" % (c, kinds[c], len(vo_g), same))
            assert_soft_close(vo_g, vo_o, lvl_g, lvl_o)
            ident += int((vo_g.view(np.uint32) == vo_o.view(np.uint32)).sum())
            total += len(vo_g)
        got[c] = [(f.chn, f.len, f.err, bytes(f.crc), bytes(f.txt[: f.len]), f.end_bit) for f in oc.frames]
    assert ident == total, (ident, total)
    mine = {}
    for s in lean:
        for f in s[2]:
            mine.setdefault(f[0], []).append((f[0], f[2], f[3], f[5], f[6], f[1]))
    for c in range(nch):
        assert sorted(mine.get(c, [])) == sorted(got[c]), (c, kinds[c])
        if kinds[c] in (0, 1, 2, 3):
            assert len(got[c]) >= 3, (c, kinds[c], len(got[c]))          # both polarities and the DEL ending really decode


def test_kept_records_append_across_the_chunks_of_a_call(D, O, S, tune):
    """one call of three callbacks in chunks of one: the second and third launch append to the log the first began"""
    from acarsdec_amd import _capi as K
    M, nblk, nch = 160, 3, 9
    nout = nblk * 1024
    rows, taps = [], []
    env, _ = tracks(S, nch, nout, 77)
    for c in range(nch):
        off = 25000.0 * (2 + c) * (-1) ** c
        rows.append(S.iq_u8_from_envelopes(env[c][None, :].astype(np.float64), M, [off], phases=[0.37 * c], noise=0.0,
                                           rng=np.random.default_rng(500 + c)).reshape(-1))
        taps.append(O.rtl_taps(131000000 + int(off), 131000000, M))
    iq, taps = np.stack(rows), np.stack(taps)
    tune("ACG_PIPE_BLOCKS", "1")

    def go():
        dec = D.Decoder(nch, decim=M, max_blocks=nblk)
        dec.set_taps(taps)
        dec.in_callback(iq)
        dec.sync()
        snap = snapshot(dec, K)
        cnt, vo, lvl = dec.bits_all()
        dm = [dec.dm(c, nout) for c in range(nch)]
        dec.close()
        return snap, cnt, vo, lvl, dm

    lean = go()
    tune("ACG_MSK_NOLEAN", "1")
    inline = go()
    assert lean[0] == inline[0]
    assert np.array_equal(lean[1], inline[1]) and int(lean[1].min()) > nout // 6
    for c in range(nch):
        n = lean[1][c]
        assert np.array_equal(lean[2][c, :n].view(np.uint32), inline[2][c, :n].view(np.uint32)), c
        assert np.array_equal(lean[3][c, :n].view(np.uint32), inline[3][c, :n].view(np.uint32)), c
        oc = O.Channel(c, max_bits=nout // 4 + 8)
        oc.demod(lean[4][c])
        vo_o, lvl_o = oc.bits
        assert len(vo_o) == n, c
        if np.any(lvl_o != 0):
            assert_soft_close(lean[2][c, :n], vo_o, lean[3][c, :n], lvl_o)
            assert (lean[2][c, :n].view(np.uint32) == vo_o.view(np.uint32)).mean() >= 0.9999, c
