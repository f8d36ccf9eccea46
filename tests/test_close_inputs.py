"""Inputs for tests/test_gpu_lean_closes.py, and the proof on the CPU that they visit what that test is about.

msk_lean.hip runs its bit periods in segments of up to 8 whose framing waits; a channel whose next byte close could reset the loop
(SYN2, SOH1, CRC2, END, TXT next to its limits) lets only the bits in front of that close wait, and the period of the close is
taken msk.hip's way, through frame_bit() (msk_common.h).  The closes that do this all the time on idle channels -- the byte behind a
false sync -- are framed there by selects; the rest goes through decode_acars().  Which exit of the unrolled segment loop such a
period leaves by is the number of periods that waited in front of it, 0..7.

The tracks, 16 channels x 16384 samples (two calls of 8192), seeded: noise only (false SYN / ~SYN all the time), frames cut behind a
damaged second SYN, SYN followed by ~SYN, frames cut behind a damaged SOH, good short frames (CRC2 and END closes), frames whose
terminator is lost so that they end at DLE after more than 20 characters, each kind in both polarities, frame starts staggered by
one bit from channel to channel, silence and a constant.  The oracle (oracle.Channel, one sample per demod() call, so that the
framing state around every bit can be read) and the kernel's segment rule for the 8 channels of a wave then say at which exit every
close falls, and every one of {SYN2 miss, SYN2 ~SYN, SYN2 -> SOH1, SOH1 miss, END} must occur at each of the eight exits."""
import numpy as np

import msk_exact_inputs as X

NCH = 16
CALLS = [8192, 8192]
RAGGED = [8192, 4096]                      # a close on a call boundary: the second call starts inside the traffic
NSAMP = sum(CALLS)
SEED = 20261101
NOISE, SILENT, CONSTANT = (0, 8), 7, 15    # one noise channel in each wave of eight
WSYN, SYN2, SOH1, TXT, CRC1, CRC2, END = range(7)
CATEGORIES = ["SYN2 miss", "SYN2 ~SYN", "SYN2 -> SOH1", "SOH1 miss", "END"]
MAXPERR, SEG = 3, 8
_cache = {}


def tracks():
    """[NCH, NSAMP] float32 envelopes at 12.5 kHz, read-only, the same array for every caller"""
    if "x" in _cache:
        return _cache["x"]
    from acarsdec_amd import synth as S
    rng = np.random.default_rng(SEED)
    x = np.zeros((NCH, NSAMP), dtype=np.float32)
    head = bytes(S.odd_parity(b) for b in (ord("+"), ord("*")))
    syn, nsyn = bytes([0x16]), bytes([0xE9])

    def event(kind):
        if kind == 0:                                   # the second SYN damaged: SYN2 miss
            return head + syn + bytes([0x16 ^ (1 << int(rng.integers(0, 8)))]) + bytes(rng.integers(0, 256, size=2).astype(np.uint8).tolist())
        if kind == 1:                                   # SYN, ~SYN: the polarity turns in SYN2, and the byte behind it decides again
            return head + syn + nsyn + (nsyn if rng.integers(0, 2) else syn) + bytes([0xFE])
        if kind == 2:                                   # the SOH damaged: SYN2 -> SOH1, SOH1 miss
            return head + syn + syn + bytes([0x01 ^ (1 << int(rng.integers(0, 8)))]) + bytes([0x55])
        if kind == 3:                                   # a good frame: TXT, CRC1, CRC2, END
            return S.acars_frame(text=S.random_text(rng, 1, 6))
        fr = bytearray(S.acars_frame(text=S.random_text(rng, 12, 20)))     # 13 bytes of header: more than 20 characters at DLE
        fr[len(fr) - 4] = S.odd_parity(0x41 + int(rng.integers(0, 26)))     # the terminator becomes a letter: the block ends at DLE
        return bytes(fr)

    nev = 0
    for c in range(NCH):
        if c in NOISE:
            x[c] = rng.normal(0.5, 0.2, size=NSAMP).astype(np.float32)
        elif c == SILENT:
            x[c] = 0.0
        elif c == CONSTANT:
            x[c] = 0.37
        else:
            parts = [np.zeros(int(round(c * S.INTRATE / 2400.0)))]          # starts staggered by one bit from channel to channel
            n = len(parts[0])
            i = c
            while True:
                a = S.msk_audio(S.frame_bits(event((0, 1, 2, 3, 0, 1, 2, 4)[i % 8]), prekey=32 + (i // 8 + c) % 8, tail=8), phase0=float(rng.uniform(0, 2 * np.pi)))
                gap = int(rng.integers(30, 160))
                if n + len(a) + gap > NSAMP:
                    break
                parts += [a, np.zeros(gap)]
                n += len(a) + gap
                i += 1
                nev += 1
            a = np.concatenate(parts + [np.zeros(NSAMP - n)])
            x[c] = S.envelope(-a if c % 2 else a, noise=0.01 if c % 3 == 0 else 0.0, rng=rng)
    assert np.isfinite(x).all() and nev > 200
    x.setflags(write=False)
    _cache["x"] = x
    return x


def oracle_run(schedule):
    """the oracle over tracks() in calls of the lengths `schedule`: [call][channel] -> msk_exact_inputs.Snap.  Cached."""
    key = tuple(schedule)
    if key not in _cache:
        from oracle import oracle as O
        x = tracks()
        out = [[None] * NCH for _ in schedule]
        for ch in range(NCH):
            oc = O.Channel(ch, max_bits=NSAMP, max_frames=256)
            a0 = 0
            for i, n in enumerate(schedule):
                b0, f0 = oc.c.bitlog_n, oc.c.frames_n
                oc.demod(x[ch, a0:a0 + n])
                a0 += n
                assert oc.c.frames_n <= 256
                s = X.Snap()
                s.c = O.OrcChan.from_buffer_copy(oc.c)
                s.text = bytes(oc.c.blk_txt[: oc.c.blk_len]) if oc.c.Acarsstate in (TXT, CRC1) else b""
                vo, lvl = oc.bits
                s.vo, s.lvl = vo[b0:], lvl[b0:]
                s.blocks = [O.OrcFrame.from_buffer_copy(f) for f in oc.frames[f0:]]
                out[i][ch] = s
        _cache[key] = out
    return _cache[key]


def bit_states():
    """[call][channel] -> [(Acarsstate, nbits, blk_err, blk_len) in front of the bit, Acarsstate behind it, MskS & 2 turned by it]"""
    if "bits" in _cache:
        return _cache["bits"]
    from oracle import oracle as O
    x = tracks()
    out = [[None] * NCH for _ in CALLS]
    for ch in range(NCH):
        oc = O.Channel(ch, max_frames=256)
        c = oc.c
        a0 = 0
        for i, n in enumerate(CALLS):
            row = []
            for j in range(a0, a0 + n):
                before = (c.Acarsstate, c.nbits, c.blk_err, c.blk_len)
                nb, s = c.nbit_total, c.MskS
                oc.demod(x[ch, j:j + 1])
                if c.nbit_total != nb:
                    assert c.nbit_total == nb + 1
                    row.append((before, c.Acarsstate, ((c.MskS ^ (s + 1)) & 2) != 0))
            out[i][ch] = row
            a0 += n
    _cache["bits"] = out
    return out


def category(bit):
    """which of CATEGORIES the bit closes, or None"""
    (a, nbits, _, _), after, turned = bit
    if nbits != 1:
        return None
    if a == SYN2:
        return "SYN2 -> SOH1" if after == SOH1 else ("SYN2 ~SYN" if after == SYN2 and turned else ("SYN2 miss" if after == WSYN else None))
    if a == SOH1 and after == WSYN:
        return "SOH1 miss"
    return "END" if a == END else None


def lim_of(before):
    """how many bits of a channel may wait at the start of a segment (msk_lean.hip: `safe`, `lim`)"""
    a, nbits, berr, blen = before
    safe = (a == WSYN or (a == TXT and berr <= MAXPERR and blen <= 239) or a == CRC1) and 1 <= nbits <= 8
    return SEG if safe else nbits - 1


def closes_by_exit(lanes=range(8)):
    """{(category, exit)}: count of closes over the waves of eight channels, both calls"""
    bits = bit_states()
    seen = {}
    for call in range(len(CALLS)):
        for w0 in range(0, NCH, 8):
            rows = [bits[call][w0 + i] for i in lanes]
            nbit = min(len(r) for r in rows)
            t = 0
            while t < nbit:
                c = max(0, min(SEG, min(lim_of(r[t][0]) for r in rows), nbit - t))
                t += c
                if c < SEG and t < nbit:
                    for r in rows:
                        k = category(r[t])
                        if k:
                            seen[(k, c)] = seen.get((k, c), 0) + 1
                    t += 1
    return seen


def test_every_close_occurs_at_every_exit_of_the_segment_loop():
    seen = closes_by_exit()
    missing = [(k, e) for k in CATEGORIES for e in range(SEG) if not seen.get((k, e))]
    assert not missing, (missing, seen)
    assert set(seen) <= {(k, e) for k in CATEGORIES for e in range(SEG)}


def test_the_tracks_reach_the_other_closes_too():
    """blocks from the good frames (CRC2 close) and from the frames that end at DLE with more than 20 characters; both polarities;
    the silent and the constant channel decide bits and never leave WSYN... or whatever the reference makes of them"""
    snaps = oracle_run(CALLS)
    blocks = [f for row in snaps for s in row for f in s.blocks]
    assert len(blocks) > 40
    assert any(f.len > 20 for f in blocks) and any(f.len <= 20 for f in blocks)
    assert {f.chn % 2 for f in blocks} == {0, 1}
    for ch in (SILENT, CONSTANT):
        assert all(len(row[ch].vo) > 1000 for row in snaps) and not any(row[ch].blocks for row in snaps)
    # the ragged schedule cuts the same stream elsewhere: the same blocks in all
    rag = [X.frame_key(f) for row in oracle_run(RAGGED) for s in row for f in s.blocks]
    assert rag and set(rag) <= {X.frame_key(f) for f in blocks}


def test_a_close_falls_next_to_the_ragged_call_boundary():
    """at the cut of RAGGED (sample 8192 is the end of CALLS' first call too) some channel stands in front of a byte close that
    cannot wait: the first segment of the next call is a short one"""
    edge = [s.c for s in oracle_run(RAGGED)[0]]
    assert any(c.Acarsstate in (SYN2, SOH1, CRC2, END) for c in edge), [(c.Acarsstate, c.nbits) for c in edge]
