"""How often a segment of msk_lean.hip is cut short, and by what, on traffic as the bench builds it -- a CPU model, no GPU:
python profiles/probe/lean_segment_stats.py [waves] [seconds per channel] [channels per wave]

The oracle's demodulator (oracle.Channel, one sample per demod() call, so that the framing state in front of every bit can be
read) runs over synth.channel_audio as benchlib/case.py calls it (gap (3125, 12500), text of 20-220 characters, AM depth 0.5) with
envelope noise for 20 dB in the channel.  The channels of a wave then go through the kernel's rule period by period: at the start
of a segment a channel may let `lim` bits wait -- all 8 from a state in which the next possible reset of the loop is at least a
byte away (`safe`: WSYN, TXT away from its limits, CRC1), else up to the bit before its byte closes (nbits - 1) --, the segment runs
while every channel of the wave may (the ballot), and the period that a channel cannot let wait is the "tail": framing inline, the
way msk.hip does it, and a new segment behind it.  Printed: periods, segments, tails, and for every tail the state of the channel
that forced it.  (A period is one bit of every channel of the wave: the model leaves out the call boundaries and the rare period
in which a channel's clock does not fire.)"""
import os
import sys
from collections import Counter

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
from acarsdec_amd import synth as S
from oracle import oracle as O

WSYN, SYN2, SOH1, TXT, CRC1, CRC2, END = range(7)
NAMES = ["WSYN", "SYN2", "SOH1", "TXT", "CRC1", "CRC2", "END"]
MAXPERR, SEG = 3, 8
CARRIER, DEPTH, SNR_DB = 0.5, 0.5, 20.0


def states_before_bits(x, ch):
    """[(Acarsstate, nbits, blk_err, blk_len)] in front of every bit the oracle decides on the samples x"""
    oc = O.Channel(ch, max_frames=4096)
    c = oc.c
    out = []
    before = (c.Acarsstate, c.nbits, c.blk_err, c.blk_len)
    nb = c.nbit_total
    for i in range(x.size):
        oc.demod(x[i:i + 1])
        if c.nbit_total != nb:
            assert c.nbit_total == nb + 1
            out.append(before)
            nb = c.nbit_total
        before = (c.Acarsstate, c.nbits, c.blk_err, c.blk_len)
    return out


def lim_of(s):
    a, nbits, berr, blen = s
    safe = (a == WSYN or (a == TXT and berr <= MAXPERR and blen <= 239) or a == CRC1) and 1 <= nbits <= 8
    return SEG if safe else nbits - 1


def wave_stats(rows):
    """rows: per channel of the wave the list of states before its bits"""
    nbit = min(len(r) for r in rows)
    t = periods = segments = tails = 0
    why = Counter()
    while t < nbit:
        lims = [lim_of(r[t]) for r in rows]
        c = max(0, min(SEG, min(lims), nbit - t))
        segments += 1
        periods += c
        t += c
        if c < SEG and t < nbit:
            # the channel whose bit cannot wait closes the segment: framing inline
            j = int(np.argmin(lims))
            a = rows[j][t][0]
            why[NAMES[a] if a != TXT else "TXT at its limits"] += 1
            tails += 1
            periods += 1
            t += 1
    return periods, segments, tails, why


def main():
    waves = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    secs = float(sys.argv[2]) if len(sys.argv) > 2 else 12.0
    cpw = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    n = int(secs * O.INTRATE)
    sigma = CARRIER * 10 ** (-SNR_DB / 20) / 2 ** 0.5        # the in-phase part of noise 20 dB under the carrier
    tot = [0, 0, 0]
    why = Counter()
    for w in range(waves):
        rows = []
        for i in range(cpw):
            ch = w * cpw + i
            rng = np.random.default_rng(0xACA25 + ch)
            a, _ = S.channel_audio(rng, n, gap=(3125, 12500), text_len=(20, 220))
            rows.append(states_before_bits(S.envelope(a, depth=DEPTH, carrier=CARRIER, noise=sigma, rng=rng), ch))
        p, s, t, y = wave_stats(rows)
        tot[0] += p; tot[1] += s; tot[2] += t
        why.update(y)
    p, s, t = tot
    print("waves %d x %d channels, %.1f s per channel, envelope noise sigma %.4f" % (waves, cpw, secs, sigma))
    print("periods %d  segments %d  tails %d" % (p, s, t))
    print("periods per segment %.2f of %d; %.1f %% of the segments cut short; one period in %.1f is a tail" % (
        p / s, SEG, 100.0 * t / s, p / max(t, 1)))
    for k, v in why.most_common():
        print("  cut by a channel in %-17s %6d  (%.1f %%)" % (k, v, 100.0 * v / max(t, 1)))


if __name__ == "__main__":
    main()
