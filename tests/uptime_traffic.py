"""Inputs of the uptime tests (tests/test_uptime_inputs.py, tests/test_gpu_uptime.py): one piece of traffic, the counter values a
decoder reaches after days of running, and the oracle's run over that traffic with its counters preset.

2^31 samples at 12.5 kHz are 47.7 hours, 2^32 samples 95.4 hours, 2^31 bits 10.4 days.  A sample base is what nsamp_total holds
before the first call, a bit base what nbit_total holds."""
import numpy as np

NCH, NCALLS, CLEN = 24, 6, 8192
NSAMP = NCALLS * CLEN
SEED = 20261018

EVEN_CUTS = [k * CLEN for k in range(NCALLS + 1)]
RAGGED_CUTS = [0, 3000, 3001, 9000, 20480, 20481 + 7, 33333, NSAMP]          # call lengths that are no multiples of 32

# (sample base, the power of two the run crosses or None)
SAMPLE_BASES = [
    ((1 << 31) - 8648, 1 << 31),
    ((1 << 32) - 4796, 1 << 32),            # the wrap of the low word falls inside the first call
    ((1 << 32) - 16384, 1 << 32),           # ... exactly on a call boundary (even cuts)
    ((1 << 32) - 16383, 1 << 32),           # ... one sample to either side of it
    ((1 << 32) - 16385, 1 << 32),
    ((1 << 32) - 29796, 1 << 32),
    ((1 << 40) + 12345, None),              # nothing is crossed: the upper word is simply not zero
]
BIT_BASES = [((1 << 31) - 2000, 1 << 31), ((1 << 32) - 2000, 1 << 32), (1 << 36, None)]
# the sinks' bases: multiples of 12500, so that a sink handed t0 - B / 12500 s prints the time stamps of a run from 0
SINK_BASES = [12500 * 171798, 12500 * 343597, 12500 * 343595, 12500 * 87960931]
SINK_BIT_BASES = [(1 << 32) - 2000, 1 << 40]

_cache = {}


def traffic():
    """[NCH, NSAMP] float32: dense traffic (a block is under way most of the time), the same array for every caller"""
    if "x" not in _cache:
        from acarsdec_amd import synth as S
        rng = np.random.default_rng(SEED)
        x = np.zeros((NCH, NSAMP), dtype=np.float32)
        for c in range(NCH):
            a, _ = S.channel_audio(rng, NSAMP, gap=(250, 700), text_len=(20, 220))
            x[c] = S.envelope(a, noise=0.01, rng=rng)
        x.setflags(write=False)
        _cache["x"] = x
    return _cache["x"]


def frame_key(f):
    """everything a block carries, exactly: (chn, len, err, crc, txt), the level's bits, the three stamps"""
    return (int(f.chn), int(f.len), int(f.err), bytes(f.crc), bytes(f.txt[: max(0, f.len)]),
            np.float32(f.lvl).tobytes(), int(f.end_bit), int(f.end_sample), int(f.soh_sample))


def oracle_run(cuts, sample_base=0, bit_base=0):
    """The oracle over traffic() in calls cut at `cuts`, counters preset.  Per call: ({chn: [frame_key]} of the blocks that call
    completed, {chn: Acarsstate}, {chn: cur - soh} for the channels inside a block (TXT, CRC1, CRC2) at its end)."""
    key = (tuple(cuts), sample_base, bit_base)
    if key not in _cache:
        from oracle import oracle as O
        x = traffic()
        calls = [({}, {}, {}) for _ in cuts[1:]]
        for c in range(NCH):
            ch = O.Channel(c, max_frames=512)
            if sample_base or bit_base:
                ch.preset(sample_base, bit_base)
            seen = 0
            for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
                ch.demod(x[c, a:b])
                fr = ch.frames
                assert len(fr) == ch.c.frames_n
                if len(fr) > seen:
                    calls[k][0][c] = [frame_key(f) for f in fr[seen:]]
                seen = len(fr)
                calls[k][1][c] = int(ch.c.Acarsstate)
                if ch.c.Acarsstate in (3, 4, 5):
                    calls[k][2][c] = int(ch.c.nsamp_total) - int(ch.c.soh_sample)
        _cache[key] = calls
    return _cache[key]
