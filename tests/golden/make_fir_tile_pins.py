"""Pins of the three tile down-converters (csrc/fir_tile_kernel.h: fir_u8_persist_kernel, fir_u8_shared_kernel, fir_fmt_kernel): the
float32 bits of dm for seeded inputs, recorded on the GPU through the public Python API of the tree given as argument (default:
this one).

    python tests/golden/make_fir_tile_pins.py [tree to import acarsdec_amd from] [output file]

The tests of these kernels compare against float64 or the oracle with a bar and would not notice another order of additions, and
the order is a contract (the shared-stream kernel gives the bits of the one-channel kernel, the host feed's pieces the bits of one
device call); tests/test_gpu_tile_pins.py holds every later tree to these bits.  Recorded at 5c33a5d, the commit before the three
kernels were given one skeleton.

One callback of 1024 windows, NS streams through a scrambled stream map, every device call made twice (the second round gives the
bits of the first).  The cases and the instantiation each launches (persist<NT, DYN, FULL, S8>, shared<FULL, S8>, fmt<FMT>):
  u8-*         in_callback under ACG_FIR_VARIANT=3, ACG_FIR_SHARED=0: persist<1,1,1,0> at M = 8 (one chunk), 168 (21 chunks, even
               stride padding), 200, 320 (the last staging slot) and (M, ntaps) = (160, 37) (waves with no taps)
  u8-ticket    M = 200, 80 channels on 5 streams, ACG_FIR_WG_PER_CU=1: 320 runs on at most one workgroup per CU (asserted from the
               device's CU count), so runs are taken by ticket
  s8-*         complex int8 by device call at M = 168 and 320: persist<1,1,1,1>; s8-feed: the first 300 windows of the M = 168
               input by Decoder.feed in pieces of 100, 157 and 43 windows: persist<1,1,0,1>
  shared-*     ACG_FIR_MM=0, streams feeding 1, 3, 8 and 11 channels in scrambled order (a full group, a partial one, both
               reduction rounds), M = 200 and 160: shared<1,0> (u8) and shared<1,1> (int8); shared-s8-feed: shared<0,1>
  cs16-*, split-*, f32r-*, cf32-*   the format kernel under ACG_FIR_VARIANT=3: int16 pairs at M = 164 and 400 (two column slices),
               split planes at M = 160, real float32 at M = 200 and 480 (slices), float32 pairs at M = 2, 164, 400 and 1024; one
               ragged feed each (100, 157, 43 windows) for int16 and float32 pairs
The u8 kernels' ragged instantiations persist<1,1,0,0> and shared<0,0> are reached by no public entry point (u8 arrives in whole
callbacks; only the sample formats have a host feed), and persist<0,0,0> / <1,0,0> are the lab build's variants 1 and 2.
Output: fir_tile_pins.npz with, per case, "<name>/dm" float32 [channels, windows] and "<name>/crc" uint32 [2]: zlib.crc32 of the input
bytes and of the tap bytes."""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

PATH = os.path.join(HERE, "fir_tile_pins.npz")
NWIN = 1024
PIECES = (100, 157, 43)             # windows per feed: no multiple of 64, so every launch is ragged
SIZES = [1, 3, 8, 11]               # channels per stream of the shared-stream cases
U8, S8, CS16, SPLIT, F32R, CF32 = "u8", "s8", "cs16", "split", "f32r", "cf32"


def case(name, fmt, M, ntaps=None, ns=4, sizes=None, feed=False, key=None, tunes=()):
    return dict(name=name, fmt=fmt, M=M, ntaps=ntaps or M, ns=ns, sizes=sizes or [1] * ns, feed=feed, key=key or name, tunes=dict(tunes))


PLAIN = (("ACG_FIR_VARIANT", 3), ("ACG_FIR_SHARED", 0))
SHARED = (("ACG_FIR_MM", 0),)
CASES = [case("u8-M%d" % M, U8, M, ns=ns, tunes=PLAIN) for M, ns in ((8, 4), (168, 3), (200, 3), (320, 3))] + [
    case("u8-M160-t37", U8, 160, ntaps=37, ns=3, tunes=PLAIN),
    case("u8-ticket", U8, 200, ns=5, sizes=[16] * 5, tunes=PLAIN + (("ACG_FIR_WG_PER_CU", 1),)),
    case("s8-M168", S8, 168, ns=3, tunes=PLAIN),
    case("s8-M320", S8, 320, ns=3, tunes=PLAIN),
    case("s8-feed-M168", S8, 168, ns=3, feed=True, key="s8-M168", tunes=PLAIN),
    case("shared-u8-M200", U8, 200, sizes=SIZES, tunes=SHARED),
    case("shared-u8-M160", U8, 160, sizes=SIZES, tunes=SHARED),
    case("shared-s8-M200", S8, 200, sizes=SIZES, tunes=SHARED),
    case("shared-s8-M160", S8, 160, sizes=SIZES, tunes=SHARED),
    case("shared-s8-feed-M200", S8, 200, sizes=SIZES, feed=True, key="shared-s8-M200", tunes=SHARED),
    case("cs16-M164", CS16, 164, ns=3, tunes=PLAIN),
    case("cs16-M400", CS16, 400, ns=3, tunes=PLAIN),
    case("cs16-feed-M164", CS16, 164, ns=3, feed=True, key="cs16-M164", tunes=PLAIN),
    case("split-M160", SPLIT, 160, ns=4, tunes=PLAIN),
    case("f32r-M200", F32R, 200, ns=3, tunes=PLAIN),
    case("f32r-M480", F32R, 480, ns=3, tunes=PLAIN),
    case("cf32-M2", CF32, 2, ns=3, tunes=PLAIN),
    case("cf32-M164", CF32, 164, ns=3, tunes=PLAIN),
    case("cf32-M400", CF32, 400, ns=3, tunes=PLAIN),
    case("cf32-M1024", CF32, 1024, ns=3, tunes=PLAIN),
    case("cf32-feed-M164", CF32, 164, ns=3, feed=True, key="cf32-M164", tunes=PLAIN),
]
# a feed case and the device call it shares its input with: the pieces give the bits of the one call
FEED_OF = {c["name"]: c["key"] for c in CASES if c["feed"]}


def inputs(c):
    """(planes of samples [ns, values] -- two for split int16, else one --, taps float32 [nch, ntaps, 2], stream map), from the
    case's seed key alone"""
    rng = np.random.default_rng(zlib.crc32(c["key"].encode()))
    ns, M, fmt = c["ns"], c["M"], c["fmt"]
    nch = int(sum(c["sizes"]))
    if fmt == U8:
        x = (rng.integers(0, 256, size=(ns, NWIN * M * 2), dtype=np.uint8),)
    elif fmt == S8:
        x = (rng.integers(-128, 128, size=(ns, NWIN * M * 2), dtype=np.int8),)
    elif fmt == CS16:
        x = (rng.integers(-32768, 32768, size=(ns, NWIN * M * 2), dtype=np.int16),)
    elif fmt == SPLIT:
        x = tuple(rng.integers(-32768, 32768, size=(ns, NWIN * M), dtype=np.int16) for _ in range(2))
    else:
        x = (rng.standard_normal((ns, NWIN * M * (2 if fmt == CF32 else 1)), dtype=np.float32),)
    taps = (rng.standard_normal((nch, c["ntaps"], 2)) / M).astype(np.float32)
    smap = np.repeat(np.arange(ns), c["sizes"])
    while nch > 1 and np.array_equal(smap, np.repeat(np.arange(ns), c["sizes"])):
        rng.shuffle(smap)
    return x, taps, smap.astype(np.int32)


def crcs(x, taps):
    return np.array([zlib.crc32(b"".join(a.tobytes() for a in x)), zlib.crc32(taps.tobytes())], dtype=np.uint32)


def to_device(x, pad=48):
    """the planes on the device, rows `pitch` bytes apart with a filler between them, the second plane `plane` bytes behind the
    first; returns (tensor, pitch, plane)"""
    import torch
    ns, rowb = x[0].shape[0], x[0].shape[1] * x[0].itemsize
    assert rowb % 16 == 0
    pitch = rowb + pad
    plane = ns * pitch + 32 if len(x) == 2 else 0
    buf = np.full(plane * (len(x) - 1) + ns * pitch, 0x5A, dtype=np.uint8)
    for p, a in enumerate(x):
        for s in range(ns):
            buf[p * plane + s * pitch: p * plane + s * pitch + rowb] = a[s].view(np.uint8)
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 16 == 0
    return t, pitch, plane


def run(D, K, tune, c, x, taps, smap, tunes=None):
    """dm of the case, float32 [channels, windows]; tune(name, value) sets a switch of the library (the caller puts them back).
    tunes: other switches than the case's own."""
    fmt, M, ns = c["fmt"], c["M"], c["ns"]
    nch = int(smap.size)
    kfmt = {U8: None, S8: K.FMT_CS8, CS16: K.FMT_CS16, SPLIT: K.FMT_S16_SPLIT, F32R: K.FMT_F32_REAL, CF32: K.FMT_CF32}[fmt]
    tunes = c["tunes"] if tunes is None else tunes
    for name, value in tunes.items():
        tune(name, str(value))
    shared = "ACG_FIR_MM" in tunes
    dec = D.Decoder(nch, decim=M, ntaps=c["ntaps"], nstreams=ns, max_blocks=1, bitlog=False)
    dec.set_taps(taps)
    dec.set_channel_streams(smap)               # (ACG_FIR_SHARED is read here)
    if kfmt is not None:
        fam = dec.samples_launch(kfmt, 1).family
        assert fam == (K.FIR_SHARED_VECTOR if shared else K.FIR_WORKGROUP), (c["name"], fam)
    else:
        s = dec.launch_shape(1)
        assert s.kernel == 0, (c["name"], s.kernel)                                 # the vector pipe
        if "ACG_FIR_WG_PER_CU" in tunes:        # more runs of FIR_RUN = 4 tiles than workgroups: runs are taken by ticket
            assert nch * (NWIN // 64) // 4 > s.device_cus * int(tunes["ACG_FIR_WG_PER_CU"]), (nch, s.device_cus)
    if c["feed"]:
        out, w0 = [], 0
        per = 1 if fmt in (SPLIT, F32R) else 2
        for n in PIECES:
            cut = [a[:, per * M * w0: per * M * (w0 + n)] for a in x]
            dec.feed(kfmt, cut[0], cut[1] if len(cut) == 2 else None)
            out.append(np.stack([dec.dm(ch, n) for ch in range(nch)]))
            w0 += n
        dm = np.concatenate(out, axis=1)
    else:
        t, pitch, plane = to_device(x)
        rounds = []
        for _ in range(2):
            if kfmt is None:
                dec.in_callback(t, nblocks=1, pitch=pitch)
            else:
                dec.process_samples(kfmt, t, 1, pitch, plane)
            rounds.append(np.stack([dec.dm(ch, NWIN) for ch in range(nch)]))
        assert np.array_equal(rounds[0].view(np.uint32), rounds[1].view(np.uint32)), c["name"]
        dm = rounds[0]
    dec.close()
    return dm.astype(np.float32)


if __name__ == "__main__":
    tree = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else ROOT
    sys.path.insert(0, tree)
    from acarsdec_amd import decoder as D, _capi as K
    assert os.path.dirname(os.path.dirname(os.path.abspath(D.__file__))) == tree, D.__file__
    assert K.load().acg_device_count() > 0, "the recorder needs a GPU"
    out = {}
    for c in CASES:
        x, taps, smap = inputs(c)
        try:
            out[c["name"] + "/dm"] = run(D, K, K.tune, c, x, taps, smap)
        finally:
            for name in c["tunes"]:
                K.tune(name, None)
        out[c["name"] + "/crc"] = crcs(x, taps)
    for f, d in FEED_OF.items():
        n = sum(PIECES)
        assert np.array_equal(out[f + "/dm"].view(np.uint32), out[d + "/dm"][:, :n].view(np.uint32)), (f, d)
    path = sys.argv[2] if len(sys.argv) > 2 else PATH
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes, %d cases from %s" % (path, os.path.getsize(path), len(CASES), tree))
