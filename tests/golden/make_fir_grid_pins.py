"""Pins of the two grid down-converters (csrc/fir_rate.hip, csrc/fir_long.hip): the float32 bits of dm for seeded inputs, recorded
on the GPU through the public Python API of the tree given as argument (default: this one).

    python tests/golden/make_fir_grid_pins.py [tree to import acarsdec_amd from]

The tests of both kernels compare against float64 with a derived bar (tests/rate_ref.py, tests/long_ref.py) and would not notice
another order of additions; tests/test_gpu_grid_pins.py holds every later tree to these bits.  Recorded at f3a4d22, the commit
before the two kernels were given one skeleton (csrc/fir_grid_kernel.h), so that the move is shown to change nothing.

Cases: one channel per stream, two calls of 203 and 131 windows (tiles that are not whole, a second call that does not begin
at grid position 0, a halo and a history across the call), the first presented with all but one sample of a further window;
inputs of rate_ref.make_input.  Three streams; complex float32 takes six, since make_input scales streams 3 and 4 of that format.
  rate path    cu8 at 2 048 000; cs8 at 1 999 999 (Q = 12 500); cs16 at 2 560 000; cf32 at 3 999 999 (decim 320, several slices);
               cu8 at 31 250 (decim 3, a window inside one chunk); rate_ref.make_taps' tables
  filter path  the five (fmt, M, J) of test_gpu_long_fir.SHAPES with long_ref.tap_tables("kaiser")
Output: fir_grid_pins.npz with, per case, "<name>/dm" float32 [streams, 334] and "<name>/crc" uint32 [2]: zlib.crc32 of the input
bytes of both calls and of the tap bytes."""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rate_ref as RR  # noqa: E402
import long_ref as LR  # noqa: E402

PATH = os.path.join(HERE, "fir_grid_pins.npz")
CALLS = (203, 131)
RATE_CASES = [(RR.CU8, 2048000), (RR.CS8, 1999999), (RR.CS16, 2560000), (RR.CF32, 3999999), (RR.CU8, 31250)]
LONG_CASES = [(RR.CU8, 160, 4), (RR.CS8, 160, 2), (RR.CS16, 200, 3), (RR.CF32, 320, 4), (RR.CF32, 8, 4)]     # test_gpu_long_fir.SHAPES
CASES = [("rate-%s-%d" % c, c) for c in RATE_CASES] + [("long-%s-M%d-J%d" % c, c) for c in LONG_CASES]


def streams(fmt):
    return 6 if fmt == RR.CF32 else 3


def inputs(name, case, D):
    """(rate, box taps, filter taps or None, the two calls' rows), from seeds of the case alone"""
    fmt = case[0]
    ns = streams(fmt)
    seed = zlib.crc32(name.encode())
    rng = np.random.default_rng(seed)
    if name.startswith("rate"):
        rate, filt = case[1], None
    else:
        rate = 12500 * case[1]
        filt = LR.tap_tables("kaiser", rate, case[2], ns, np.random.default_rng(seed + 1), D)
    box = RR.make_taps(D, rate, ns, np.random.default_rng(seed + 2))
    rows, k0 = [], 0
    for call, nwin in enumerate(CALLS):
        extra = RR.span(rate, k0 + nwin, 1) - 1 if call == 0 else 0
        rows.append(RR.make_input(fmt, rate, ns, k0, nwin, rng, k=call, extra=extra))
        k0 += nwin
    return rate, box, filt, rows


def crcs(box, filt, rows):
    taps = box.tobytes() + (filt.tobytes() if filt is not None else b"")
    return np.array([zlib.crc32(b"".join(np.ascontiguousarray(x).tobytes() for x in rows)), zlib.crc32(taps)], dtype=np.uint32)


def to_device(x, pad=48):
    """rows on the device, the row rounded up to 16 bytes plus `pad` apart, the gaps filled with a byte that is no sample"""
    import torch
    x = np.ascontiguousarray(x)
    ns, rowb = x.shape[0], x.shape[1] * x.itemsize
    pitch = ((rowb + 15) & ~15) + pad
    buf = np.full(ns * pitch, 0x5A, dtype=np.uint8)
    for s in range(ns):
        buf[s * pitch: s * pitch + rowb] = x[s].view(np.uint8)
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 16 == 0
    return t, pitch, x.shape[1] // 2


def run(D, fmt, rate, box, filt, rows):
    """dm of both calls, float32 [streams, 334]"""
    ns = streams(fmt)
    dec = D.Decoder(ns, decim=RR.decim(rate), nstreams=ns, max_blocks=1, bitlog=False)
    dec.set_taps(box)
    dec.set_input_rate(rate)
    if filt is not None:
        dec.set_channel_filter(filt)
    out, k0 = [], 0
    for nwin, x in zip(CALLS, rows):
        t, pitch, n = to_device(x)
        assert dec.process_rate(RR.capi_fmt(fmt), t, n, pitch) == (nwin, RR.span(rate, k0, nwin)), (fmt, rate, k0)
        out.append(np.stack([dec.dm(c, nwin) for c in range(ns)]))
        k0 += nwin
    dec.close()
    return np.concatenate(out, axis=1).astype(np.float32)


if __name__ == "__main__":
    tree = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else ROOT
    sys.path.insert(0, tree)
    from acarsdec_amd import decoder as D, _capi as K
    assert os.path.dirname(os.path.dirname(os.path.abspath(D.__file__))) == tree, D.__file__
    assert K.load().acg_device_count() > 0, "the recorder needs a GPU"
    out = {}
    for name, case in CASES:
        rate, box, filt, rows = inputs(name, case, D)
        out[name + "/dm"] = run(D, case[0], rate, box, filt, rows)
        out[name + "/crc"] = crcs(box, filt, rows)
    path = sys.argv[2] if len(sys.argv) > 2 else PATH
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes, %d cases from %s" % (path, os.path.getsize(path), len(CASES), tree))
