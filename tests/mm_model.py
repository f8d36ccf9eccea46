"""The matrix-pipe down-converter's arithmetic (acarsdec_amd/csrc/fir_mm.hip: mm_chan_kernel, mm_image_kernel, tile_step) as a
bit-exact numpy model: integers where the kernel uses integers, f64 where it uses f64, ONE rounding to f32 where it rounds.  The
kernels (fir_u8_mm_kernel in both stage variants, fir_u8_mm1_kernel) are held to equality with model_dm on every output
(tests/test_gpu_mm_shapes.py); tests/test_mm_model.py holds the model to the f64-exact value and to the oracle.

Every integer sum here is computed with a float64 matrix product: all operands are integers and every partial sum stays below
2^53 (a digit sum below 2^23, a whole sum below 2 * 200 * 128 * 2^30 < 2^47), so the product is exact in any order of summation.
"""
from types import SimpleNamespace

import numpy as np

C127 = np.float32(127.37)                       # rtl.c:338-339 subtracts this float from every byte
DC = 128.0 - float(C127)                        # u8 - 127.37f = (u8 - 128) + DC, exactly


def chan_consts(taps, M):
    """what mm_chan_kernel and the image kernels derive from one tap table: any (False: every output is +0.0), e, up = 2^(30 - e),
    scale = 2^(e - 30), q int64 [M, 2] (the 31-bit fixed-point taps, zero past the table), dc_re, dc_im"""
    taps = np.asarray(taps, dtype=np.float32).reshape(-1, 2)
    n1 = min(taps.shape[0], M)
    w = np.zeros((M, 2), dtype=np.float32)
    w[:n1] = taps[:n1]
    k = SimpleNamespace()
    mx = np.float32(np.abs(w).max()) if n1 else np.float32(0)
    k.any = bool(mx > 0 and mx < np.float32(3.0e38))
    k.q = np.zeros((M, 2), dtype=np.int64)
    k.e, k.up, k.scale, k.dc_re, k.dc_im = 0, 0.0, 0.0, 0.0, 0.0
    if not k.any:
        return k
    k.e = int(np.frexp(mx)[1])                                      # mx = f 2^e, 0.5 <= f < 1
    k.up = float(np.ldexp(1.0, 30 - k.e))
    k.scale = float(np.ldexp(1.0, k.e - 30))
    k.q = np.rint(w.astype(np.float64) * k.up).astype(np.int64)     # half to even, as __double2int_rn
    assert np.abs(k.q).max() <= 2 ** 30
    sr, si = int(k.q[:, 0].sum()), int(k.q[:, 1].sum())
    k.dc_re = (DC * float(sr - si)) * k.scale                       # one f64 rounding (the product by a power of two is exact)
    k.dc_im = (DC * float(sr + si)) * k.scale
    return k


def digits(q):
    """four balanced base-256 digits of q (int64, |q| <= 2^30): q = d0 + 2^8 d1 + 2^16 d2 + 2^24 d3, every d in [-128, 127]"""
    digs, r = [], np.asarray(q, dtype=np.int64).copy()
    for p in range(4):
        d = ((r + 128) % 256) - 128 if p < 3 else r.copy()
        digs.append(d)
        r = (r - d) // 256
    assert np.all(r == 0) and all(d.min() >= -128 and d.max() <= 127 for d in digs)
    assert np.array_equal(digs[0] + 256 * digs[1] + 65536 * digs[2] + (1 << 24) * digs[3], q)
    return digs


def samples(iq_row, M, nout):
    """s = u8 - 128 of nout windows as float64 [nout, 2 M] (byte order: I, Q interleaved)"""
    x = np.asarray(iq_row, dtype=np.uint8)[: nout * M * 2].reshape(nout, 2 * M)
    return x.astype(np.float64) - 128.0


def byte_coefs(v):
    """[M, 2] per-tap values -> [2 M, 2] per-byte coefficients: column "re" (b odd ? -vi : vr), column "im" (b odd ? vr : vi)"""
    v = np.asarray(v, dtype=np.float64)
    out = np.empty((2 * v.shape[0], 2), dtype=np.float64)
    out[0::2, 0], out[1::2, 0] = v[:, 0], -v[:, 1]
    out[0::2, 1], out[1::2, 1] = v[:, 1], v[:, 0]
    return out


def exact_sums(s, qs, check_digits=True):
    """(Sre, Sim) int64 [K, nout] for K channels on one stream: Sre = sum sI q(wr) - sQ q(wi), Sim = sum sI q(wi) + sQ q(wr).
    check_digits: also form the sums the way the kernel does -- four int8 digit planes, int32 digit sums, lo = a1 256 + a0,
    hi = a3 256 + a2, hi 65536 + lo -- and check the bounds the kernel relies on and that the recombination is the same integer."""
    K = len(qs)
    W = np.concatenate([byte_coefs(q) for q in qs], axis=1)                         # [2 M, 2 K]
    S = np.rint(s @ W).astype(np.int64)
    if check_digits:
        digs = [digits(q) for q in qs]
        a = []
        for p in range(4):
            Wp = np.concatenate([byte_coefs(d[p]) for d in digs], axis=1)
            ap = np.rint(s @ Wp).astype(np.int64)
            assert np.abs(ap).max() < 2 ** 23                                       # what v_mfma_i32_32x32x32_i8 accumulates
            a.append(ap)
        lo = a[1] * 256 + a[0]
        hi = a[3] * 256 + a[2]
        assert np.abs(lo).max() < 2 ** 31 and np.abs(hi).max() < 2 ** 31
        D = hi.astype(np.float64) * 65536.0 + lo.astype(np.float64)                 # the kernel's fma: exact (47 bits)
        assert np.array_equal(D.astype(np.int64), hi * 65536 + lo) and np.array_equal(hi * 65536 + lo, S)
    S = S.T.reshape(K, 2, -1)
    return S[:, 0], S[:, 1]


def finish(Sre, Sim, k):
    """the epilogue: re = f32(Sre scale + dc_re) (the product is exact, so the kernel's fma is this one f64 addition), likewise
    im; dm = f32(sqrt(f64(re)^2 + f64(im)^2)) (glibc's cabsf)"""
    if not k.any:
        return np.zeros(Sre.shape, dtype=np.float32)
    re = (Sre.astype(np.float64) * k.scale + k.dc_re).astype(np.float32)
    im = (Sim.astype(np.float64) * k.scale + k.dc_im).astype(np.float32)
    return cabs(re, im)


def cabs(re, im):
    re, im = re.astype(np.float64), im.astype(np.float64)
    return np.sqrt(re * re + im * im).astype(np.float32)


def model_dm_many(iq_row_u8, M, taps_list, nout, check_digits=True):
    """model_dm for several tap tables on one stream: float32 [K, nout]"""
    ks = [chan_consts(t, M) for t in taps_list]
    s = samples(iq_row_u8, M, nout)
    Sre, Sim = exact_sums(s, [k.q for k in ks], check_digits)
    return np.stack([finish(Sre[i], Sim[i], k) for i, k in enumerate(ks)])


def model_dm(iq_row_u8, M, taps_f32, nout, check_digits=True):
    """what the matrix-pipe kernels write for nout windows of one stream and one tap table [ntaps, 2]: float32 [nout]"""
    return model_dm_many(iq_row_u8, M, [taps_f32], nout, check_digits)[0]


def exact_dm(iq_row, M, taps, nout):
    """|sum (u8 - 127.37f) w| of rtl.c:335-353 with every product and the whole sum in f64: what an infinitely precise
    evaluation of the reference's expression gives (its f32 operands taken as they are)."""
    x = np.asarray(iq_row)[: nout * M * 2].astype(np.float64).reshape(nout, M, 2) - np.float64(C127)
    taps = np.asarray(taps, dtype=np.float32).reshape(-1, 2)
    w = np.zeros((M, 2), dtype=np.float64)
    n1 = min(taps.shape[0], M)
    w[:n1] = taps[:n1].astype(np.float64)
    re = x[:, :, 0] @ w[:, 0] - x[:, :, 1] @ w[:, 1]
    im = x[:, :, 0] @ w[:, 1] + x[:, :, 1] @ w[:, 0]
    return np.hypot(re, im)
