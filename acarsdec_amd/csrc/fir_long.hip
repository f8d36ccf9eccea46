// fir_long.hip -- the channel filter over several windows (fir_long.h, include/acarsdec_amd.h "channel filters"): at an input
// rate that is a multiple of 12 500 Hz (Q == 1, window k = samples [k M, (k + 1) M)) output k is
//     dm[k] = scale_fmt | sum_{n < J M} v[(k - J + 1) M + n] t[n] |,   J = nseg windows of taps.
// The Q == 1 sibling of fir_rate_kernel (fir_rate.hip) with the same skeleton: a tile of ACG_TILE_WIN windows goes through LDS
// one padded row per window, lane = window, the four waves split the taps, aligned 16-byte non-temporal loads staged through
// registers and re-aligned on the way into LDS, a static contiguous partition of the (channel, tile) space.  What changes is
// the polyphase split
//     dm[k] = | sum_{j < J} P_j[k - (J - 1 - j)] |,   P_j[w] = sum_{i < M} v[w M + i] t[j M + i]:
//   * partial sums.  Every row is still one non-overlapping window, fetched once; each lane keeps J pairs of packed
//     accumulators, one per tap segment, and the cross-wave reduction has J slots per lane.  Output k is the sum of J partials of
//     neighbouring rows, read back from that LDS array.  Global and LDS traffic per sample are fir_rate_kernel's; the arithmetic
//     is J times its.
//   * the halo.  A tile's rows are windows [T t - (J - 1), T t + T) of the launch with T = 64 - (J - 1) outputs: (J - 1) / 64 of
//     the rows are computed twice, no state passes between workgroups.
//   * the order of additions is fixed: within a partial as the wave split gives it (a function of decim and the format only),
//     across waves (w0 + w1) + (w2 + w3) per component, re and im of a partial from those, across segments oldest window first.
//     So the result does not depend on the tile, the launch or the call a window falls into.
//   * history.  A row whose window lies before the call's first sample reads the history rows (the J - 1 windows before the
//     call, kept by the host runtime); a row before the context's first sample contributes nothing: its partials are replaced
//     by zero (not its samples, which u8 could not express).
//   * the u8 constant is NOT folded out: with 60 - 70 dB of cancellation in the stop band the folded form's error would be that
//     of a sum 127 times larger.  x = (float)I - 127.37f per sample, rounded once (rtl.c:338-339).
// A unit of its own, stored as a compressed bundle (the flags in _build.py): three instantiations, one per sample size.  J is a launch
// argument, not a template parameter (twelve instantiations were three times the code in both libraries): the segment loops are
// unrolled to ACG_LONG_MAXSEG and a segment at or above J is skipped by a scalar branch.
#include <hip/hip_runtime.h>
#include "acg_internal.h"
#include "fir_long.h"
#include "fir_kernels.h"

#define LONG_MAXLD 9    // 64 rows * 36 load slots / 256 threads (the plan keeps a slice at 35 chunks)

template <int BPS>
__device__ __forceinline__ void long_store_pieces(unsigned char* dst, const uint4& v)
{
    if (BPS == 8) {
        ((uint2*)dst)[0] = make_uint2(v.x, v.y);
        ((uint2*)dst)[1] = make_uint2(v.z, v.w);
    } else {
        unsigned int* d = (unsigned int*)dst;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
}

template <int FMT>
__global__ __launch_bounds__(ACG_WG_FIR, 3) void fir_long_kernel(const FirLongArgs a, const uint8_t* __restrict__ in_base,
                                                               const uint8_t* __restrict__ hist_base, const float* __restrict__ taps_base,
                                                               const int* __restrict__ stream_of, float* __restrict__ dm_base)
{
    constexpr int BPS = (FMT == RATE_CF32) ? 8 : (FMT == RATE_CS16) ? 4 : 2;
    constexpr int SPC = 16 / BPS;                       // samples (taps) per chunk
    constexpr int JMAX = ACG_LONG_MAXSEG;
    const int J = a.nseg;                               // 2 .. JMAX, wave-uniform
    const int T = ACG_TILE_WIN - (J - 1);               // outputs per tile
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ntile = (a.nwin + T - 1) / T;
    const long long G = (long long)a.nch * ntile;
    const long long g0 = G * blockIdx.x / gridDim.x;
    const long long g1 = G * (blockIdx.x + 1) / gridDim.x;
    if (g0 >= g1) return;

    const int K = a.kseg;
    const int cpr = a.cpr;
    const int cprl = cpr + 1;                           // aligned chunks loaded per row and slice
    const int slots = ACG_TILE_WIN * cprl;
    const int nld = (slots + ACG_WG_FIR - 1) / ACG_WG_FIR;
    const unsigned int magic = a.ld_magic;
    const int win_bytes = a.decim * BPS;
    unsigned char* tileL = fir_smem;
    float4* red = (float4*)(fir_smem + ACG_TILE_WIN * a.row_stride);      // [4 waves][J][64]
    const int nstep_total = a.cpr_total;
    const unsigned int flip8 = a.fmt == RATE_CS8 ? 0x80808080u : 0u;       // (the two 1-byte formats share RATE_CU8's instantiation)
    const float off8 = a.fmt == RATE_CS8 ? 128.0f : 127.37f;

    // row r of tile ft: its window counted from the call's first (negative: in the history), and where it begins in its row
    auto row_win = [&](int ft, int r) -> int { return a.win0 + ft * T - (J - 1) + r; };
    auto row_start = [&](int wi) -> long long { return (long long)(wi < 0 ? wi + (J - 1) : wi) * win_bytes; };

    int ch = (int)(g0 / ntile);
    int t = (int)(g0 - (long long)ch * ntile);
    int k = 0;
    uint4 stage[LONG_MAXLD];

    auto fetch = [&](int fch, int ft, int fk) {
        const int st = stream_of[fch];
        const uint8_t* __restrict__ src = in_base + (size_t)st * a.pitch;
        const uint8_t* __restrict__ hsrc = hist_base + (size_t)st * a.hist_pitch;
        typedef unsigned int u4v __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int i = 0; i < LONG_MAXLD; ++i) {
            if (i < nld) {
                const int c = tid + i * ACG_WG_FIR;
                uint4 v = make_uint4(0, 0, 0, 0);
                if (c < slots) {
                    const int r = (int)(((unsigned int)c * magic) >> 20);
                    const int col = c - r * cprl;
                    const int wi = row_win(ft, r);
                    const long long sb = row_start(wi);
                    const int colg = fk * cpr + col;                    // aligned chunk of the row
                    const long long off = (sb & ~15ll) + ((long long)colg << 4);
                    const unsigned long long lim = wi < 0 ? (unsigned long long)a.hist_pitch : a.valid_bytes;
                    // a window that exists; inside the launch; the chunks that hold its decim samples; inside what may be read
                    if (wi >= -a.nprev && ft * T - (J - 1) + r < a.nwin && (colg << 4) < (int)(sb & 15) + win_bytes &&
                        (unsigned long long)off + 16 <= lim) {
                        const u4v x = __builtin_nontemporal_load((const u4v*)((wi < 0 ? hsrc : src) + off));
                        v = make_uint4(x.x, x.y, x.z, x.w);
                    }
                }
                stage[i] = v;
            }
        }
    };

    f2 accA[JMAX], accB[JMAX];  // per tap segment: (sum r*wr, sum g*wi), (sum r*wi, sum g*wr)
#pragma unroll
    for (int j = 0; j < JMAX; ++j) { accA[j] = {0.f, 0.f}; accB[j] = {0.f, 0.f}; }
    const long long u1 = (g1 - g0) * K;
    // round -1 only issues the first unit's loads (one fetch site: the staging registers' code is the bulk of the kernel)
    for (long long u = -1; u < u1; ++u) {
        const bool live = u >= 0;
        if (live) {
#pragma unroll
            for (int i = 0; i < LONG_MAXLD; ++i) {
                if (i < nld) {
                    const int c = tid + i * ACG_WG_FIR;
                    if (c < slots) {
                        const int r = (int)(((unsigned int)c * magic) >> 20);
                        const int col = c - r * cprl;
                        const int skew = (int)(row_start(row_win(t, r)) & 15);
                        // realigned: the chunk's place in the row minus the row's skew, behind the 16 bytes in front
                        // (2-byte samples: minus the skew's whole words only -- an odd half word is the reader's, see below)
                        long_store_pieces<(BPS == 2 ? 4 : BPS)>(tileL + r * a.row_stride + 16 + (col << 4) - (skew & (BPS == 2 ? 12 : 15)), stage[i]);
                    }
                }
            }
        }
        int nch_ = ch, nt_ = t, nk_ = live ? k + 1 : 0;
        if (live && nk_ == K) {
            nk_ = 0;
            if (++nt_ == ntile) { nt_ = 0; ++nch_; }
        }
        __syncthreads();
        if (u + 1 < u1) fetch(nch_, nt_, nk_);
        if (!live) continue;

        // this slice's chunks, split over the 4 waves
        const int nstep = max(0, min(cpr, nstep_total - k * cpr));
        const int c0 = nstep * wave / 4;
        const int c1 = nstep * (wave + 1) / 4;
        const float* __restrict__ taps = taps_base + (size_t)ch * a.tap_pitch;
        const unsigned char* rowp = tileL + lane * a.row_stride + 16;
        const int my_win = row_win(t, lane);
        // 2-byte samples: a row whose skew is an odd number of half words lies one half word late (its words were stored whole);
        // the lane shifts its 16 bytes into place with the next word, v_alignbit by 0 or 16
        const unsigned int half = BPS == 2 ? (unsigned int)(row_start(my_win) & 2) * 8u : 0u;
        for (int c = c0; c < c1; ++c) {
            const int cg = k * cpr + c;                                 // wave-uniform
            const float* __restrict__ w = taps + cg * SPC * 2;
            const uint4 q = *(const uint4*)(rowp + (c << 4));
            unsigned int qq[4] = {q.x, q.y, q.z, q.w};
            if (BPS == 2) {
                const unsigned int nx = *(const unsigned int*)(rowp + (c << 4) + 16);
                qq[0] = __builtin_amdgcn_alignbit(q.y, q.x, half);
                qq[1] = __builtin_amdgcn_alignbit(q.z, q.y, half);
                qq[2] = __builtin_amdgcn_alignbit(q.w, q.z, half);
                qq[3] = __builtin_amdgcn_alignbit(nx, q.w, half);
            }
            f2 x[SPC];
#pragma unroll
            for (int j = 0; j < SPC; ++j) {
                if (FMT == RATE_CU8) {
                    // u8: (float)I - 127.37f, rounded once per sample (rtl.c:338-339).  int8 takes the same instantiation:
                    // x xor 0x80 is x + 128 as u8, and (float)(x + 128) - 128.0f is the integer, exactly
                    const unsigned int word = qq[j >> 1] ^ flip8;
                    const unsigned int sh = (j & 1) * 16;
                    x[j].x = (float)((word >> sh) & 0xffu) - off8;
                    x[j].y = (float)((word >> (sh + 8)) & 0xffu) - off8;
                } else if (FMT == RATE_CS16) {
                    x[j].x = (float)(short)(qq[j] & 0xffffu);              // soapy.c:238
                    x[j].y = (float)((int)qq[j] >> 16);                    // soapy.c:239
                } else {
                    x[j].x = __uint_as_float(qq[2 * j]);
                    x[j].y = __uint_as_float(qq[2 * j + 1]);
                }
            }
            const int left = a.decim - cg * SPC;                           // samples of the window from this chunk on, wave-uniform
            if (left < SPC) {
                // the window's last chunk: the samples behind the window are the next one's and count as zero (replaced, not
                // multiplied: they may be anything); the taps read with them are the channel's next segment's or the zeros behind
                // its table (ctx.cpp) -- the products are zeros and the sums do not move
#pragma unroll
                for (int j = 0; j < SPC; ++j)
                    if (j >= left) x[j] = {0.f, 0.f};
            }
#pragma unroll
            for (int s = 0; s < JMAX; ++s) {
                if (s < J) {
                    const float* __restrict__ ws_ = w + (size_t)s * a.decim * 2;
#pragma unroll
                    for (int j = 0; j < SPC; ++j) {
                        const f2 wv = {ws_[2 * j], ws_[2 * j + 1]};
                        const f2 ws = {ws_[2 * j + 1], ws_[2 * j]};
                        accA[s] = __builtin_elementwise_fma(x[j], wv, accA[s]);
                        accB[s] = __builtin_elementwise_fma(x[j], ws, accB[s]);
                    }
                }
            }
        }
        if (nk_ == 0) {                                 // last slice of this tile: the partials meet in LDS, emit |D|
            const bool exists = my_win >= -a.nprev;     // a window before the context's first sample contributes nothing
#pragma unroll
            for (int s = 0; s < JMAX; ++s) {
                if (s < J) red[(wave * J + s) * 64 + lane] = exists ? make_float4(accA[s].x, accA[s].y, accB[s].x, accB[s].y) : make_float4(0.f, 0.f, 0.f, 0.f);
                accA[s] = {0.f, 0.f};
                accB[s] = {0.f, 0.f};
            }
            __syncthreads();
            if (wave == 0 && lane >= J - 1) {
                float Dr = 0.f, Di = 0.f;
#pragma unroll
                for (int s = 0; s < JMAX; ++s) {        // oldest window first: segment s lies in the row J - 1 - s before this one
                    if (s >= J) break;
                    const int row = lane - (J - 1 - s);
                    const float4 r0 = red[(0 * J + s) * 64 + row], r1 = red[(1 * J + s) * 64 + row];
                    const float4 r2 = red[(2 * J + s) * 64 + row], r3 = red[(3 * J + s) * 64 + row];
                    const float pr = ((r0.x + r1.x) + (r2.x + r3.x)) - ((r0.y + r1.y) + (r2.y + r3.y));
                    const float pi = ((r0.z + r1.z) + (r2.z + r3.z)) + ((r0.w + r1.w) + (r2.w + r3.w));
                    Dr = s == 0 ? pr : Dr + pr;
                    Di = s == 0 ? pi : Di + pi;
                }
                const int m = t * T + lane - (J - 1);
                if (m < a.nwin) dm_base[(size_t)ch * a.dm_pitch + m] = cabs_like_glibc(Dr, Di) * a.scale;
            }
        } else {
            __syncthreads();                            // the slice in LDS is overwritten next round
        }
        ch = nch_;
        t = nt_;
        k = nk_;
    }
}

template <int FMT>
static int launch_long_fmt(const FirLongArgs* a, long long grid, size_t lds, hipStream_t stream)
{
    FIR_LAUNCH(fir_long_kernel<FMT>, dim3((unsigned int)grid), dim3(ACG_WG_FIR), lds, stream, *a, a->in, a->hist, a->taps, a->stream_of, a->dm);
    return (int)hipGetLastError();
}

// The one launcher: the plan is in the arguments (acg_fir_long_plan), the grid is the sibling's -- as many workgroups as stay
// resident, a static contiguous partition of the (channel, tile) space.
extern "C" int acg_launch_fir_long(const FirLongArgs* a, void* stream)
{
    if (a->nseg < 2 || a->nseg > ACG_LONG_MAXSEG || a->nwin < 1 || a->nprev < 0 || a->nprev > a->nseg - 1 || a->win0 < 0)
        return (int)hipErrorInvalidValue;
    const size_t lds = acg_fir_long_lds(a);
    int num_cu = 0;
    if (int e = acg_fir_device_cus(&num_cu)) return e;
    if (lds > ACG_LONG_LDS_MAX || a->cpr > 35 || a->cpr < 1 || a->kseg * a->cpr < a->cpr_total) return (int)hipErrorInvalidValue;
    int per_cu = (int)((160 * 1024) / lds);
    if (per_cu > 3) per_cu = 3;                         // three waves per SIMD: what the registers allow (the kernel's launch bounds)
    const int T = ACG_TILE_WIN - (a->nseg - 1);
    const long long ntile = (a->nwin + T - 1) / T;
    const long long G = (long long)a->nch * ntile;
    long long grid = (long long)(a->ncu > 0 ? a->ncu : num_cu) * per_cu;
    if (grid > G) grid = G;
    switch (a->fmt) {
    case RATE_CU8: return launch_long_fmt<RATE_CU8>(a, grid, lds, (hipStream_t)stream);
    case RATE_CS8: return launch_long_fmt<RATE_CU8>(a, grid, lds, (hipStream_t)stream);
    case RATE_CS16: return launch_long_fmt<RATE_CS16>(a, grid, lds, (hipStream_t)stream);
    case RATE_CF32: return launch_long_fmt<RATE_CF32>(a, grid, lds, (hipStream_t)stream);
    }
    return (int)hipErrorInvalidValue;
}
