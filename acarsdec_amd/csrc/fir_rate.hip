// fir_rate.hip -- the down-converter at any input rate: windows on the rational grid s_k = floor(k P / Q) (fir_rate.h,
// include/acarsdec_amd.h "any input sample rate").  The sibling of fir_fmt_kernel (fir_kernels.h): a tile of ACG_TILE_WIN windows
// goes through LDS one padded row per window, lane = window, the four waves split the taps, partial sums meet in LDS, windows
// longer than a slice go through in column slices.  What the grid changes:
//   * row placement.  The windows of a tile are one contiguous span of the stream, but a window starts at any sample.  The span
//     is fetched in ALIGNED 16-byte non-temporal chunks -- per row from its start rounded down to 16 bytes, so a chunk that two
//     windows share is fetched for both (it hits L2 the second time) -- and RE-ALIGNED ON THE WAY INTO LDS: the chunk is stored
//     at its place minus the row's skew, in 8- or 4-byte pieces (the skew is a multiple of the sample size: 2, 4 or 8 bytes;
//     2-byte samples are stored minus the skew's whole words, and a lane whose row lies one half word late shifts its 16 bytes
//     into place with v_alignbit: stored in 2-byte pieces, the compiler makes one ds_write_b128 at 2-byte alignment of them,
//     which the hardware performs piece by piece -- profiles/LEDGER.md).
//     A row has 16 bytes in front and behind its data, so the first and the last chunk need no predicate.  Every row then
//     begins at its own window's start: the reads are the sibling's aligned ds_read_b128 at an odd row stride, and the taps are
//     wave-uniform scalar loads.
//   * window length per lane.  Every lane runs decim tap steps; a lane whose window is the short one (decim - 1 samples) takes
//     no contribution from index decim - 1, which holds the next window's first sample (the sample is replaced by zero, not
//     multiplied by it).  Only the window's last chunk can hold that index: the steps before it are the sibling's, unmasked.
//     Each lane scales |D| by its own scale_fmt / L.
//   * the u8 constant.  sum (x - 127.37) t = sum x t - 127.37 (1 + j) sum_{i < L} t[i], as fir.hip folds it; the two tap sums
//     of a channel (L = decim - 1, decim) are made on the host when taps or rate change.  int8: x xor 0x80 is x + 128 as u8, the
//     constant is 128.
//   * the grid.  Window starts relative to the call come from a device table of floor(r P / Q), r <= Q: one 32-bit division
//     per row and tile, by the first 65 threads, a tile ahead.
// A unit of its own, stored as a compressed bundle (the flags in _build.py): four instantiations.
#include <hip/hip_runtime.h>
#include "acg_internal.h"
#include "fir_rate.h"
#include "fir_kernels.h"

#define RATE_MAXLD 13   // 64 rows * 52 load slots / 256 threads

template <int BPS>
__device__ __forceinline__ void store_pieces(unsigned char* dst, const uint4& v)
{
    if (BPS == 8) {
        ((uint2*)dst)[0] = make_uint2(v.x, v.y);
        ((uint2*)dst)[1] = make_uint2(v.z, v.w);
    } else if (BPS == 4) {
        unsigned int* d = (unsigned int*)dst;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    } else {
        unsigned short* d = (unsigned short*)dst;
        const unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            d[2 * j] = (unsigned short)(w[j] & 0xffffu);
            d[2 * j + 1] = (unsigned short)(w[j] >> 16);
        }
    }
}

template <int FMT>
__global__ __launch_bounds__(ACG_WG_FIR) void fir_rate_kernel(const FirRateArgs a, const uint8_t* __restrict__ in_base,
                                                               const float* __restrict__ taps_base, const float* __restrict__ tapsum,
                                                               const unsigned int* __restrict__ grid, const int* __restrict__ stream_of,
                                                               float* __restrict__ dm_base)
{
    constexpr int BPS = (FMT == RATE_CF32) ? 8 : (FMT == RATE_CS16) ? 4 : 2;
    constexpr int SPC = 16 / BPS;                       // samples (taps) per chunk
    constexpr bool FOLD = FMT == RATE_CU8 || FMT == RATE_CS8;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ntile = (a.nwin + ACG_TILE_WIN - 1) / ACG_TILE_WIN;
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
    float4* red = (float4*)(fir_smem + ACG_TILE_WIN * a.row_stride);
    int* rowtab = (int*)(red + 4 * 64);                 // [2][72]: byte offset of rows 0 .. 64 from the tile's aligned base
    // the window's chunks: those before the one that holds index decim - 1 need no mask
    const int nstep_total = a.cpr_total;
    const int n_main = (a.decim - 1) / SPC;             // == nstep_total - 1

    // first sample of launch window w, relative to the call's row start
    const unsigned int base_r0 = grid[a.r0];
    auto start = [&](unsigned int w) -> unsigned long long {
        const unsigned int idx = a.r0 + a.win0 + w;
        const unsigned int q = idx / a.Q;
        const unsigned int rem = idx - q * a.Q;
        return (unsigned long long)q * a.P + grid[rem] - base_r0;
    };
    // rows 0 .. 64 of tile ft: where they begin, in bytes from the tile's aligned base; returns that base
    auto tile_base = [&](int ft) -> unsigned long long {
        return (start((unsigned int)ft * ACG_TILE_WIN) * BPS) & ~15ull;
    };
    auto fill_rowtab = [&](int ft, int par, unsigned long long A16) {
        if (tid <= ACG_TILE_WIN) rowtab[par * 72 + tid] = (int)(start((unsigned int)ft * ACG_TILE_WIN + tid) * BPS - A16);
    };

    int ch = (int)(g0 / ntile);
    int t = (int)(g0 - (long long)ch * ntile);
    int k = 0;
    uint4 stage[RATE_MAXLD];

    auto fetch = [&](int fch, int ft, int fk, int par, unsigned long long A16) {
        const uint8_t* __restrict__ src = in_base + (size_t)stream_of[fch] * a.pitch;
        typedef unsigned int u4v __attribute__((ext_vector_type(4)));
        const int* rt = rowtab + par * 72;
#pragma unroll
        for (int i = 0; i < RATE_MAXLD; ++i) {
            if (i < nld) {
                const int c = tid + i * ACG_WG_FIR;
                uint4 v = make_uint4(0, 0, 0, 0);
                if (c < slots) {
                    const int r = (int)(((unsigned int)c * magic) >> 20);
                    const int col = c - r * cprl;
                    const int rb = rt[r];
                    const int colg = fk * cpr + col;                    // aligned chunk of the row
                    const unsigned long long off = A16 + (unsigned long long)(rb & ~15) + ((unsigned long long)colg << 4);
                    // the chunks that hold the window's decim samples; inside the launch; inside what the caller presented
                    if (ft * ACG_TILE_WIN + r < a.nwin && (colg << 4) < (rb & 15) + win_bytes && off + 16 <= a.valid_bytes) {
                        const u4v x = __builtin_nontemporal_load((const u4v*)(src + off));
                        v = make_uint4(x.x, x.y, x.z, x.w);
                    }
                }
                stage[i] = v;
            }
        }
    };

    f2 accA = {0.f, 0.f};       // (sum r*wr, sum g*wi)
    f2 accB = {0.f, 0.f};       // (sum r*wi, sum g*wr)
    const long long u1 = (g1 - g0) * K;
    unsigned long long A16 = tile_base(t);
    fill_rowtab(t, 0, A16);
    int par = 0;
    // round -1 only issues the first unit's loads (one fetch site: the staging registers' code is the bulk of the kernel)
    for (long long u = -1; u < u1; ++u) {
        const bool live = u >= 0;
        if (live) {
            const int* rt = rowtab + par * 72;
#pragma unroll
            for (int i = 0; i < RATE_MAXLD; ++i) {
                if (i < nld) {
                    const int c = tid + i * ACG_WG_FIR;
                    if (c < slots) {
                        const int r = (int)(((unsigned int)c * magic) >> 20);
                        const int col = c - r * cprl;
                        // realigned: the chunk's place in the row minus the row's skew, behind the 16 bytes in front
                        // (2-byte samples: minus the skew's whole words only -- an odd half word is the reader's, see below)
                        store_pieces<(BPS == 2 ? 4 : BPS)>(tileL + r * a.row_stride + 16 + (col << 4) - (rt[r] & (BPS == 2 ? 12 : 15)), stage[i]);
                    }
                }
            }
        }
        int nch_ = ch, nt_ = t, nk_ = live ? k + 1 : 0, npar = par;
        unsigned long long nA16 = A16;
        if (live && nk_ == K) {
            nk_ = 0;
            if (++nt_ == ntile) { nt_ = 0; ++nch_; }
            if (u + 1 < u1) {
                npar = par ^ 1;
                nA16 = tile_base(nt_);
                fill_rowtab(nt_, npar, nA16);
            }
        }
        __syncthreads();
        if (u + 1 < u1) fetch(nch_, nt_, nk_, npar, nA16);
        if (!live) continue;

        // the lane's window: long (decim samples) or short (decim - 1)
        const bool is_long = (rowtab[par * 72 + lane + 1] - rowtab[par * 72 + lane]) == win_bytes;
        // this slice's chunks, split over the 4 waves
        const int nstep = max(0, min(cpr, nstep_total - k * cpr));
        const int c0 = nstep * wave / 4;
        const int c1 = nstep * (wave + 1) / 4;
        const float* __restrict__ taps = taps_base + (size_t)ch * a.decim * 2;
        const unsigned char* rowp = tileL + lane * a.row_stride + 16;
        // 2-byte samples: a row whose skew is an odd number of half words lies one half word late (its words were stored whole);
        // the lane shifts its 16 bytes into place with the next word, v_alignbit by 0 or 16
        const unsigned int half = BPS == 2 ? (unsigned int)(rowtab[par * 72 + lane] & 2) * 8u : 0u;
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
            if (FMT == RATE_CS8) {
#pragma unroll
                for (int j = 0; j < 4; ++j) qq[j] ^= 0x80808080u;
            }
            f2 x[SPC];
#pragma unroll
            for (int j = 0; j < SPC; ++j) {
                if (FOLD) {
                    const unsigned int word = qq[j >> 1];
                    const unsigned int sh = (j & 1) * 16;
                    x[j].x = (float)((word >> sh) & 0xffu);                 // rtl.c:338-339, the constant folded out
                    x[j].y = (float)((word >> (sh + 8)) & 0xffu);
                } else if (FMT == RATE_CS16) {
                    x[j].x = (float)(short)(qq[j] & 0xffffu);              // soapy.c:238
                    x[j].y = (float)((int)qq[j] >> 16);                    // soapy.c:239
                } else {
                    x[j].x = __uint_as_float(qq[2 * j]);
                    x[j].y = __uint_as_float(qq[2 * j + 1]);
                }
            }
            if (cg < n_main) {
#pragma unroll
                for (int j = 0; j < SPC; ++j) {
                    const f2 wv = {w[2 * j], w[2 * j + 1]};
                    const f2 ws = {w[2 * j + 1], w[2 * j]};
                    accA = __builtin_elementwise_fma(x[j], wv, accA);
                    accB = __builtin_elementwise_fma(x[j], ws, accB);
                }
            } else {
                // the window's last chunk: taps end at decim, and index decim - 1 belongs to the long windows only
                const int left = a.decim - cg * SPC;                       // 1 .. SPC, wave-uniform
#pragma unroll
                for (int j = 0; j < SPC; ++j) {
                    if (j < left) {
                        f2 xs = x[j];
                        if (j == left - 1 && !is_long) xs = {0.f, 0.f};
                        const f2 wv = {w[2 * j], w[2 * j + 1]};
                        const f2 ws = {w[2 * j + 1], w[2 * j]};
                        accA = __builtin_elementwise_fma(xs, wv, accA);
                        accB = __builtin_elementwise_fma(xs, ws, accB);
                    }
                }
            }
        }
        if (nk_ == 0) {                                 // last slice of this tile: reduce the 4 waves, emit |D|
            red[wave * 64 + lane] = make_float4(accA.x, accA.y, accB.x, accB.y);
            accA = {0.f, 0.f};
            accB = {0.f, 0.f};
            __syncthreads();
            if (wave == 0) {
                const float4 r0 = red[lane], r1 = red[64 + lane], r2 = red[128 + lane], r3 = red[192 + lane];
                float Dr = ((r0.x + r1.x) + (r2.x + r3.x)) - ((r0.y + r1.y) + (r2.y + r3.y));
                float Di = ((r0.z + r1.z) + (r2.z + r3.z)) + ((r0.w + r1.w) + (r2.w + r3.w));
                if (FOLD) {
                    const float4 ts = ((const float4*)tapsum)[ch];
                    const float sr = is_long ? ts.z : ts.x, si = is_long ? ts.w : ts.y;
                    const float off = FMT == RATE_CS8 ? 128.0f : 127.37f;
                    Dr -= off * (sr - si);
                    Di -= off * (sr + si);
                }
                const int m = t * ACG_TILE_WIN + lane;
                if (m < a.nwin) dm_base[(size_t)ch * a.dm_pitch + m] = cabs_like_glibc(Dr, Di) * (is_long ? a.scale_long : a.scale_short);
            }
        } else {
            __syncthreads();                            // the slice in LDS is overwritten next round
        }
        ch = nch_;
        t = nt_;
        k = nk_;
        par = npar;
        A16 = nA16;
    }
}

template <int FMT>
static int launch_rate(const FirRateArgs* a, long long grid, size_t lds, hipStream_t stream)
{
    FIR_LAUNCH(fir_rate_kernel<FMT>, dim3((unsigned int)grid), dim3(ACG_WG_FIR), lds, stream, *a, a->in, a->taps, a->tapsum, a->grid,
               a->stream_of, a->dm);
    return (int)hipGetLastError();
}

// The one launcher: the plan is in the arguments (acg_fir_rate_plan), the grid is the sibling's -- as many workgroups as stay
// resident, a static contiguous partition of the (channel, tile) space.
extern "C" int acg_launch_fir_rate(const FirRateArgs* a, void* stream)
{
    const size_t lds = acg_fir_rate_lds(a);
    int num_cu = 0;
    if (int e = acg_fir_device_cus(&num_cu)) return e;
    if (lds > 64 * 1024 || a->cpr > 51 || a->nwin < 1) return (int)hipErrorInvalidValue;
    int per_cu = (int)((160 * 1024) / lds);
    if (per_cu > 4) per_cu = 4;
    const long long ntile = (a->nwin + ACG_TILE_WIN - 1) / ACG_TILE_WIN;
    const long long G = (long long)a->nch * ntile;
    long long grid = (long long)(a->ncu > 0 ? a->ncu : num_cu) * per_cu;
    if (grid > G) grid = G;
    switch (a->fmt) {
    case RATE_CU8: return launch_rate<RATE_CU8>(a, grid, lds, (hipStream_t)stream);
    case RATE_CS8: return launch_rate<RATE_CS8>(a, grid, lds, (hipStream_t)stream);
    case RATE_CS16: return launch_rate<RATE_CS16>(a, grid, lds, (hipStream_t)stream);
    case RATE_CF32: return launch_rate<RATE_CF32>(a, grid, lds, (hipStream_t)stream);
    }
    return (int)hipErrorInvalidValue;
}
