// fir_rate.hip -- the down-converter at any input rate: windows on the rational grid s_k = floor(k P / Q) (fir_grid.h,
// include/acarsdec_amd.h "any input sample rate").  The tile, the slices, the aligned fetch and the realigned rows are
// fir_grid_kernel.h's.  What is this kernel's own:
//   * row placement.  The windows of a tile are one contiguous span of the launch's own stream.  Window starts relative to the
//     call come from a device table of floor(r P / Q), r <= Q: one 32-bit division per row and tile, by the first 65 threads, a
//     tile ahead, into one of two row tables in LDS (the tile in LDS reads one, the fetch of the next tile the other).
//   * window length per lane.  Every lane runs decim tap steps; a lane whose window is the short one (decim - 1 samples) takes
//     no contribution from index decim - 1, which holds the next window's first sample (the sample is replaced by zero, not
//     multiplied by it).  Only the window's last chunk can hold that index: the steps before it are the sibling's, unmasked.
//     Each lane scales |D| by its own scale_fmt / L.
//   * the u8 constant.  sum (x - 127.37) t = sum x t - 127.37 (1 + j) sum_{i < L} t[i], as fir.hip folds it; the two tap sums
//     of a channel (L = decim - 1, decim) are made on the host when taps or rate change.  int8: x xor 0x80 is x + 128 as u8, the
//     constant is 128.
// A unit of its own, stored as a compressed bundle (the flags in _build.py): four instantiations.
#include "fir_grid_kernel.h"

#define RATE_MAXLD ((RATE_CPR_MAX + 1) / 4)     // 64 rows * 52 load slots / 256 threads

template <int FMT>
__global__ __launch_bounds__(ACG_WG_FIR) void fir_rate_kernel(const FirRateArgs a, const uint8_t* __restrict__ in_base,
                                                               const float* __restrict__ taps_base, const float* __restrict__ tapsum,
                                                               const unsigned int* __restrict__ grid, const int* __restrict__ stream_of,
                                                               float* __restrict__ dm_base)
{
    constexpr int BPS = ACG_FIR_GRID_FMT[FMT].bps;
    constexpr int SPC = 16 / BPS;                       // samples (taps) per chunk
    constexpr bool FOLD = FMT == RATE_CU8 || FMT == RATE_CS8;
    GridWalk w(a, ACG_TILE_WIN, BPS);
    if (w.u1 <= 0) return;
    const int tid = w.tid, lane = w.lane, wave = w.wave;
    unsigned char* tileL = fir_smem;
    float4* red = (float4*)(fir_smem + ACG_TILE_WIN * a.row_stride);
    int* rowtab = (int*)(red + 4 * 64);                 // [2][72]: byte offset of rows 0 .. 64 from the tile's aligned base
    // the window's chunks: those before the one that holds index decim - 1 need no mask
    const int n_main = (a.decim - 1) / SPC;             // == cpr_total - 1

    // first sample of launch window i, relative to the call's row start
    const unsigned int base_r0 = grid[a.r0];
    auto start = [&](unsigned int i) -> unsigned long long {
        const unsigned int idx = a.r0 + (unsigned int)a.win0 + i;
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

    uint4 stage[RATE_MAXLD];
    f2 accA = {0.f, 0.f};       // (sum r*wr, sum g*wi)
    f2 accB = {0.f, 0.f};       // (sum r*wi, sum g*wr)
    unsigned long long A16 = tile_base(w.t), nA16 = A16;
    fill_rowtab(w.t, 0, A16);
    int par = 0, npar = 0;
    // round -1 only issues the first unit's loads (one fetch site: the staging registers' code is the bulk of the kernel)
    for (long long u = -1; u < w.u1; ++u) {
        const bool live = u >= 0, more = u + 1 < w.u1;
        const int* rt = rowtab + par * 72;
        if (live) grid_stage_store<BPS>(w, stage, tileL, [&](int r) { return rt[r]; });
        if (w.successor(live) && more) {
            npar = par ^ 1;
            nA16 = tile_base(w.nt);
            fill_rowtab(w.nt, npar, nA16);
        }
        __syncthreads();
        if (more) {
            const uint8_t* __restrict__ src = in_base + (size_t)stream_of[w.nch] * a.pitch;
            const int* nrt = rowtab + npar * 72;
            // every row is inside the launch's own stream, and inside what the caller presented of it
            grid_fetch(w, stage, [&](int r) {
                const int rb = nrt[r];
                return GridRow{src, nA16 + (unsigned long long)(rb & ~15), a.valid_bytes, rb & 15, w.nt * ACG_TILE_WIN + r < a.nwin};
            });
        }
        if (!live) continue;

        // the lane's window: long (decim samples) or short (decim - 1)
        const bool is_long = (rt[lane + 1] - rt[lane]) == w.win_bytes;
        int c0, c1;
        w.wave_chunks(c0, c1);
        const float* __restrict__ taps = taps_base + (size_t)w.ch * a.decim * 2;
        const unsigned char* rowp = tileL + lane * a.row_stride + 16;
        for (int c = c0; c < c1; ++c) {
            const int cg = w.k * a.cpr + c;                             // wave-uniform
            const float* __restrict__ tw = taps + cg * SPC * 2;
            unsigned int qq[4];
            grid_read_chunk<BPS>(rowp, c, rt[lane], qq);
            if (FMT == RATE_CS8) {
#pragma unroll
                for (int j = 0; j < 4; ++j) qq[j] ^= 0x80808080u;
            }
            f2 x[SPC];
#pragma unroll
            for (int j = 0; j < SPC; ++j) x[j] = grid_sample<BPS>(qq, j);  // (1-byte samples: the constant is folded out)
            if (cg < n_main) {
                grid_mac(x, tw, accA, accB);
            } else {
                // the window's last chunk: taps end at decim, and index decim - 1 belongs to the long windows only
                const int left = a.decim - cg * SPC;                       // 1 .. SPC, wave-uniform
#pragma unroll
                for (int j = 0; j < SPC; ++j) {
                    if (j < left) {
                        f2 xs = x[j];
                        if (j == left - 1 && !is_long) xs = {0.f, 0.f};
                        const f2 wv = {tw[2 * j], tw[2 * j + 1]};
                        const f2 ws = {tw[2 * j + 1], tw[2 * j]};
                        accA = __builtin_elementwise_fma(xs, wv, accA);
                        accB = __builtin_elementwise_fma(xs, ws, accB);
                    }
                }
            }
        }
        if (w.nk == 0) {                                // last slice of this tile: reduce the 4 waves, emit |D|
            red[wave * 64 + lane] = make_float4(accA.x, accA.y, accB.x, accB.y);
            accA = {0.f, 0.f};
            accB = {0.f, 0.f};
            __syncthreads();
            if (wave == 0) {
                f2 D = grid_wave_sum(red, 64, lane);
                if (FOLD) {
                    const float4 ts = ((const float4*)tapsum)[w.ch];
                    const float sr = is_long ? ts.z : ts.x, si = is_long ? ts.w : ts.y;
                    const float off = FMT == RATE_CS8 ? 128.0f : 127.37f;
                    D.x -= off * (sr - si);
                    D.y -= off * (sr + si);
                }
                const int m = w.t * ACG_TILE_WIN + lane;
                if (m < a.nwin) dm_base[(size_t)w.ch * a.dm_pitch + m] = cabs_like_glibc(D.x, D.y) * (is_long ? a.scale_long : a.scale_short);
            }
        } else {
            __syncthreads();                            // the slice in LDS is overwritten next round
        }
        w.advance();
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

// The one launcher: the plan is in the arguments (acg_fir_rate_plan), the grid is grid_resident_blocks' at four workgroups per CU.
extern "C" int acg_launch_fir_rate(const FirRateArgs* a, void* stream)
{
    const size_t lds = acg_fir_rate_lds(a);
    long long grid = 0;
    if (lds > 64 * 1024 || a->cpr > RATE_CPR_MAX || a->nwin < 1) return (int)hipErrorInvalidValue;
    if (int e = grid_resident_blocks(a, lds, 4, ACG_TILE_WIN, &grid)) return e;
    switch (a->fmt) {
    case RATE_CU8: return launch_rate<RATE_CU8>(a, grid, lds, (hipStream_t)stream);
    case RATE_CS8: return launch_rate<RATE_CS8>(a, grid, lds, (hipStream_t)stream);
    case RATE_CS16: return launch_rate<RATE_CS16>(a, grid, lds, (hipStream_t)stream);
    case RATE_CF32: return launch_rate<RATE_CF32>(a, grid, lds, (hipStream_t)stream);
    }
    return (int)hipErrorInvalidValue;
}
