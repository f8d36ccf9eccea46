// fir_long.hip -- the channel filter over several windows (fir_grid.h, include/acarsdec_amd.h "channel filters"): at an input
// rate that is a multiple of 12 500 Hz (Q == 1, window k = samples [k M, (k + 1) M)) output k is
//     dm[k] = scale_fmt | sum_{n < J M} v[(k - J + 1) M + n] t[n] |,   J = nseg windows of taps.
// The Q == 1 sibling of fir_rate_kernel (fir_rate.hip): the tile, the slices, the aligned fetch and the realigned rows are
// fir_grid_kernel.h's.  What is this kernel's own is the polyphase split
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
#include "fir_grid_kernel.h"

#define LONG_MAXLD ((LONG_CPR_MAX + 1) / 4)     // 64 rows * 36 load slots / 256 threads

template <int FMT>
__global__ __launch_bounds__(ACG_WG_FIR, 3) void fir_long_kernel(const FirLongArgs a, const uint8_t* __restrict__ in_base,
                                                               const uint8_t* __restrict__ hist_base, const float* __restrict__ taps_base,
                                                               const int* __restrict__ stream_of, float* __restrict__ dm_base)
{
    constexpr int BPS = ACG_FIR_GRID_FMT[FMT].bps;
    constexpr int SPC = 16 / BPS;                       // samples (taps) per chunk
    constexpr int JMAX = ACG_LONG_MAXSEG;
    const int J = a.nseg;                               // 2 .. JMAX, wave-uniform
    const int T = ACG_TILE_WIN - (J - 1);               // outputs per tile
    GridWalk w(a, T, BPS);
    if (w.u1 <= 0) return;
    const int lane = w.lane, wave = w.wave;
    unsigned char* tileL = fir_smem;
    float4* red = (float4*)(fir_smem + ACG_TILE_WIN * a.row_stride);      // [4 waves][J][64]
    const unsigned int flip8 = a.fmt == RATE_CS8 ? 0x80808080u : 0u;       // (the two 1-byte formats share RATE_CU8's instantiation)
    const float off8 = a.fmt == RATE_CS8 ? 128.0f : 127.37f;

    // row r of tile ft: its window counted from the call's first (negative: in the history), and where it begins in its row
    auto row_win = [&](int ft, int r) -> int { return a.win0 + ft * T - (J - 1) + r; };
    auto row_start = [&](int wi) -> long long { return (long long)(wi < 0 ? wi + (J - 1) : wi) * w.win_bytes; };

    uint4 stage[LONG_MAXLD];
    f2 accA[JMAX], accB[JMAX];  // per tap segment: (sum r*wr, sum g*wi), (sum r*wi, sum g*wr)
#pragma unroll
    for (int j = 0; j < JMAX; ++j) { accA[j] = {0.f, 0.f}; accB[j] = {0.f, 0.f}; }
    // round -1 only issues the first unit's loads (one fetch site: the staging registers' code is the bulk of the kernel)
    for (long long u = -1; u < w.u1; ++u) {
        const bool live = u >= 0;
        if (live) grid_stage_store<BPS>(w, stage, tileL, [&](int r) { return (int)row_start(row_win(w.t, r)); });
        w.successor(live);
        __syncthreads();
        if (u + 1 < w.u1) {
            const int st = stream_of[w.nch];
            const uint8_t* __restrict__ src = in_base + (size_t)st * a.pitch;
            const uint8_t* __restrict__ hsrc = hist_base + (size_t)st * a.hist_pitch;
            // a row may lie in the history, all of which may be read; a window before the context's first sample does not exist
            grid_fetch(w, stage, [&](int r) {
                const int wi = row_win(w.nt, r);
                const long long sb = row_start(wi);
                return GridRow{wi < 0 ? hsrc : src, (unsigned long long)(sb & ~15ll), wi < 0 ? (unsigned long long)a.hist_pitch : a.valid_bytes,
                               (int)(sb & 15), wi >= -a.nprev && w.nt * T - (J - 1) + r < a.nwin};
            });
        }
        if (!live) continue;

        int c0, c1;
        w.wave_chunks(c0, c1);
        const float* __restrict__ taps = taps_base + (size_t)w.ch * a.tap_pitch;
        const unsigned char* rowp = tileL + lane * a.row_stride + 16;
        const int my_win = row_win(w.t, lane);
        const int my_skew = (int)row_start(my_win);
        for (int c = c0; c < c1; ++c) {
            const int cg = w.k * a.cpr + c;                             // wave-uniform
            const float* __restrict__ tw = taps + cg * SPC * 2;
            unsigned int qq[4];
            grid_read_chunk<BPS>(rowp, c, my_skew, qq);
            // u8: (float)I - 127.37f, rounded once per sample (rtl.c:338-339).  int8 takes the same instantiation:
            // x xor 0x80 is x + 128 as u8, and (float)(x + 128) - 128.0f is the integer, exactly
            if (BPS == 2) {
#pragma unroll
                for (int j = 0; j < 4; ++j) qq[j] ^= flip8;
            }
            f2 x[SPC];
#pragma unroll
            for (int j = 0; j < SPC; ++j) {
                x[j] = grid_sample<BPS>(qq, j);
                if (BPS == 2) x[j] -= off8;
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
                if (s < J) grid_mac(x, tw + (size_t)s * a.decim * 2, accA[s], accB[s]);
            }
        }
        if (w.nk == 0) {                                // last slice of this tile: the partials meet in LDS, emit |D|
            const bool exists = my_win >= -a.nprev;     // a window before the context's first sample contributes nothing
#pragma unroll
            for (int s = 0; s < JMAX; ++s) {
                if (s < J) red[(wave * J + s) * 64 + lane] = exists ? make_float4(accA[s].x, accA[s].y, accB[s].x, accB[s].y) : make_float4(0.f, 0.f, 0.f, 0.f);
                accA[s] = {0.f, 0.f};
                accB[s] = {0.f, 0.f};
            }
            __syncthreads();
            if (wave == 0 && lane >= J - 1) {
                f2 D = {0.f, 0.f};
#pragma unroll
                for (int s = 0; s < JMAX; ++s) {        // oldest window first: segment s lies in the row J - 1 - s before this one
                    if (s >= J) break;
                    const f2 p = grid_wave_sum(red + s * 64, J * 64, lane - (J - 1 - s));
                    D = s == 0 ? p : D + p;
                }
                const int m = w.t * T + lane - (J - 1);
                if (m < a.nwin) dm_base[(size_t)w.ch * a.dm_pitch + m] = cabs_like_glibc(D.x, D.y) * a.scale;
            }
        } else {
            __syncthreads();                            // the slice in LDS is overwritten next round
        }
        w.advance();
    }
}

template <int FMT>
static int launch_long_fmt(const FirLongArgs* a, long long grid, size_t lds, hipStream_t stream)
{
    FIR_LAUNCH(fir_long_kernel<FMT>, dim3((unsigned int)grid), dim3(ACG_WG_FIR), lds, stream, *a, a->in, a->hist, a->taps, a->stream_of, a->dm);
    return (int)hipGetLastError();
}

// The one launcher: the plan is in the arguments (acg_fir_long_plan), the grid is grid_resident_blocks' at three workgroups per
// CU: the kernel's launch bounds, and what the plan's LDS budget (ACG_LONG_LDS_MAX) is cut for.
extern "C" int acg_launch_fir_long(const FirLongArgs* a, void* stream)
{
    if (a->nseg < 2 || a->nseg > ACG_LONG_MAXSEG || a->nwin < 1 || a->nprev < 0 || a->nprev > a->nseg - 1 || a->win0 < 0)
        return (int)hipErrorInvalidValue;
    const size_t lds = acg_fir_long_lds(a);
    long long grid = 0;
    if (lds > ACG_LONG_LDS_MAX || a->cpr > LONG_CPR_MAX || a->cpr < 1 || a->kseg * a->cpr < a->cpr_total) return (int)hipErrorInvalidValue;
    if (int e = grid_resident_blocks(a, lds, 3, ACG_TILE_WIN - (a->nseg - 1), &grid)) return e;
    switch (a->fmt) {
    case RATE_CU8: return launch_long_fmt<RATE_CU8>(a, grid, lds, (hipStream_t)stream);
    case RATE_CS8: return launch_long_fmt<RATE_CU8>(a, grid, lds, (hipStream_t)stream);
    case RATE_CS16: return launch_long_fmt<RATE_CS16>(a, grid, lds, (hipStream_t)stream);
    case RATE_CF32: return launch_long_fmt<RATE_CF32>(a, grid, lds, (hipStream_t)stream);
    }
    return (int)hipErrorInvalidValue;
}
