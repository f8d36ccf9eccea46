// fir_grid.h -- the two grid down-converters, the one at any input rate (fir_rate.hip) and the channel filter over several windows
// (fir_long.hip): what their launchers take and the plan of a launch.  Shared by the units (their common device code:
// fir_grid_kernel.h) and the host runtime (process.cpp, ctx.cpp); nothing here is a kernel.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "acg_internal.h"

// the formats of the acg_*_rate_* entry points, as the kernel templates count them: bytes per complex sample and scale_fmt
#define RATE_CU8 0
#define RATE_CS8 1
#define RATE_CS16 2
#define RATE_CF32 3
static constexpr struct { int bps; float scale; } ACG_FIR_GRID_FMT[4] = {{2, 1.0f / 127.5f}, {2, 1.0f / 128.0f}, {4, 1.0f / 32768.0f}, {8, 1.0f}};

#define RATE_CPR_MAX 51             // chunks of a slice, rate kernel: 64 rows x 52 load slots are 13 staging registers per thread
#define LONG_CPR_MAX 35             // ... filter kernel: 36 load slots per row, nine staging registers
#define ACG_LONG_MAXSEG 4           // == ACG_MAXSEG of the public header
// LDS per workgroup of the filter: a third of a CU's 160 KB, so that three workgroups stay resident (the kernel is built for three
// waves per SIMD; with two its loads and its arithmetic overlap too little: profiles/LEDGER.md)
#define ACG_LONG_LDS_MAX ((160 * 1024) / 3)

// What both kernels take.  A launch is windows [win0, win0 + nwin) of a call, a call is rows of samples that begin at a window start.
struct FirGridArgs {
    const uint8_t* in;              // [nstreams] rows that begin at the call's first window start
    size_t pitch;                   // bytes between rows (multiple of 16)
    unsigned long long valid_bytes; // bytes of a row that may be read: the samples presented, rounded up to 16
    const int* stream_of;           // [nch]
    float* dm;                      // window 0 of the launch, channel 0
    size_t dm_pitch;
    int nch, decim, nwin, fmt;
    int win0;                       // the launch's first window, counted from the call's
    int ncu;                        // CUs the launch may use (0 = the whole device)
    // the plan (acg_fir_grid_plan)
    int bps;                        // bytes per complex sample
    int cpr_total;                  // 16-byte chunks of a window's decim samples, realigned to its start
    int kseg;                       // column slices a window passes through LDS in
    int cpr;                        // realigned chunks per row and slice (<= RATE_CPR_MAX, LONG_CPR_MAX)
    int row_stride;                 // LDS bytes per row: 16 in front, cpr chunks, 16 behind; an odd number of 16-byte slots
    unsigned int ld_magic;          // ceil(2^20 / (cpr + 1)): the row of a load slot
};

// Any rate: window w of a launch is window k0 + win0 + w of the context.  With r0 = k0 mod Q and grid[r] = floor(r P / Q), r <= Q,
// its first sample relative to the call's row start is  q P + grid[rem] - grid[r0],  q = (r0 + win0 + w) / Q, rem = the remainder:
// floor((a Q + x) P / Q) = a P + floor(x P / Q), exactly, so the table keeps 64-bit division out of the kernel.
struct FirRateArgs : FirGridArgs {
    const float* taps;              // [nch][decim][2]: the bare oscillator
    const float* tapsum;            // [nch][4]: sum of taps [0, decim - 1) re, im; of taps [0, decim) re, im (the u8 / int8 constant)
    const unsigned int* grid;       // [Q + 1]
    unsigned int P, Q, r0;
    float scale_long, scale_short;  // scale_fmt / decim, scale_fmt / (decim - 1)
};

// The filter, Q == 1: window w of the call is samples [w M, (w + 1) M) of the call's rows, M = decim.  The rows of a tile begin
// nseg - 1 windows before the launch's first, and a window of the call below 0 is window nseg - 1 + w of the history rows (the
// nseg - 1 windows before the call's first sample, oldest first).
struct FirLongArgs : FirGridArgs {
    const uint8_t* hist;            // [nstreams] rows of (nseg - 1) * decim raw samples: what came before the call
    size_t hist_pitch;              // bytes between them (multiple of 16, >= the samples rounded up to 16): all of it may be read
    const float* taps;              // [nch][nseg * decim + 8][2]: index 0 multiplies the oldest sample, the last 8 are zeros (a
    size_t tap_pitch;               // window's last chunk reads up to 7 taps past its segment); floats per channel
    int nseg;
    int nprev;                      // windows of history that exist (0 .. nseg - 1): the rows before them contribute nothing
    float scale;                    // scale_fmt: the taps carry the gain
};

// LDS of a workgroup: the tile's rows, red_slots arrays [4 waves][64] of float4 partial sums, the rate kernel's two row tables
static inline size_t acg_fir_grid_lds(int row_stride, int red_slots, bool rowtab)
{
    return (size_t)ACG_TILE_WIN * row_stride + (size_t)4 * red_slots * 64 * 16 + (rowtab ? 2 * 72 * sizeof(int) : 0);
}

// One plan for every format, rate and kernel: a window's decim samples are cpr_total realigned chunks; a slice holds at most
// cpr_max of them, because the loads of a slice are one aligned chunk more per row (the row's skew) and 64 rows x (cpr_max + 1)
// chunks is what the 256 threads stage in their registers.  With lds_max (the filter, whose partial sums take nseg times the
// room) a window goes through in as many slices as keep a workgroup's LDS at or below it (decim 320, complex float32, nseg 4: 5
// slices of 32 chunks, 51 KB).
static inline void acg_fir_grid_plan(FirGridArgs* a, int cpr_max, int red_slots, size_t lds_max)
{
    a->bps = ACG_FIR_GRID_FMT[a->fmt].bps;
    a->cpr_total = (a->decim * a->bps + 15) / 16;
    for (a->kseg = (a->cpr_total + cpr_max - 1) / cpr_max;; ++a->kseg) {
        a->cpr = (a->cpr_total + a->kseg - 1) / a->kseg;
        const int slots = a->cpr + 2;
        a->row_stride = 16 * ((slots & 1) ? slots : slots + 1);
        if (!lds_max || acg_fir_grid_lds(a->row_stride, red_slots, false) <= lds_max || a->cpr == 1) break;
    }
    a->ld_magic = ((1u << 20) + (unsigned int)a->cpr) / (unsigned int)(a->cpr + 1);
}
static inline void acg_fir_rate_plan(FirRateArgs* a) { acg_fir_grid_plan(a, RATE_CPR_MAX, 1, 0); }
static inline void acg_fir_long_plan(FirLongArgs* a) { acg_fir_grid_plan(a, LONG_CPR_MAX, a->nseg, ACG_LONG_LDS_MAX); }
static inline size_t acg_fir_rate_lds(const FirRateArgs* a) { return acg_fir_grid_lds(a->row_stride, 1, true); }
static inline size_t acg_fir_long_lds(const FirLongArgs* a) { return acg_fir_grid_lds(a->row_stride, a->nseg, false); }

// fir_rate.hip, fir_long.hip.  Weak references, as the sinks' launchers: the host runtime is also linked without the device units,
// where the rate entry points and acg_set_channel_filter say ACG_ESTATE.
extern "C" {
__attribute__((weak)) int acg_launch_fir_rate(const FirRateArgs* a, void* stream);
__attribute__((weak)) int acg_launch_fir_long(const FirLongArgs* a, void* stream);
}
