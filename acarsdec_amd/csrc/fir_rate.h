// fir_rate.h -- the down-converter on a rational window grid (fir_rate.hip): what its launcher takes and the plan of a launch.
// Shared by the unit and the host runtime (process.cpp, ctx.cpp); nothing here is a kernel.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "acg_internal.h"

// the formats of the acg_*_rate_* entry points, as the kernel template counts them
#define RATE_CU8 0
#define RATE_CS8 1
#define RATE_CS16 2
#define RATE_CF32 3

// Window w of a launch is window k0 + win0 + w of the context.  With r0 = k0 mod Q and grid[r] = floor(r P / Q), r <= Q, its
// first sample relative to the call's row start is  q P + grid[rem] - grid[r0],  q = (r0 + win0 + w) / Q, rem = the remainder:
// floor((a Q + x) P / Q) = a P + floor(x P / Q), exactly, so the table keeps 64-bit division out of the kernel.
struct FirRateArgs {
    const uint8_t* in;              // [nstreams] rows that begin at the call's first window start
    size_t pitch;                   // bytes between rows (multiple of 16)
    unsigned long long valid_bytes; // bytes of a row that may be read: the samples presented, rounded up to 16
    const int* stream_of;           // [nch]
    const float* taps;              // [nch][decim][2]: the bare oscillator
    const float* tapsum;            // [nch][4]: sum of taps [0, decim - 1) re, im; of taps [0, decim) re, im (the u8 / int8 constant)
    const unsigned int* grid;       // [Q + 1]
    float* dm;                      // window 0 of the launch, channel 0
    size_t dm_pitch;
    unsigned int P, Q, r0, win0;
    int nch, decim, nwin, fmt;
    int ncu;                        // CUs the launch may use (0 = the whole device)
    float scale_long, scale_short;  // scale_fmt / decim, scale_fmt / (decim - 1)
    // the plan (acg_fir_rate_plan)
    int bps;                        // bytes per complex sample
    int cpr_total;                  // 16-byte chunks of a window's decim samples, realigned to its start
    int kseg;                       // column slices a window passes through LDS in
    int cpr;                        // realigned chunks per row and slice (<= 51)
    int row_stride;                 // LDS bytes per row: 16 in front, cpr chunks, 16 behind; an odd number of 16-byte slots
    unsigned int ld_magic;          // ceil(2^20 / (cpr + 1)): the row of a load slot
};

static inline int acg_fir_rate_bps(int fmt) { return fmt == RATE_CF32 ? 8 : fmt == RATE_CS16 ? 4 : 2; }

// One plan for every format and rate: a window's decim samples are cpr_total realigned chunks; a slice holds at most 51 of
// them, because the loads of a slice are one aligned chunk more per row (the row's skew) and 64 rows x 52 chunks is what the 256
// threads stage in 13 registers each (the sibling's limit, fir_kernels.h FMT_MAXLD).
static inline void acg_fir_rate_plan(FirRateArgs* a)
{
    a->bps = acg_fir_rate_bps(a->fmt);
    a->cpr_total = (a->decim * a->bps + 15) / 16;
    a->kseg = (a->cpr_total + 50) / 51;
    a->cpr = (a->cpr_total + a->kseg - 1) / a->kseg;
    const int slots = a->cpr + 2;
    a->row_stride = 16 * ((slots & 1) ? slots : slots + 1);
    a->ld_magic = ((1u << 20) + (unsigned int)a->cpr) / (unsigned int)(a->cpr + 1);
}

static inline size_t acg_fir_rate_lds(const FirRateArgs* a)
{
    return (size_t)ACG_TILE_WIN * a->row_stride + 4 * 64 * 16 /* partial sums */ + 2 * 72 * sizeof(int) /* row tables */;
}

#ifdef __cplusplus
extern "C" {
#endif
// fir_rate.hip.  A weak reference, as the sinks' launchers: the host runtime is also linked without the device units, where the
// rate entry points say ACG_ESTATE.
__attribute__((weak)) int acg_launch_fir_rate(const FirRateArgs* a, void* stream);
#ifdef __cplusplus
}
#endif
