// fir_long.h -- the channel filter over several windows (fir_long.hip, include/acarsdec_amd.h "channel filters"): what its
// launcher takes and the plan of a launch.  Shared by the unit and the host runtime (process.cpp, ctx.cpp); nothing here is a
// kernel.  The formats are fir_rate.h's (RATE_CU8 ..).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "acg_internal.h"
#include "fir_rate.h"

#define ACG_LONG_MAXSEG 4           // == ACG_MAXSEG of the public header
// LDS per workgroup: a third of a CU's 160 KB, so that three workgroups stay resident (the kernel is built for three waves per
// SIMD; with two its loads and its arithmetic overlap too little: profiles/LEDGER.md)
#define ACG_LONG_LDS_MAX ((160 * 1024) / 3)

// Q == 1: window w of the call is samples [w M, (w + 1) M) of the call's rows, M = decim.  Window w of a launch is window
// win0 + w of the call; the rows of a tile begin nseg - 1 windows earlier, and a window of the call below 0 is window
// nseg - 1 + w of the history rows (the nseg - 1 windows before the call's first sample, oldest first).
struct FirLongArgs {
    const uint8_t* in;              // [nstreams] rows that begin at the call's first window start
    size_t pitch;                   // bytes between rows (multiple of 16)
    unsigned long long valid_bytes; // bytes of a row that may be read: the samples presented, rounded up to 16
    const uint8_t* hist;            // [nstreams] rows of (nseg - 1) * decim raw samples: what came before the call
    size_t hist_pitch;              // bytes between them (multiple of 16, >= the samples rounded up to 16): all of it may be read
    const int* stream_of;           // [nch]
    const float* taps;              // [nch][nseg * decim + 8][2]: index 0 multiplies the oldest sample, the last 8 are zeros (a
    size_t tap_pitch;               // window's last chunk reads up to 7 taps past its segment); floats per channel
    float* dm;                      // window 0 of the launch, channel 0
    size_t dm_pitch;
    int nch, decim, nseg, nwin, fmt;
    int win0;                       // the launch's first window, counted from the call's
    int nprev;                      // windows of history that exist (0 .. nseg - 1): the rows before them contribute nothing
    int ncu;                        // CUs the launch may use (0 = the whole device)
    float scale;                    // scale_fmt: the taps carry the gain
    // the plan (acg_fir_long_plan)
    int bps;                        // bytes per complex sample
    int cpr_total;                  // 16-byte chunks of a window's decim samples, realigned to its start
    int kseg;                       // column slices a window passes through LDS in
    int cpr;                        // realigned chunks per row and slice (<= 35)
    int row_stride;                 // LDS bytes per row: 16 in front, cpr chunks, 16 behind; an odd number of 16-byte slots
    unsigned int ld_magic;          // ceil(2^20 / (cpr + 1)): the row of a load slot
};

static inline size_t acg_fir_long_lds(const FirLongArgs* a)
{
    return (size_t)ACG_TILE_WIN * a->row_stride + (size_t)4 * a->nseg * 64 * 16 /* partial sums: [wave][segment][row] */;
}

// fir_rate.h's plan with one more rule: the partial sums take nseg times the room, so a window goes through in as many slices as
// keep a workgroup's LDS at or below ACG_LONG_LDS_MAX (decim 320, complex float32, nseg 4: 5 slices of 32 chunks, 51 KB).
static inline void acg_fir_long_plan(FirLongArgs* a)
{
    a->bps = acg_fir_rate_bps(a->fmt);
    a->cpr_total = (a->decim * a->bps + 15) / 16;
    for (a->kseg = (a->cpr_total + 34) / 35;; ++a->kseg) {       // 36 load slots per row: nine staging registers per thread
        a->cpr = (a->cpr_total + a->kseg - 1) / a->kseg;
        const int slots = a->cpr + 2;
        a->row_stride = 16 * ((slots & 1) ? slots : slots + 1);
        if (acg_fir_long_lds(a) <= ACG_LONG_LDS_MAX || a->cpr == 1) break;
    }
    a->ld_magic = ((1u << 20) + (unsigned int)a->cpr) / (unsigned int)(a->cpr + 1);
}

#ifdef __cplusplus
extern "C" {
#endif
// fir_long.hip.  A weak reference, as acg_launch_fir_rate: without the unit acg_set_channel_filter says ACG_ESTATE.
__attribute__((weak)) int acg_launch_fir_long(const FirLongArgs* a, void* stream);
#ifdef __cplusplus
}
#endif
