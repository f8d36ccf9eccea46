// fir_plan.h -- the shape of one launch of a wave-private down-converter (fir.hip: fir_u8_direct_kernel, fir_fmt_direct_kernel and the
// lab's fir_u8_coltap_kernel / fir_u8_mfma_kernel), decided in ONE place, and which launches those kernels take.  Host arithmetic
// only, inline, nothing of HIP: tests/fir_plan_check.cpp compiles it for the host and holds it to what the kernels assume
// (their comments say "(launcher)").  The matrix-pipe kernels' plan is fir_mm_plan.h.
#ifndef ACG_FIR_PLAN_H
#define ACG_FIR_PLAN_H

#include "acg_internal.h"

extern "C" int acg_tune_get(const char* name, int dflt);          // measurement / layout switches (acg_api.cpp)

#define FIRD_R 2                // tiles per body: a wave walks its run two tiles at a time
#define FIR_CU_LDS (160 * 1024)

struct FirWavePlan {
    int wpg;                    // waves per workgroup: 1, 2 or 4
    int fit;                    // workgroups per CU that LDS and the wave cap allow (0: not even one)
    int per_cu;                 // ... and what the launch is sized for (ACG_FIR_WG_PER_CU overrides)
    size_t lds;                 // dynamic LDS bytes per workgroup
    long long grid;             // workgroups
    long long bodies_per_ch;    // two-tile bodies per channel
    int pairs;                  // bodies per dispensed run: 1, 2, 4 or 8, divides bodies_per_ch
    long long nrun;             // nch * bodies_per_ch / pairs
};

// wave_lds: the kernel's LDS bytes per wave; tile_win: windows per tile; cap: most waves per CU (8, the matrix-pipe lab kernel 12)
static inline FirWavePlan acg_fir_wave_plan(const FirArgs* a, int device_cus, int wave_lds, int tile_win, int cap)
{
    FirWavePlan p;
    // The waves of a workgroup are independent, so the workgroup size only decides in what pieces LDS is handed out
    // (ACG_FIR_WAVES_PER_WG = 1, 2, 4).  Four measured best alone (+5 % over single-wave workgroups at 16 384
    // channels) and within noise of the others beside the demodulator.  At most 8 waves per CU (2 per SIMD).
    // Beside demodulator workgroups on the same CUs (no CU partition: > 2048 channels) single-wave workgroups, seven per
    // CU: the demodulator's LDS (28 KiB per CU at 16 384 channels) then fits next to them instead of keeping a whole
    // 4-wave workgroup out (+13 % whole job at 4096 channels, +2 % at 16 384).
    p.wpg = acg_tune_get("ACG_FIR_WAVES_PER_WG", a->shares_cus ? 1 : 4);
    if (p.wpg != 1 && p.wpg != 2 && p.wpg != 4) p.wpg = 4;
    p.lds = (size_t)p.wpg * (size_t)wave_lds;
    p.fit = (int)(FIR_CU_LDS / p.lds);
    if (p.fit > cap / p.wpg) p.fit = cap / p.wpg;
    if (a->shares_cus && p.wpg == 1 && p.fit > 7) p.fit = 7;
    p.per_cu = acg_tune_get("ACG_FIR_WG_PER_CU", p.fit);
    p.grid = (long long)(a->ncu > 0 ? a->ncu : device_cus) * p.per_cu;
    // two-tile bodies per run: as many (1, 2, 4, 8) as leave every resident wave ~32 runs (the tail of the launch is
    // one run long) and divide the bodies of a channel
    p.bodies_per_ch = a->nwin / tile_win / FIRD_R;
    const long long bodies = (long long)a->nch * p.bodies_per_ch;
    p.pairs = 1;
    while (p.pairs < 8 && p.bodies_per_ch % (2 * p.pairs) == 0 && bodies / (2 * p.pairs) >= 32 * p.grid * p.wpg) p.pairs *= 2;
    p.pairs = acg_tune_get("ACG_FIR_RUN_PAIRS", p.pairs);
    if (p.pairs < 1 || p.pairs > 8 || (p.pairs & (p.pairs - 1)) || p.bodies_per_ch % p.pairs) p.pairs = 1;      // 1, 2, 4 or 8
    p.nrun = bodies / p.pairs;
    const long long need = (p.nrun + p.wpg - 1) / p.wpg;
    if (p.grid > need) p.grid = need;
    return p;
}

// The u8 wave-private kernels take whole two-tile bodies of 64 windows, (channel, tile) below 2^31 and no more taps than the window
static inline bool acg_fir_u8_wave_takes(const FirArgs* a)
{
    return a->nwin > 0 && a->nwin % ACG_TILE_WIN == 0 && (a->nwin / ACG_TILE_WIN) % FIRD_R == 0 &&
           (long long)a->nch * (a->nwin / ACG_TILE_WIN) < (1ll << 31) && a->ntaps_pad <= a->decim;
}

// The format kernels (tiles of tile_win windows): whole bodies, (channel, window) below 2^31
static inline bool acg_fir_fmt_wave_takes(const FirArgs* a, int tile_win)
{
    return a->nwin > 0 && (long long)a->nch * a->nwin < (1ll << 31) && a->nwin % (tile_win * FIRD_R) == 0;
}

// ---- the tile kernels (fir_tile_kernel.h, fir_grid_kernel.h): a grid of resident workgroups ------------------------------------
// the (unit, tile) space of a launch: nunits channels or groups, tiles of tile_out outputs
static inline long long acg_fir_tile_units(int nunits, int nwin, int tile_out)
{
    return (long long)nunits * ((nwin + tile_out - 1) / tile_out);
}

// As many workgroups as stay resident: on each of `cus` CUs (the context's partition, else the device's) what the LDS bytes of a
// workgroup allow, `cap` at most (the kernel's VGPR budget), and no more than there are runs of `run` units.  tunable: the u8
// kernels' -- the context's wg_per_cu (0: none) bounds it too, never below one, and ACG_FIR_WG_PER_CU overrides the lot.
static inline long long acg_fir_tile_grid(int cus, size_t lds, int cap, int wg_per_cu, bool tunable, long long units, int run = 1)
{
    int per_cu = (int)(FIR_CU_LDS / lds);
    if (per_cu > cap) per_cu = cap;
    if (tunable) {
        if (wg_per_cu > 0 && per_cu > wg_per_cu) per_cu = wg_per_cu;
        if (per_cu < 1) per_cu = 1;
        per_cu = acg_tune_get("ACG_FIR_WG_PER_CU", per_cu);
    }
    const long long grid = (long long)cus * per_cu, nrun = (units + run - 1) / run;
    return grid > nrun ? nrun : grid;
}

#endif /* ACG_FIR_PLAN_H */
