// fir_mm_plan.h -- the shape of one launch of a matrix-pipe down-converter (fir_mm.hip), decided in ONE place: the launchers launch what
// these functions say, acg_lab_fir_launch_shape (acg_api.cpp) reports it.  Host arithmetic only, inline: the API unit needs no
// symbol of the kernel units for it.  The caller has checked acg_fir_mm_takes / acg_fir_mm1_takes.
#ifndef ACG_FIR_MM_PLAN_H
#define ACG_FIR_MM_PLAN_H

#include "acg_internal.h"

extern "C" int acg_tune_get(const char* name, int dflt);          // measurement / layout switches (acg_api.cpp)

struct MmPlan {
    int kernel;                 // 1 fir_u8_mm_kernel, 2 fir_u8_mm1_kernel
    int stages;                 // tiles in flight per wave (the kernel's STAGES; 1 for fir_u8_mm1_kernel)
    int cpr;                    // the kernel's CPR = decim / 8
    int ncu;                    // CUs the launch is sized for
    unsigned int units;         // groups (fir_u8_mm_kernel) or channels (fir_u8_mm1_kernel)
    unsigned int runs_per_unit;
    unsigned int tiles_per_run; // 32-window tiles per dispensed run
    unsigned int runs;          // units * runs_per_unit
    unsigned int wave_slots;    // resident waves the run length is sized for (ncu * waves per CU)
    unsigned int workgroups;    // the grid
    unsigned int waves;         // waves launched: the first `waves` runs are nobody's ticket
};

// fir_u8_mm_kernel<CPR, STAGES> (device_cus: the CUs of the device, used where the launch has no CU mask)
static inline MmPlan acg_fir_mm_plan(const FirArgs* a, int device_cus)
{
    // beside the demodulator on the same CUs: one wave per SIMD with two tiles in flight (see the kernel's comment)
    const int stages = acg_tune_get("ACG_FIR_MM_STAGES", a->shares_cus ? 2 : 1) == 2 ? 2 : 1;
    const int ncu = a->ncu > 0 ? a->ncu : device_cus;
    const unsigned int nwaves = (unsigned int)ncu * (stages == 1 ? 8u : 4u);
    const unsigned int ntile = (unsigned int)a->nwin / 32u;          // (FirMM<CPR>::WIN)
    // ~4 runs per wave where the launch is large enough, at least two tiles per run (a run pays one tile of load latency
    // and 26 KiB of digits from L2)
    unsigned int rpg = 1;
    while (rpg * 2 * (unsigned int)a->ngroups <= 4 * nwaves && ntile % (rpg * 2) == 0 && ntile / (rpg * 2) >= 2) rpg *= 2;
    const unsigned long long nrun = (unsigned long long)a->ngroups * rpg;
    const unsigned int need = (unsigned int)((nrun + 3) / 4);
    const unsigned int blocks = (unsigned int)ncu * (stages == 1 ? 2u : 1u);
    MmPlan p;
    p.kernel = 1;
    p.stages = stages;
    p.cpr = a->decim / 8;
    p.ncu = ncu;
    p.units = (unsigned int)a->ngroups;
    p.runs_per_unit = rpg;
    p.tiles_per_run = ntile / rpg;
    p.runs = (unsigned int)nrun;
    p.wave_slots = nwaves;
    p.workgroups = need < blocks ? need : blocks;
    p.waves = p.workgroups * 4u;
    return p;
}

// fir_u8_mm1_kernel<CPR>
static inline MmPlan acg_fir_mm1_plan(const FirArgs* a, int device_cus)
{
    const int ncu = a->ncu > 0 ? a->ncu : device_cus;
    // 13.2 KiB of LDS and 160 VGPRs per wave: twelve fit a CU that the demodulator does not share (<= 2048 channels: measured
    // 8 / 10 / 12 waves 2.30 / 2.33 / 2.46 M channel*Msps at 2048 channels); beside the demodulator's workgroups (15.4 KiB each: two
    // per CU up to 4096 channels, four from 8192) nine or seven (profiles/r06_mm1_waves_ab_*.json)
    int per_cu = !a->shares_cus ? 12 : a->nch >= 8192 ? 7 : 9;
    per_cu = acg_tune_get("ACG_FIR_MM1_WAVES", per_cu);
    if (per_cu < 1 || per_cu > 12) per_cu = 8;
    const unsigned int nwaves = (unsigned int)ncu * (unsigned int)per_cu;
    const unsigned int ntile = (unsigned int)a->nwin / 32u;          // (FirMM<CPR>::WIN)
    unsigned int rpc = 1;                                            // ~4 runs per wave, at least 8 tiles per run
    while (rpc * 2 * (unsigned int)a->nch <= 4 * nwaves && ntile % (rpc * 2) == 0 && ntile / (rpc * 2) >= 8) rpc *= 2;
    const unsigned long long nrun = (unsigned long long)a->nch * rpc;
    MmPlan p;
    p.kernel = 2;
    p.stages = 1;
    p.cpr = a->decim / 8;
    p.ncu = ncu;
    p.units = (unsigned int)a->nch;
    p.runs_per_unit = rpc;
    p.tiles_per_run = ntile / rpc;
    p.runs = (unsigned int)nrun;
    p.wave_slots = nwaves;
    p.workgroups = nrun < nwaves ? (unsigned int)nrun : nwaves;
    p.waves = p.workgroups;
    return p;
}

#endif /* ACG_FIR_MM_PLAN_H */
