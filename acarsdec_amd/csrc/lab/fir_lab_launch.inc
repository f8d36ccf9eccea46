// csrc/lab/fir_lab_launch.inc -- the launchers of the lab variants: LAB BUILD ONLY (libacarsdec_amd_lab.so, -DACG_LAB).  Textually included by fir.hip, which
// provides the helpers it uses; the product library never sees this file (tests/test_host_logic.py compares the product's
// kernel list; the product object is byte-identical with and without it).
// register-resident taps (ACG_FIR_VARIANT=7 / 8, 2.5 Msps): 13 / 17 KiB of LDS per wave
// (twelve waves per CU fit and measure 1-6 % slower than eight, alone and beside the demodulator: profiles/r02_experiments)
template <bool FOLD = true, int UU = 13, int BB = 1, bool STAGED = false>
static int launch_coltap(const FirArgs* a, int num_cu, hipStream_t stream)
{
    constexpr int WAVE_LDS = STAGED ? FirC<UU, BB>::WAVE_LDS_STAGED : FirC<UU, BB>::WAVE_LDS;
    static_assert(4 * WAVE_LDS <= FIR_CU_LDS, "a four-wave workgroup fits a CU: the plan's fit is >= 1");
    const FirWavePlan p = acg_fir_wave_plan(a, num_cu, WAVE_LDS, ACG_TILE_WIN, 8);
    if (acg_tune_has("ACG_FIR_DEBUG_SHAPE"))
        fprintf(stderr, "fir_u8_coltap: nch %d nwin %d  wpg %d per_cu %d grid %lld  bodies/ch %lld pairs %d runs %lld  shares_cus %d prio %d lds %zu\n",
                a->nch, a->nwin, p.wpg, p.per_cu, p.grid, p.bodies_per_ch, p.pairs, p.nrun, a->shares_cus, a->high_prio, p.lds);
    return launch_planned(fir_u8_coltap_kernel<FOLD, UU, BB, STAGED>, p, *a, stream);
}

// matrix-pipe variant (ACG_FIR_VARIANT=6): as many waves as the LDS holds, twelve per CU at most (9 at 2.5 Msps)
template <int CPR>
static int launch_mfma(const FirArgs* a, int num_cu, hipStream_t stream)
{
    static_assert(4 * FirM<CPR>::WAVE_LDS <= FIR_CU_LDS, "a four-wave workgroup fits a CU: the plan's fit is >= 1");
    const FirWavePlan p = acg_fir_wave_plan(a, num_cu, FirM<CPR>::WAVE_LDS, ACG_TILE_WIN, 12);
    if (acg_tune_has("ACG_FIR_DEBUG_SHAPE"))
        fprintf(stderr, "fir_u8_mfma<%d>: nch %d nwin %d  wpg %d per_cu %d grid %lld pairs %d runs %lld lds %zu\n", CPR, a->nch, a->nwin, p.wpg, p.per_cu, p.grid, p.pairs,
                p.nrun, p.lds);
    return launch_planned(fir_u8_mfma_kernel<CPR>, p, *a, stream);
}
