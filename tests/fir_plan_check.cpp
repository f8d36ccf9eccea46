// Host check of acarsdec_amd/csrc/fir_plan.h, the launch plan of the wave-private down-converters: what the kernels assume of
// their launcher (their comments say "(launcher)") holds for every shape of the sweep.  Built with -fsanitize=address,undefined
// and run by tests/test_host_logic.py; prints the first violation.
#include <stdio.h>
#include <string.h>
struct int4;                    // acg_internal.h names HIP's vector types only behind pointers
struct uint2;
struct float2;
#include "fir_plan.h"

// ---- the tune table: the two overrides of the sweep (-1: unset)
static int g_waves_per_wg = -1, g_run_pairs = -1;
extern "C" int acg_tune_get(const char* name, int dflt)
{
    if (!strcmp(name, "ACG_FIR_WAVES_PER_WG") && g_waves_per_wg >= 0) return g_waves_per_wg;
    if (!strcmp(name, "ACG_FIR_RUN_PAIRS") && g_run_pairs >= 0) return g_run_pairs;
    return dflt;
}

// ---- LDS bytes per wave, as fir.hip's FirD / FirX / FirC / FirM form them
static constexpr int odd(int n) { return (n & 1) ? n : n + 1; }
static constexpr int fird_lds(int cpr) { return 4 * (cpr + 63) * 16 + 64 * odd(cpr) * 8; }
static constexpr int firx_lds(int npl, int cpr, int w) { return npl * (cpr + 63) * 16 + 64 * odd(cpr / (64 / w)) * 8; }
static constexpr int firc_lds(bool staged) { return (((64 * 25 + 28) * 8 + 15) & ~15) + (staged ? 16 * 256 + 16 * 8 : 0); }
static constexpr int firm_lds(int cpr) { return ((32 * cpr + 63) / 64) * 1024 + 2 * ((cpr + 1) / 2) * 128 + 2 * 32 * 16; }

struct Inst {
    const char* name;
    int wave_lds, w, cap;
};
static const Inst INST[] = {
    {"fir_u8_direct_kernel<20>", fird_lds(20), 64, 8},        {"fir_u8_direct_kernel<24>", fird_lds(24), 64, 8},
    {"fir_u8_direct_kernel<25>", fird_lds(25), 64, 8},        {"fir_fmt_direct_kernel<CS16, 40, 32>", firx_lds(2, 40, 32), 32, 8},
    {"fir_fmt_direct_kernel<CS16, 48, 32>", firx_lds(2, 48, 32), 32, 8}, {"fir_fmt_direct_kernel<CS16, 50, 32>", firx_lds(2, 50, 32), 32, 8},
    {"fir_fmt_direct_kernel<F32R, 50, 32>", firx_lds(2, 50, 32), 32, 8}, {"fir_fmt_direct_kernel<F32R, 60, 16>", firx_lds(2, 60, 16), 16, 8},
    {"fir_fmt_direct_kernel<F32R, 120, 8>", firx_lds(2, 120, 8), 8, 8},  {"fir_fmt_direct_kernel<F32R, 200, 8>", firx_lds(2, 200, 8), 8, 8},
    {"fir_fmt_direct_kernel<SPLIT, 20, 64>", firx_lds(4, 20, 64), 64, 8}, {"fir_u8_coltap_kernel", firc_lds(false), 64, 8},
    {"fir_u8_coltap_kernel (staged)", firc_lds(true), 64, 8}, {"fir_u8_mfma_kernel<25>", firm_lds(25), 64, 12},
};

static int fail(const Inst& in, const FirArgs& a, const FirWavePlan& p, const char* what)
{
    printf("%s nch %d nwin %d ncu %d shares_cus %d WAVES_PER_WG %d RUN_PAIRS %d: %s  (wpg %d fit %d per_cu %d lds %zu grid %lld bodies/ch %lld pairs %d nrun %lld)\n",
           in.name, a.nch, a.nwin, a.ncu, a.shares_cus, g_waves_per_wg, g_run_pairs, what, p.wpg, p.fit, p.per_cu, p.lds, p.grid, p.bodies_per_ch,
           p.pairs, p.nrun);
    return 1;
}

int main(void)
{
    static const int NCH[] = {1, 2, 5, 300, 1024, 16384}, NCU[] = {0, 8, 80, 176, 256};
    static const int WPG[] = {-1, 1, 2, 3, 4}, PAIRS[] = {-1, 1, 2, 3, 8, 16};
    const int device_cus = 256;
    long long n = 0;
    for (const Inst& in : INST)
        for (int nch : NCH)
            for (int blk = 1; blk <= 8; ++blk)
                for (int ncu : NCU)
                    for (int shares = 0; shares <= 1; ++shares)
                        for (int wpg : WPG)
                            for (int pairs : PAIRS) {
                                FirArgs a;
                                memset(&a, 0, sizeof(a));
                                a.nch = nch;
                                a.nwin = 1024 * blk;
                                a.ncu = ncu;
                                a.shares_cus = shares;
                                a.ntaps_pad = a.decim = 200;
                                g_waves_per_wg = wpg;
                                g_run_pairs = pairs;
                                const FirWavePlan p = acg_fir_wave_plan(&a, device_cus, in.wave_lds, in.w, in.cap);
                                ++n;
                                if (!acg_fir_fmt_wave_takes(&a, in.w) || (in.w == ACG_TILE_WIN && !acg_fir_u8_wave_takes(&a)))
                                    return fail(in, a, p, "a whole callback is not taken");
                                if (p.wpg != 1 && p.wpg != 2 && p.wpg != 4) return fail(in, a, p, "wpg is not 1, 2 or 4");
                                if (p.lds != (size_t)p.wpg * (size_t)in.wave_lds) return fail(in, a, p, "lds is not wpg * the wave's bytes");
                                if (p.fit < 1) return fail(in, a, p, "no workgroup fits a CU");
                                if (p.pairs != 1 && p.pairs != 2 && p.pairs != 4 && p.pairs != 8) return fail(in, a, p, "pairs is not 1, 2, 4 or 8");
                                if (p.bodies_per_ch != a.nwin / in.w / FIRD_R || p.bodies_per_ch % p.pairs) return fail(in, a, p, "pairs does not divide the bodies of a channel");
                                if (p.nrun != (long long)a.nch * p.bodies_per_ch / p.pairs || p.nrun >= (1ll << 31)) return fail(in, a, p, "nrun");
                                if (p.grid < 1 || p.grid > (p.nrun + p.wpg - 1) / p.wpg) return fail(in, a, p, "grid outside 1 .. ceil(nrun / wpg)");
                                if (p.wpg * p.per_cu > in.cap) return fail(in, a, p, "more waves per CU than the cap");
                                if (p.lds * (size_t)p.per_cu > (size_t)FIR_CU_LDS) return fail(in, a, p, "more LDS per CU than 160 KiB");
                            }
    // what is not a whole two-tile body, or too large, is not taken
    FirArgs a;
    memset(&a, 0, sizeof(a));
    a.nch = 4;
    a.ntaps_pad = a.decim = 200;
    const int bad_nwin[] = {0, -64, 64, 100, 192};
    for (int nwin : bad_nwin) {
        a.nwin = nwin;
        if (acg_fir_u8_wave_takes(&a) || acg_fir_fmt_wave_takes(&a, 64)) return printf("nwin %d is taken\n", nwin), 1;
    }
    a.nwin = 1024;
    a.ntaps_pad = 208;
    if (acg_fir_u8_wave_takes(&a)) return printf("more taps than the window are taken\n"), 1;
    a.ntaps_pad = 200;
    a.nch = 1 << 27;
    if (acg_fir_u8_wave_takes(&a) || acg_fir_fmt_wave_takes(&a, 64)) return printf("2^31 tiles are taken\n"), 1;
    printf("ok %lld plans\n", n);
    return 0;
}
