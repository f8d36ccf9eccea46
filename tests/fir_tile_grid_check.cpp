// Host check of acg_fir_tile_grid (acarsdec_amd/csrc/fir_plan.h), the one grid of resident workgroups of the tile down-converters:
// it gives what each of the six computations it replaced gave -- restated here literally, as acg_launch_fir, persist_grid,
// acg_launch_fir_shared, acg_launch_fir_fmt, acg_launch_fir_cf32 and grid_resident_blocks had them -- over CU counts, the
// context's ncu, LDS sizes from 1 KiB to 64 KiB, the caps, the wg_per_cu and ACG_FIR_WG_PER_CU overrides and channels x windows,
// ragged ones included.  Built with -fsanitize=address,undefined and run by tests/test_host_logic.py; prints the first violation.
#include <stdio.h>
#include <string.h>
struct int4;                    // acg_internal.h names HIP's vector types only behind pointers
struct uint2;
struct float2;
#include "fir_plan.h"

#define FIR_RUN 4               // fir_tile_kernel.h (a HIP header)

static int g_wg_per_cu = -1;    // ACG_FIR_WG_PER_CU; -1: not set
extern "C" int acg_tune_get(const char* name, int dflt)
{
    if (!strcmp(name, "ACG_FIR_WG_PER_CU") && g_wg_per_cu >= 0) return g_wg_per_cu;
    return dflt;
}
static int env_int(const char* name, int dflt) { return acg_tune_get(name, dflt); }

struct In {
    int nch, ngroups, nwin, ncu, wg_per_cu;
};

// ---- the six, as they were ----------------------------------------------------------------------------------------------------
// acg_launch_fir (fir.hip); *before_run: what the lab's variants 1 and 2 took
static long long old_launch_fir(const In* a, size_t lds, int num_cu, long long* before_run)
{
    int per_cu = (int)((160 * 1024) / lds);
    if (per_cu > 5) per_cu = 5;
    if (a->wg_per_cu > 0 && per_cu > a->wg_per_cu) per_cu = a->wg_per_cu;
    if (per_cu < 1) per_cu = 1;
    per_cu = env_int("ACG_FIR_WG_PER_CU", per_cu);
    const long long ntile = (a->nwin + ACG_TILE_WIN - 1) / ACG_TILE_WIN;
    const long long G = (long long)a->nch * ntile;
    long long grid = (long long)(a->ncu > 0 ? a->ncu : num_cu) * per_cu;
    if (grid > G) grid = G;
    *before_run = grid;
    const long long nrun = (G + FIR_RUN - 1) / FIR_RUN;
    if (grid > nrun) grid = nrun;
    return grid;
}
// persist_grid (fir_kernels.h)
static long long old_persist_grid(const In* a, size_t lds, int num_cu)
{
    int per_cu = (int)((160 * 1024) / lds);
    if (per_cu > 5) per_cu = 5;
    if (a->wg_per_cu > 0 && per_cu > a->wg_per_cu) per_cu = a->wg_per_cu;
    if (per_cu < 1) per_cu = 1;
    per_cu = env_int("ACG_FIR_WG_PER_CU", per_cu);
    const long long ntile = (a->nwin + ACG_TILE_WIN - 1) / ACG_TILE_WIN;
    const long long G = (long long)a->nch * ntile;
    const long long nrun = (G + FIR_RUN - 1) / FIR_RUN;
    long long grid = (long long)(a->ncu > 0 ? a->ncu : num_cu) * per_cu;
    if (grid > nrun) grid = nrun;
    return grid;
}
// acg_launch_fir_shared (fir.hip)
static long long old_launch_fir_shared(const In* a, size_t lds, int num_cu)
{
    int per_cu = (int)((160 * 1024) / lds);
    if (per_cu > 4) per_cu = 4;
    if (per_cu < 1) per_cu = 1;
    per_cu = env_int("ACG_FIR_WG_PER_CU", per_cu);
    const long long ntile = (a->nwin + ACG_TILE_WIN - 1) / ACG_TILE_WIN;
    const long long G = (long long)a->ngroups * ntile;
    const long long nrun = (G + FIR_RUN - 1) / FIR_RUN;
    long long grid = (long long)(a->ncu > 0 ? a->ncu : num_cu) * per_cu;
    if (grid > nrun) grid = nrun;
    return grid;
}
// acg_launch_fir_fmt (fir.hip) and, word for word, acg_launch_fir_cf32 (fir_iq.hip)
static long long old_launch_fir_fmt(const In* a, size_t lds, int num_cu)
{
    int per_cu = (int)((160 * 1024) / lds);
    if (per_cu > 4) per_cu = 4;
    const long long ntile = (a->nwin + ACG_TILE_WIN - 1) / ACG_TILE_WIN;
    const long long G = (long long)a->nch * ntile;
    long long grid = (long long)(a->ncu > 0 ? a->ncu : num_cu) * per_cu;
    if (grid > G) grid = G;
    return grid;
}
static long long old_launch_fir_cf32(const In* a, size_t lds, int num_cu)
{
    int per_cu = (int)((160 * 1024) / lds);
    if (per_cu > 4) per_cu = 4;
    const long long ntile = (a->nwin + ACG_TILE_WIN - 1) / ACG_TILE_WIN;
    const long long G = (long long)a->nch * ntile;
    long long grid = (long long)(a->ncu > 0 ? a->ncu : num_cu) * per_cu;
    if (grid > G) grid = G;
    return grid;
}
// grid_resident_blocks (fir_grid_kernel.h): per_cu_max 4 (rate) or 3 (filter), tile_out 64 or 64 - (nseg - 1)
static long long old_grid_resident_blocks(const In* a, size_t lds, int per_cu_max, int tile_out, int num_cu)
{
    int per_cu = (int)((160 * 1024) / lds);
    if (per_cu > per_cu_max) per_cu = per_cu_max;
    const long long ntile = (a->nwin + tile_out - 1) / tile_out;
    const long long G = (long long)a->nch * ntile;
    long long grid = (long long)(a->ncu > 0 ? a->ncu : num_cu) * per_cu;
    if (grid > G) grid = G;
    return grid;
}

static int fail(const In& a, size_t lds, int num_cu, const char* what, long long got, long long want)
{
    printf("nch %d ngroups %d nwin %d ncu %d wg_per_cu %d ACG_FIR_WG_PER_CU %d lds %zu device CUs %d: %s gives %lld, was %lld\n", a.nch, a.ngroups, a.nwin, a.ncu,
           a.wg_per_cu, g_wg_per_cu, lds, num_cu, what, got, want);
    return 1;
}

int main(void)
{
    static_assert(FIR_CU_LDS == 160 * 1024, "");
    static const int cus[] = {1, 8, 64, 228, 256, 304};
    static const int ncus[] = {0, 1, 24, 200};
    static const size_t ldss[] = {1024, 4096 + 16, 9232, 13328, 17424, 25616, 32768, 32769, 40976, 45072, 53264, 54613, 54614, 65536};
    static const int nchs[] = {1, 3, 40, 2048, 16384};
    static const int nwins[] = {1, 63, 64, 65, 100, 300, 1024, 4096, 16 * 1024 + 7};
    static const int wgs[] = {0, 1, 2, 7};
    static const int envs[] = {-1, 1, 3, 9};
    long long n = 0;
    for (int num_cu : cus) for (int ncu : ncus) for (size_t lds : ldss) for (int nch : nchs) for (int nwin : nwins) for (int wg : wgs) for (int env : envs) {
        g_wg_per_cu = env;
        const In a = {nch, (nch + 2) / 3, nwin, ncu, wg};
        const int c = ncu > 0 ? ncu : num_cu;
        const long long G = acg_fir_tile_units(a.nch, a.nwin, ACG_TILE_WIN), Gs = acg_fir_tile_units(a.ngroups, a.nwin, ACG_TILE_WIN);
        if (G != (long long)nch * ((nwin + 63) / 64)) return fail(a, lds, num_cu, "acg_fir_tile_units", G, (long long)nch * ((nwin + 63) / 64));
        long long before_run = 0, want = old_launch_fir(&a, lds, num_cu, &before_run), got;
        if ((got = acg_fir_tile_grid(c, lds, 5, a.wg_per_cu, true, G, FIR_RUN)) != want) return fail(a, lds, num_cu, "acg_launch_fir", got, want);
        if ((got = acg_fir_tile_grid(c, lds, 5, a.wg_per_cu, true, G)) != before_run) return fail(a, lds, num_cu, "acg_launch_fir (lab variants 1, 2)", got, before_run);
        if (got < want) return fail(a, lds, num_cu, "the run clamp widens the grid", got, want);
        if ((got = acg_fir_tile_grid(c, lds, 5, a.wg_per_cu, true, G, FIR_RUN)) != (want = old_persist_grid(&a, lds, num_cu))) return fail(a, lds, num_cu, "persist_grid", got, want);
        if ((got = acg_fir_tile_grid(c, lds, 4, 0, true, Gs, FIR_RUN)) != (want = old_launch_fir_shared(&a, lds, num_cu))) return fail(a, lds, num_cu, "acg_launch_fir_shared", got, want);
        if ((got = acg_fir_tile_grid(c, lds, 4, 0, false, G)) != (want = old_launch_fir_fmt(&a, lds, num_cu))) return fail(a, lds, num_cu, "acg_launch_fir_fmt", got, want);
        if (got != (want = old_launch_fir_cf32(&a, lds, num_cu))) return fail(a, lds, num_cu, "acg_launch_fir_cf32", got, want);
        for (int nseg = 1; nseg <= 4; ++nseg) {          // the rate kernel (four per CU), the channel filter over nseg windows (three)
            const int cap = nseg == 1 ? 4 : 3, tile_out = ACG_TILE_WIN - (nseg - 1);
            got = acg_fir_tile_grid(c, lds, cap, 0, false, acg_fir_tile_units(a.nch, a.nwin, tile_out));
            if (got != (want = old_grid_resident_blocks(&a, lds, cap, tile_out, num_cu))) return fail(a, lds, num_cu, "grid_resident_blocks", got, want);
        }
        n += 10;
    }
    printf("ok %lld grids\n", n);
    return 0;
}
