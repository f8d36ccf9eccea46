// Host check of acarsdec_amd/csrc/fir_grid.h, the one launch plan of the two grid down-converters (fir_rate.hip, fir_long.hip):
// it gives what the two plans it replaced gave -- restated here literally, as fir_rate.h and fir_long.h had them -- and what the
// kernels assume of it holds, for every decim x format x nseg (nseg 1: the rate kernel's plan).  Built with
// -fsanitize=address,undefined and run by tests/test_host_logic.py; prints the first violation.
#include <stdio.h>
struct int4;                    // acg_internal.h names HIP's vector types only behind pointers
struct uint2;
struct float2;
#include "acarsdec_amd.h"
#include "fir_grid.h"

struct Plan {
    int bps, cpr_total, kseg, cpr, row_stride;
    unsigned int ld_magic;
    size_t lds;
};

static int old_bps(int fmt) { return fmt == RATE_CF32 ? 8 : fmt == RATE_CS16 ? 4 : 2; }

static Plan old_rate_plan(int fmt, int decim)
{
    Plan p;
    p.bps = old_bps(fmt);
    p.cpr_total = (decim * p.bps + 15) / 16;
    p.kseg = (p.cpr_total + 50) / 51;
    p.cpr = (p.cpr_total + p.kseg - 1) / p.kseg;
    const int slots = p.cpr + 2;
    p.row_stride = 16 * ((slots & 1) ? slots : slots + 1);
    p.ld_magic = ((1u << 20) + (unsigned int)p.cpr) / (unsigned int)(p.cpr + 1);
    p.lds = (size_t)ACG_TILE_WIN * p.row_stride + 4 * 64 * 16 + 2 * 72 * sizeof(int);
    return p;
}

static Plan old_long_plan(int fmt, int decim, int nseg)
{
    Plan p;
    p.bps = old_bps(fmt);
    p.cpr_total = (decim * p.bps + 15) / 16;
    for (p.kseg = (p.cpr_total + 34) / 35;; ++p.kseg) {
        p.cpr = (p.cpr_total + p.kseg - 1) / p.kseg;
        const int slots = p.cpr + 2;
        p.row_stride = 16 * ((slots & 1) ? slots : slots + 1);
        p.lds = (size_t)ACG_TILE_WIN * p.row_stride + (size_t)4 * nseg * 64 * 16;
        if (p.lds <= ((160 * 1024) / 3) || p.cpr == 1) break;
    }
    p.ld_magic = ((1u << 20) + (unsigned int)p.cpr) / (unsigned int)(p.cpr + 1);
    return p;
}

static int fail(int fmt, int decim, int nseg, const FirGridArgs& a, size_t lds, const char* what)
{
    printf("fmt %d decim %d nseg %d: %s  (bps %d cpr_total %d kseg %d cpr %d row_stride %d ld_magic %u lds %zu)\n", fmt, decim, nseg, what, a.bps,
           a.cpr_total, a.kseg, a.cpr, a.row_stride, a.ld_magic, lds);
    return 1;
}

int main(void)
{
    static_assert(ACG_LONG_MAXSEG == ACG_MAXSEG && ACG_LONG_LDS_MAX == (160 * 1024) / 3 && RATE_CPR_MAX == 51 && LONG_CPR_MAX == 35, "");
    static const float scale[4] = {1.0f / 127.5f, 1.0f / 128.0f, 1.0f / 32768.0f, 1.0f};
    long long n = 0;
    for (int fmt = RATE_CU8; fmt <= RATE_CF32; ++fmt) {
        if (ACG_FIR_GRID_FMT[fmt].bps != old_bps(fmt) || ACG_FIR_GRID_FMT[fmt].scale != scale[fmt]) return printf("fmt %d: bps or scale_fmt\n", fmt), 1;
        // the rate entry points admit decim <= ACG_MAXDECIM; the plan holds what it promises up to the sample formats' limit
        for (int decim = 2; decim <= ACG_MAXDECIM_SAMPLES; ++decim)
            for (int nseg = 1; nseg <= ACG_LONG_MAXSEG; ++nseg, ++n) {
                FirRateArgs r{};
                FirLongArgs l{};
                FirGridArgs& a = nseg == 1 ? (FirGridArgs&)r : l;
                a.fmt = fmt;
                a.decim = decim;
                l.nseg = nseg;
                if (nseg == 1) acg_fir_rate_plan(&r); else acg_fir_long_plan(&l);
                const size_t lds = nseg == 1 ? acg_fir_rate_lds(&r) : acg_fir_long_lds(&l);
                const Plan p = nseg == 1 ? old_rate_plan(fmt, decim) : old_long_plan(fmt, decim, nseg);
                const int cap = nseg == 1 ? 51 : 35;
                if (a.bps != p.bps || a.cpr_total != p.cpr_total || a.kseg != p.kseg || a.cpr != p.cpr || a.row_stride != p.row_stride ||
                    a.ld_magic != p.ld_magic || lds != p.lds)
                    return fail(fmt, decim, nseg, a, lds, "not the plan of fir_rate.h / fir_long.h");
                if (a.kseg * a.cpr < a.cpr_total) return fail(fmt, decim, nseg, a, lds, "the slices do not hold the window");
                if (a.cpr < 1 || a.cpr > cap) return fail(fmt, decim, nseg, a, lds, "more chunks per slice than the staging registers hold");
                if (!((a.row_stride / 16) & 1) || a.row_stride < 16 * (a.cpr + 2)) return fail(fmt, decim, nseg, a, lds, "row stride");
                for (unsigned int c = 0; c < 64u * (unsigned int)(a.cpr + 1); ++c)
                    if (((c * a.ld_magic) >> 20) != c / (unsigned int)(a.cpr + 1)) return fail(fmt, decim, nseg, a, lds, "ld_magic is not the division");
                if (nseg > 1 && lds > ACG_LONG_LDS_MAX && a.cpr != 1) return fail(fmt, decim, nseg, a, lds, "the filter's LDS above a third of a CU's");
            }
    }
    printf("ok %lld plans\n", n);
    return 0;
}
