// fir_iq.hip -- the recordings' sample formats on the down-converter's kernel templates (fir_kernels.h):
//   ACG_FMT_CS8   interleaved int8 I,Q (SigMF ci8, HackRF): the u8 kernels with the signed switch -- the wave-private streaming
//                 kernel at decim 160 / 192 / 200, the workgroup-granular kernel at the other multiples of 8 and for ragged
//                 launches, the shared-stream vector kernel (the matrix-pipe kernel is fir_mm.hip's fir_s8_mm_kernel);
//   ACG_FMT_CF32  interleaved float32 I,Q (SigMF cf32_le, GNU Radio .cfile, SoapySDR CF32): fir_fmt_direct_kernel<FMT_CF32, 80 /
//                 96 / 100, 16> and fir_fmt_kernel<FMT_CF32>.
// A unit of its own, reached only through fir.hip's launchers: its code objects are stored as a compressed bundle (the flags in
// _build.py), so that the library's size grows by a quarter of what eleven more kernel instantiations weigh.
#include <hip/hip_runtime.h>
#include "acg_internal.h"
#include "fir_plan.h"
#include "fir_kernels.h"

template <int CPR>
static int launch_s8_direct(const FirArgs* a, int num_cu, hipStream_t stream)
{
    const FirWavePlan p = acg_fir_wave_plan(a, num_cu, FirD<CPR>::WAVE_LDS, ACG_TILE_WIN, 8);
    return launch_planned(fir_s8_direct_kernel<CPR>, p, *a, stream);
}

// The same two kernels behind the same rules as acg_launch_fir's u8 path: the streaming kernel for whole two-tile bodies at a
// window length it is instantiated for (ACG_FIR_VARIANT=3 forces the other), else the workgroup-granular one.
extern "C" int acg_launch_fir_s8(const FirArgs* a, void* stream)
{
    const size_t lds = acg_fir_lds_bytes(a);
    int num_cu = 0;
    if (int e = acg_fir_device_cus(&num_cu)) return e;
    if (env_int("ACG_FIR_VARIANT", 5) != 3 && acg_fir_u8_wave_takes(a)) {
        switch (a->cpr) {
        case 20: return launch_s8_direct<20>(a, num_cu, (hipStream_t)stream);
        case 24: return launch_s8_direct<24>(a, num_cu, (hipStream_t)stream);
        case 25: return launch_s8_direct<25>(a, num_cu, (hipStream_t)stream);
        default: break;
        }
    }
    long long grid = 0;
    if (int e = persist_grid(a, lds, num_cu, &grid)) return e;
    if (a->nwin % ACG_TILE_WIN == 0)      // whole callbacks: every tile is complete
        FIR_LAUNCH((fir_u8_persist_kernel<true, true, true, true>), dim3((unsigned int)grid), dim3(ACG_WG_FIR), lds, (hipStream_t)stream, *a,
                   a->iq, a->taps, a->stream_of, a->dm);
    else
        FIR_LAUNCH((fir_u8_persist_kernel<true, true, false, true>), dim3((unsigned int)grid), dim3(ACG_WG_FIR), lds, (hipStream_t)stream, *a,
                   a->iq, a->taps, a->stream_of, a->dm);
    return (int)hipGetLastError();
}

// grid and lds: as acg_launch_fir_shared sized them
extern "C" int acg_launch_fir_shared_s8(const FirArgs* a, long long grid, size_t lds, void* stream)
{
    if (a->nwin % ACG_TILE_WIN == 0)
        FIR_LAUNCH((fir_u8_shared_kernel<true, true>), dim3((unsigned int)grid), dim3(ACG_WG_FIR), lds, (hipStream_t)stream, *a, a->iq,
                   a->gtaps, a->groups, a->group_ch, a->dm);
    else
        FIR_LAUNCH((fir_u8_shared_kernel<false, true>), dim3((unsigned int)grid), dim3(ACG_WG_FIR), lds, (hipStream_t)stream, *a, a->iq,
                   a->gtaps, a->groups, a->group_ch, a->dm);
    return (int)hipGetLastError();
}

// acg_launch_fir_fmt's two steps for complex float32: the streaming kernel where it is instantiated for the window length and
// the launch is whole runs, else the workgroup-granular kernel
extern "C" int acg_launch_fir_cf32(const FirArgs* a, void* stream)
{
    const size_t lds = (size_t)ACG_TILE_WIN * a->row_stride + 4 * 64 * sizeof(float4);
    int num_cu = 0;
    if (int e = acg_fir_device_cus(&num_cu)) return e;
    if (env_int("ACG_FIR_VARIANT", 5) >= 5) {
#define FIRX_TRY(F_, C_, W_) \
        if (a->cpr_total == C_ && acg_fir_fmt_wave_takes(a, W_)) return launch_fmt_direct<F_, C_, W_>(a, num_cu, (hipStream_t)stream);
        FIRX_LIST_IQ(FIRX_TRY)
#undef FIRX_TRY
    }
    if (lds > 64 * 1024) return (int)hipErrorInvalidValue;
    int per_cu = (int)((160 * 1024) / lds);
    if (per_cu > 4) per_cu = 4;
    const long long ntile = (a->nwin + ACG_TILE_WIN - 1) / ACG_TILE_WIN;
    const long long G = (long long)a->nch * ntile;
    long long grid = (long long)(a->ncu > 0 ? a->ncu : num_cu) * per_cu;
    if (grid > G) grid = G;
    return launch_fmt<FMT_CF32>(a, grid, lds, (hipStream_t)stream);
}
