// fir_iq.hip -- the recordings' sample formats on the down-converter's kernel templates (the tile kernels of fir_tile_kernel.h, the
// streaming kernels of fir_kernels.h):
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
#include "fir_tile_kernel.h"
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
    int num_cu = 0;
    if (int e = acg_fir_device_cus(&num_cu)) return e;
    if (env_int("ACG_FIR_VARIANT", 5) != 3 && acg_fir_u8_wave_takes(a)) {
#define FIRD_TRY(C_) if (a->cpr == C_) return launch_s8_direct<C_>(a, num_cu, (hipStream_t)stream);
        FIRD_LIST(FIRD_TRY)
#undef FIRD_TRY
    }
    return launch_persist<true>(*a, a, num_cu, (hipStream_t)stream);
}

// grid and lds: as acg_launch_fir_shared sized them
extern "C" int acg_launch_fir_shared_s8(const FirArgs* a, long long grid, size_t lds, void* stream)
{
    return launch_whole_or_ragged(fir_u8_shared_kernel<true, true>, fir_u8_shared_kernel<false, true>, a->nwin, grid, lds, (hipStream_t)stream, *a, a->iq,
                                  a->gtaps, a->groups, a->group_ch, a->dm);
}

// acg_launch_fir_fmt's two steps for complex float32: the streaming kernel where it is instantiated for the window length and
// the launch is whole runs, else the workgroup-granular kernel
extern "C" int acg_launch_fir_cf32(const FirArgs* a, void* stream)
{
    int num_cu = 0;
    if (int e = acg_fir_device_cus(&num_cu)) return e;
    if (env_int("ACG_FIR_VARIANT", 5) >= 5) {
#define FIRX_TRY(F_, C_, W_) \
        if (a->cpr_total == C_ && acg_fir_fmt_wave_takes(a, W_)) return launch_fmt_direct<F_, C_, W_>(a, num_cu, (hipStream_t)stream);
        FIRX_LIST_IQ(FIRX_TRY)
#undef FIRX_TRY
    }
    return launch_fmt<FMT_CF32>(a, num_cu, (hipStream_t)stream);
}
