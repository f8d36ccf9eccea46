// fir.hip -- the RTL down-converter on gfx950: u8 I/Q -> (x-127.37) -> per channel
// D = sum_k vb[k]*wf[k] over a window of M input samples -> |D|   (rtl.c:332-354).
//
// Shape of the problem: each input byte is used once per channel (taps == decimation), 8 flop per
// 2 bytes -> HBM-read bound, no data reuse, no MFMA (1-D convolution).  Design:
//   * a workgroup (4 waves) owns a contiguous run of 64-window tiles of ONE channel and walks it
//     in time (persistent over its segment);
//   * a tile (64 windows x 2M bytes, contiguous in HBM) is fetched with 16-byte coalesced loads,
//     staged through registers into LDS rows whose stride is an odd number of 16-byte slots, so
//     that "lane = window" ds_read_b128 reads are bank-conflict free;
//   * the loads of tile t+1 are issued before tile t is computed and only waited for at the LDS
//     write (issue-early / write-late), so HBM latency hides under the VALU work;
//   * inside a wave every lane is at the same tap index, so taps are wave-uniform: they come in
//     through scalar loads (SGPRs), not VGPRs or LDS;
//   * the 4 waves split the tap range; partial sums meet in LDS; wave 0 takes |D| and writes 64
//     consecutive floats of dm.
// That is the tile family (fir_tile_kernel.h: fir_u8_persist_kernel, fir_u8_shared_kernel, fir_fmt_kernel, and the parts they
// are made of); the default for whole callbacks at the documented rates is the wave-private streaming family (fir_kernels.h).
// This unit instantiates both for u8 I/Q and the front ends' sample formats, holds the per-device launch state, the launchers
// (their grid: fir_plan.h) and the exact-order kernel.
#include <hip/hip_runtime.h>
#include <map>
#include <mutex>
#include <cstdio>
#include <stdlib.h>
#include <type_traits>
#include "acg_internal.h"
#include "fir_plan.h"
#include "fir_tile_kernel.h"    // the tile kernels described above, and the parts they are made of ...
#include "fir_kernels.h"        // ... and the wave-private streaming kernels (both shared with fir_iq.hip)

// (the tap regrouping of the shared-stream kernel: fir_tile_kernel.h, FIR_KC)
__global__ void regroup_taps_kernel(const float* __restrict__ taps, float* __restrict__ gtaps,
                                    const int4* __restrict__ groups, const int* __restrict__ group_ch, int ntaps_pad)
{
    const int4 gi = groups[blockIdx.x];
    const int kc = gi.z;
    const int n = kc * ntaps_pad * 2;
    float* out = gtaps + (size_t)gi.y * ntaps_pad * 2;
    for (int idx = threadIdx.x; idx < n; idx += blockDim.x) {
        const int e = idx & 15;
        const int q = idx >> 4;
        const int c = q / kc;
        const int k = q - c * kc;
        out[idx] = taps[(size_t)group_ch[gi.y + k] * ntaps_pad * 2 + (c << 4) + e];
    }
}

#ifdef ACG_LAB   // round 1's first kernel (ACG_FIR_VARIANT=0): lab build only (libacarsdec_amd_lab.so)
#include "lab/fir_tile.inc"
#endif  // ACG_LAB

#ifdef ACG_LAB   // LDS-DMA variant (ACG_FIR_VARIANT=4): lab build only
#include "lab/fir_dma.inc"
#endif  // ACG_LAB

#ifdef ACG_LAB   // register-tap and matrix-pipe variants (ACG_FIR_VARIANT=7 / 8 / 6, 70..73): lab build only
#include "lab/fir_coltap_mfma.inc"
#endif  // ACG_LAB

// Launch-side state is per DEVICE (function attributes belong to the device's code object; the CU count is
// the device's): a process may hold contexts on several GPUs.  One table for every down-converter unit (fir_mm.hip too).
#define FIR_MAXDEV 64
struct FirDev {
    bool ready;
    int num_cu;
    std::map<const void*, size_t>* lds_optin;      // kernel -> dynamic LDS bytes it has been opted in for on this device
};
static FirDev g_firdev[FIR_MAXDEV];
static std::mutex g_firdev_mx;

// the current device's record; g_firdev_mx is held
static int fir_device(FirDev** out)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    if (dev < 0 || dev >= FIR_MAXDEV) return (int)hipErrorInvalidDevice;
    FirDev* d = &g_firdev[dev];
    if (!d->ready) {
        d->num_cu = 256;
        (void)hipDeviceGetAttribute(&d->num_cu, hipDeviceAttributeMultiprocessorCount, dev);
        d->lds_optin = new std::map<const void*, size_t>();
        d->ready = true;
    }
    *out = d;
    return 0;
}

extern "C" int acg_fir_device_cus(int* num_cu)
{
    std::lock_guard<std::mutex> lk(g_firdev_mx);
    FirDev* d = nullptr;
    if (int e = fir_device(&d)) return e;
    *num_cu = d->num_cu;
    return 0;
}

// Dynamic LDS above the default limit needs an opt-in per kernel (hipFuncAttributeMaxDynamicSharedMemorySize).  It is
// made HERE, at the launch site, with the bytes the launch is about to ask for and for exactly the instantiation being
// launched -- a table of instantiations kept elsewhere drifts from the launch switch (round 2's did: the write-through
// kernels that are the default were not in it).
extern "C" int acg_fir_lds_optin(const void* kernel, size_t bytes)
{
    std::lock_guard<std::mutex> lk(g_firdev_mx);
    FirDev* d = nullptr;
    if (int e = fir_device(&d)) return e;
    size_t& have = (*d->lds_optin)[kernel];
    if (bytes > have) {
        const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return (int)e;
        have = bytes;
    }
    return 0;
}

extern "C" int acg_launch_fir_fmt(const FirArgs* a, int fmt, void* stream)
{
    if (fmt == FMT_CF32) return acg_launch_fir_cf32(a, stream);            // the recordings' formats: fir_iq.hip
    int num_cu = 0;
    if (int e = acg_fir_device_cus(&num_cu)) return e;
    // the wave-private streaming kernel where it is instantiated for the window length and the launch is whole runs
    // (ACG_FIR_VARIANT=3 forces the workgroup-granular kernel below)
    if (env_int("ACG_FIR_VARIANT", 5) >= 5) {
        const int cprw = a->cpr_total;                              // 16-byte chunks per window (per plane for split int16)
#define FIRX_TRY(F_, C_, W_) \
        if (fmt == F_ && (F_ == FMT_SPLIT ? cprw / 2 : cprw) == C_ && acg_fir_fmt_wave_takes(a, W_)) \
            return launch_fmt_direct<F_, C_, W_>(a, num_cu, (hipStream_t)stream);
        FIRX_LIST(FIRX_TRY)
#undef FIRX_TRY
    }
    switch (fmt) {
    case FMT_CS16: return launch_fmt<FMT_CS16>(a, num_cu, (hipStream_t)stream);
    case FMT_SPLIT: return launch_fmt<FMT_SPLIT>(a, num_cu, (hipStream_t)stream);
    case FMT_F32R: return launch_fmt<FMT_F32R>(a, num_cu, (hipStream_t)stream);
    }
    return (int)hipErrorInvalidValue;
}

// Exact-order kernel: one thread per output, the M terms accumulated sequentially with separately rounded products,
// differences and sums and the 127.37 subtracted per sample -- rtl.c:335-353 operation for operation as an IEEE (-O2, no
// contraction) build of the reference executes it, so dm is BIT-IDENTICAL to such a build (and to oracle/orc_fir_u8).
// Two uses: the fallback for decimations whose window is not a whole number of 16-byte chunks (M % 8 != 0), and the
// verification mode (ACG_F_EXACT_FIR): the streaming kernels re-associate the sum (1e-7 relative), which can flip a
// razor-edge soft decision of the demodulator; with this kernel in front the whole GPU path is bit-identical end to end.
__global__ void fir_u8_generic_kernel(const FirArgs a)
{
    // no fused multiply-add anywhere in this kernel: HIP's __fmul_rn / __fadd_rn are plain operators and contract like any
    // other under the default -ffp-contract=fast (round 2's fallback kernel did: dm was 1e-8 off the oracle, inside the
    // tolerance nobody looked under).  tests/test_host_logic.py disassembles the kernel and checks.
#pragma clang fp contract(off)
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)a.nch * a.nwin;
    if (gid >= total) return;
    const int ch = (int)(gid / a.nwin);
    const int m = (int)(gid - (long long)ch * a.nwin);
    const uint8_t* p = a.iq + (size_t)a.stream_of[ch] * a.pitch + (size_t)m * a.row_bytes;
    const float* w = a.taps + (size_t)ch * a.ntaps_pad * 2;
    float Dr = 0.f, Di = 0.f;
    for (int k = 0; k < a.ntaps; ++k) {
        // plain operators on purpose: the pragma governs the operations written HERE, not the bodies of header inlines
        const float r = (float)p[2 * k] - 127.37f;                         // rtl.c:338
        const float g = (float)p[2 * k + 1] - 127.37f;                     // rtl.c:339
        const float wr = w[2 * k], wi = w[2 * k + 1];
        const float pr = r * wr - g * wi;                                  // rtl.c:351 vb[ind] * wf[ind]
        const float pi = r * wi + g * wr;
        Dr = Dr + pr;                                                      // D +=
        Di = Di + pi;
    }
    a.dm[(size_t)ch * a.dm_pitch + m] = cabs_like_glibc(Dr, Di);
}

extern "C" size_t acg_fir_lds_bytes(const FirArgs* a)
{
    return fir_persist_lds(*a);
}

// wave-private streaming kernel: whole tiles, runs inside one channel, a rate it is instantiated for
template <int CPR, int UU = 0, int BB = 0, bool FOLD = true, bool WT = false, bool NOMAC = false>
static int launch_direct(const FirArgs* a, int num_cu, hipStream_t stream)
{
    static_assert(4 * FirD<CPR>::WAVE_LDS <= FIR_CU_LDS, "a four-wave workgroup fits a CU: the plan's fit is >= 1");
    const FirWavePlan p = acg_fir_wave_plan(a, num_cu, FirD<CPR>::WAVE_LDS, ACG_TILE_WIN, 8);
    FirArgs b = *a;
#ifdef ACG_LAB
    if (acg_tune_get("ACG_FIR_DEBUG_DMPITCH0", 0)) b.dm_pitch = 0;          // measurement aid: every channel's dm lands in the first row (no write stream to HBM)
    if (acg_tune_has("ACG_FIR_DEBUG_SHAPE"))
        fprintf(stderr, "fir_u8_direct<%d>: nch %d nwin %d  wpg %d per_cu %d grid %lld  bodies/ch %lld pairs %d runs %lld  shares_cus %d prio %d\n",
                CPR, a->nch, a->nwin, p.wpg, p.per_cu, p.grid, p.bodies_per_ch, p.pairs, p.nrun, a->shares_cus, a->high_prio);
#endif
    return launch_planned(fir_u8_direct_kernel<CPR, UU, BB, FOLD, WT, NOMAC>, p, b, stream);
}

#ifdef ACG_LAB   // launchers of the lab variants
#include "lab/fir_lab_launch.inc"
#endif  // ACG_LAB

extern "C" int acg_launch_fir(const FirArgs* a, void* stream)
{
    const size_t lds = acg_fir_lds_bytes(a);
    int num_cu = 0;
    if (int e = acg_fir_device_cus(&num_cu)) return e;
    if (a->s8) return acg_launch_fir_s8(a, stream);          // ACG_FMT_CS8: the signed twins of the two product kernels (fir_iq.hip)
    // ACG_FIR_VARIANT.  The PRODUCT library has two kernels behind this entry point: 5 (default) the wave-private streaming
    // kernel where it applies (whole two-tile bodies, rtlMult 160 / 192 / 200; dm stored write-through), and 3, the
    // workgroup-granular kernel with the dynamic run dispenser, for everything else (ragged launches, other window lengths).
    // The LAB build (libacarsdec_amd_lab.so, -DACG_LAB; tests and probes only) adds: 0 one workgroup per segment; 1 / 2 static
    // persistent partition without / with non-temporal loads; 4 LDS-DMA double buffering; 6 matrix pipe; 7 taps in registers;
    // 8 = 7 with the results parked in LDS and written in chip-wide bursts; 50..56, 70..73 measurement knobs of 5 and 7
    // (55: write-back stores; 56: no arithmetic, dm is garbage).
    int variant = env_int("ACG_FIR_VARIANT", 5);
#ifndef ACG_LAB
    if (variant != 3) variant = 5;
#else
    if ((variant == 7 || variant == 8 || (variant >= 70 && variant <= 73)) && a->cpr == 25 && acg_fir_u8_wave_takes(a))
    {            // 70..73: measurement knobs (staging slots, burst length)
        if (variant == 8) return launch_coltap<true, 13, 1, true>(a, num_cu, (hipStream_t)stream);      // results parked in LDS, chip-wide bursts
        if (variant == 70) return launch_coltap<true, 26, 1>(a, num_cu, (hipStream_t)stream);
        if (variant == 71) return launch_coltap<true, 26, 2>(a, num_cu, (hipStream_t)stream);
        if (variant == 72) return launch_coltap<true, 26, 13>(a, num_cu, (hipStream_t)stream);
        if (variant == 73) return launch_coltap<true, 4, 2>(a, num_cu, (hipStream_t)stream);
        return launch_coltap<>(a, num_cu, (hipStream_t)stream);
    }
    if (variant == 6 && a->cpr == 25 && acg_fir_u8_wave_takes(a))
        return launch_mfma<25>(a, num_cu, (hipStream_t)stream);
#endif
    if ((variant == 5 || (variant >= 50 && variant <= 56)) && acg_fir_u8_wave_takes(a)) {
#ifdef ACG_LAB    // 50..54: measurement knobs (staging slots, burst length, 127.37 per sample)
        if (a->cpr == 25) {
            if (variant == 50) return launch_direct<25, 10, 1>(a, num_cu, (hipStream_t)stream);
            if (variant == 51) return launch_direct<25, 25, 5>(a, num_cu, (hipStream_t)stream);
            if (variant == 52) return launch_direct<25, 25, 10>(a, num_cu, (hipStream_t)stream);
            if (variant == 53) return launch_direct<25, 10, 10>(a, num_cu, (hipStream_t)stream);
            if (variant == 54) return launch_direct<25, 0, 0, false>(a, num_cu, (hipStream_t)stream);      // 127.37 subtracted per sample
            if (variant == 56) return launch_direct<25, 0, 0, true, true, true>(a, num_cu, (hipStream_t)stream);   // measurement: no arithmetic (dm is garbage)
            if (variant == 55) return launch_direct<25>(a, num_cu, (hipStream_t)stream);                    // dm stored write-back (round 2a)
        }
#endif
        // (dm is stored write-through: beside the streaming reads a write-back line costs more)
#define FIRD_TRY(C_) if (a->cpr == C_) return launch_direct<C_, 0, 0, true, true>(a, num_cu, (hipStream_t)stream);
        FIRD_LIST(FIRD_TRY)
#undef FIRD_TRY
    }
#ifdef ACG_LAB
    if (variant == 0) {
        const unsigned int grid = (unsigned int)a->nch * (unsigned int)a->nseg;
        FIR_LAUNCH(fir_u8_tile_kernel, dim3(grid), dim3(ACG_WG_FIR), lds, (hipStream_t)stream, *a,
                           a->iq, a->taps, a->stream_of, a->dm);
        return (int)hipGetLastError();
    }
    if (variant == 4 && (a->cpr & 1) && a->row_stride == a->row_bytes) {
        const size_t tile = (size_t)ACG_TILE_WIN * a->row_bytes;
        const size_t lds2 = 2 * tile + 2 * 4 * 64 * sizeof(float4) + 16;
        if (lds2 <= 96 * 1024) {
            const long long grid4 = acg_fir_tile_grid(num_cu, lds2, 4, 0, true, acg_fir_tile_units(a->nch, a->nwin, ACG_TILE_WIN), FIR_RUN);
            FIR_LAUNCH(fir_u8_dma_kernel, dim3((unsigned int)grid4), dim3(ACG_WG_FIR), lds2, (hipStream_t)stream,
                               *a, a->iq, a->taps, a->stream_of, a->dm);
            return (int)hipGetLastError();
        }
    }
#endif
    FirArgs b = *a;
#ifdef ACG_LAB
    // variants 1 and 2, the static partition: resident workgroups, LDS-limited (160 KiB per CU), at most 5 (VGPR budget of 4-wave
    // workgroups), one per (channel, tile) at most
    const long long grid = acg_fir_tile_grid(a->ncu > 0 ? a->ncu : num_cu, lds, 5, a->wg_per_cu, true, acg_fir_tile_units(a->nch, a->nwin, ACG_TILE_WIN));
    const bool nocompute = acg_tune_has("ACG_FIR_DEBUG_NOCOMPUTE") != 0;   // measurement aid: loads + LDS staging only
    if (nocompute) b.ntaps_pad = 0;
    if (variant == 1) {
        FIR_LAUNCH((fir_u8_persist_kernel<false, false, false>), dim3((unsigned int)grid), dim3(ACG_WG_FIR), lds,
                           (hipStream_t)stream, b, a->iq, a->taps, a->stream_of, a->dm);
        return (int)hipGetLastError();
    }
    if (variant == 2) {
        FIR_LAUNCH((fir_u8_persist_kernel<true, false, false>), dim3((unsigned int)grid), dim3(ACG_WG_FIR), lds,
                           (hipStream_t)stream, b, a->iq, a->taps, a->stream_of, a->dm);
        return (int)hipGetLastError();
    }
#endif
    return launch_persist<false>(b, a, num_cu, (hipStream_t)stream);
}

extern "C" int acg_launch_fir_shared(const FirArgs* a, void* stream)
{
    const size_t lds = fir_shared_lds(*a);
    int num_cu = 0;
    if (int e = acg_fir_device_cus(&num_cu)) return e;
    if (lds > 64 * 1024) return (int)hipErrorInvalidValue;
    const long long G = acg_fir_tile_units(a->ngroups, a->nwin, ACG_TILE_WIN);
    if (G >= (1ll << 31)) return (int)hipErrorInvalidValue;
    // four workgroups per CU at most (the K-channel register block)
    const long long grid = acg_fir_tile_grid(a->ncu > 0 ? a->ncu : num_cu, lds, 4, 0, true, G, FIR_RUN);
    if (a->s8) return acg_launch_fir_shared_s8(a, grid, lds, stream);      // (fir_iq.hip)
    return launch_whole_or_ragged(fir_u8_shared_kernel<true>, fir_u8_shared_kernel<false>, a->nwin, grid, lds, (hipStream_t)stream, *a, a->iq, a->gtaps,
                                  a->groups, a->group_ch, a->dm);
}

extern "C" int acg_launch_regroup_taps(const FirArgs* a, void* stream)
{
    FIR_LAUNCH(regroup_taps_kernel, dim3((unsigned int)a->ngroups), dim3(256), 0, (hipStream_t)stream, a->taps,
                       (float*)a->gtaps, a->groups, a->group_ch, a->ntaps_pad);
    return (int)hipGetLastError();
}

extern "C" int acg_launch_fir_generic(const FirArgs* a, void* stream)
{
    const long long total = (long long)a->nch * a->nwin;
    const unsigned int grid = (unsigned int)((total + 255) / 256);
    FIR_LAUNCH(fir_u8_generic_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

// Which kernel family acg_launch_fir_fmt (fmt 1, 2, 3, 5) or acg_launch_fir (fmt 4: a->s8) takes for the launch a, as those
// launchers decide it (the same table and the same plan), and the streaming kernel's tile geometry.  Launches nothing.
extern "C" int acg_fir_choice(const FirArgs* a, int fmt, FirChoice* out)
{
    int num_cu = 0;
    if (int e = acg_fir_device_cus(&num_cu)) return e;
    *out = FirChoice{};
    out->family = ACG_FIR_FAM_WORKGROUP;
    const int variant = env_int("ACG_FIR_VARIANT", 5);
    FirWavePlan p{};
    int W = 0;
    if (fmt == FMT_CS8) {
        if (variant != 3 && acg_fir_u8_wave_takes(a)) {
#define FIRD_PLAN(C_) \
            if (a->cpr == C_) { \
                W = ACG_TILE_WIN; \
                p = acg_fir_wave_plan(a, num_cu, FirD<C_>::WAVE_LDS, W, 8); \
            }
            FIRD_LIST(FIRD_PLAN)
#undef FIRD_PLAN
        }
    } else if (variant >= 5) {
        const int cprw = a->cpr_total;
#define FIRX_PLAN(F_, C_, W_) \
        if (!W && fmt == F_ && (F_ == FMT_SPLIT ? cprw / 2 : cprw) == C_ && acg_fir_fmt_wave_takes(a, W_)) { \
            W = W_; \
            p = acg_fir_wave_plan(a, num_cu, FirX<F_, C_, W_>::WAVE_LDS, W_, 8); \
        }
        FIRX_LIST(FIRX_PLAN)
        FIRX_LIST_IQ(FIRX_PLAN)
#undef FIRX_PLAN
    }
    if (W) {
        out->family = ACG_FIR_FAM_STREAMING;
        out->tile_win = W;
        out->runs = p.nrun;
        out->waves = p.grid * p.wpg;
        out->wpg = p.wpg;
        out->pairs = p.pairs;
    }
    return 0;
}
