// fir_common.h -- what both families of down-converter kernels reach: the tile kernels (fir_tile_kernel.h, fir_grid_kernel.h) and the
// wave-private streaming kernels (fir_kernels.h).  The packed pair, the dynamic LDS, |D| as the reference's libm takes it, the sample
// formats' numbers, the ticket pair of the run dispensers, and the launch macro with the switch table.  Not a unit of its own.
#ifndef ACG_FIR_COMMON_H
#define ACG_FIR_COMMON_H
#include <hip/hip_runtime.h>
#include "acg_internal.h"

typedef float f2 __attribute__((ext_vector_type(2)));

extern __shared__ __attribute__((aligned(16))) unsigned char fir_smem[];

// The sample formats; a row (one window) is 2 bytes per sample for u8 and FMT_CS8, 4 for the others, 8 for FMT_CF32
//   FMT_CS16   interleaved int16 I,Q        soapy.c:238-241   (x/32768 folded into the output scale)
//   FMT_SPLIT  int16 I plane + int16 Q plane sdrplay.c:219-223 (cabsf(D)/4 = output scale)
//   FMT_F32R   real float32 samples          air.c:314-324     (complex tap x real sample)
//   FMT_CS8    interleaved int8 I,Q          SigMF ci8, HackRF: runs on the u8 kernels' signed twins, its window is the u8 window
//   FMT_CF32   interleaved float32 I,Q       soapy.c:232-254's loop on floats (SigMF cf32_le, SoapySDR CF32; scale 1)
#define FMT_CS16 1
#define FMT_SPLIT 2
#define FMT_F32R 3
#define FMT_CS8 4
#define FMT_CF32 5

__device__ __forceinline__ float cabs_like_glibc(float re, float im)
{
    // glibc 2.35 cabsf/hypotf == (float)sqrt((double)x*x + (double)y*y) (checked on 2e8 inputs);
    // products are exact in double, one rounding in the sum, correctly rounded sqrt, one narrowing.
    double d = (double)re * (double)re + (double)im * (double)im;
    return (float)__dsqrt_rn(d);
}

// A run dispenser's ticket is an atomic whose result is needed a whole tile later.  Written as a compiler builtin it is waited
// for on the spot (it sits in divergent control flow, and the uniform-address atomic optimiser wants its result at once), which
// stalls the requesting wave -- and at the next barrier the whole workgroup -- for a full device-scope round trip per run.  As
// inline asm the compiler does not know about it; ticket_take is the matching wait.  Returns are in issue order, so once at most
// YOUNGER vector-memory operations are outstanding the (older) atomic has returned: the wait is for exactly that and costs
// nothing when the later loads have long been consumed (0: called where no newer load is wanted in flight).  The result is the
// requesting lane's; a caller that wants it uniform takes readfirstlane of it.
// tests/test_host_logic.py disassembles the kernels and checks that nothing touches the ticket register between the two statements.
__device__ __forceinline__ void ticket_request(unsigned int* counter, unsigned int& ticket)
{
    const unsigned int one = 1u;
    asm volatile("global_atomic_add %0, %1, %2, off sc0" : "=v"(ticket) : "v"(counter), "v"(one) : "memory");
}
template <int YOUNGER>
__device__ __forceinline__ unsigned int ticket_take(unsigned int& ticket)
{
    asm volatile("s_waitcnt vmcnt(%1)" : "+v"(ticket) : "i"(YOUNGER) : "memory");
    return ticket;
}

// ---- launch helpers ----------------------------------------------------------------------------------------------------
#define FIR_LAUNCH(K_, grid_, blk_, lds_, stream_, ...)                                            \
    do {                                                                                           \
        if (int oe_ = acg_fir_lds_optin((const void*)(K_), (size_t)(lds_))) return oe_;            \
        hipLaunchKernelGGL((K_), grid_, blk_, lds_, stream_, __VA_ARGS__);                         \
    } while (0)

// measurement / layout switches: one table, filled from the environment once per process (acg_api.cpp)
extern "C" int acg_tune_get(const char* name, int dflt);
extern "C" int acg_tune_has(const char* name);
static inline int env_int(const char* name, int dflt) { return acg_tune_get(name, dflt); }

#endif /* ACG_FIR_COMMON_H */
