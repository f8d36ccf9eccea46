// msk_lean_wide.hip -- msk_lean_kernel (msk_lean_kernel.h; described at the head of msk_lean.hip) with 16 lanes per channel,
// for the few-channel contexts whose demodulator leaves SIMDs of its CU partition idle (round 12).
//
// A segment is cut wave-wide: one channel that stands in SYN2 behind a false sync takes every channel of its wave out of the
// segment, and a cut costs ~1.7 periods' worth of time that overlaps with nothing (LEDGER round 11).  Fewer channels per wave means
// fewer cuts per wave: 8 / 4 channels per wave get 6.91 / 7.43 periods per segment on the bench's traffic
// (profiles/r12_segment_stats.txt).  A period's instruction stream does not depend on the group width: above 6 lanes every lane
// mixes at most one sample (SPL 1), and lanes 6 ... LPC - 1 mix into the ring's spare row as lanes 6 and 7 of an 8-lane group do.
// Lane g < 8 keeps bit record g of the segment, and every lane moves one float4 of the dm window per refill.  (32 lanes per channel
// were built too and are not in the tree: nothing over 16 in the pipeline; LEDGER round 12.)  Same operations on the same operands in the same order per channel: state,
// blocks, text and bit records equal the 8-lane kernel's bit for bit (tests/test_gpu_lean_wide.py), and the periods hold the
// bounds pinned for msk_lean.hip (tests/test_lean_wide_asm.py).
//
// Four-wave workgroups only (the shape of a context with a CU partition): acg_launch_msk (msk.hip) sends every other launch to
// the 8-lane kernel, which is exact from launch to launch because the channel state does not depend on the width.
#include <hip/hip_runtime.h>
#include "acg_internal.h"

#include "msk_common.h"

#include "msk_lean_kernel.h"

extern "C" int acg_launch_msk_lean_wide(const MskArgs* a, int lpc, int wpg, unsigned int grid, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const dim3 blk(64 * wpg);
#define LEAN_LAUNCH(L_, W_) do { if (a->bits) hipLaunchKernelGGL((msk_lean_kernel<L_, W_, true>), dim3(grid), blk, 0, s, *a); \
                                 else hipLaunchKernelGGL((msk_lean_kernel<L_, W_, false>), dim3(grid), blk, 0, s, *a); } while (0)
    switch (lpc * 16 + wpg) {
    case 16 * 16 + 4: LEAN_LAUNCH(16, 4); break;
    default: return (int)hipErrorInvalidValue;
    }
#undef LEAN_LAUNCH
    return (int)hipGetLastError();
}
