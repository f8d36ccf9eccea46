// stats.hip -- per-channel reception statistics (acg_chan_stats, include/acarsdec_amd.h): the events the reference reports under
// -v (blk_thread, acars.c:120-209) and the drops of outputmsg()'s filters (output.c:537-540,650), counted per channel over the
// blocks an entry point consumes.  ONE launch, a thread per block, on the stream and behind the passes the entry point already
// runs: it reads the head of each AcgFrameRec -- chn, len, the outcome byte blk_repair_kernel left in pad[0], the level's two
// operands, end_sample; never the text -- and, when a filter is set, asks label.hip's own predicates (msg_keep.h) about the
// split's record of the same block.
//
// Every accumulator is an integer add or an integer maximum with device scope: a snapshot does not depend on the order the waves
// ran in.  The level is kept as the bit pattern of the non-negative double MskLvlSum / MskBitCount (IEEE division, as the host
// would do it), which orders like the double; the minimum as the maximum of the complement (AcgChanStats, acg_internal.h).
#include <hip/hip_runtime.h>
#include "acg_internal.h"
#include "acarsdec_amd.h"
#include "msg_keep.h"

#define STATS_WG 256

static_assert(sizeof(AcgChanStats) == sizeof(acg_chan_stats) && offsetof(AcgChanStats, lvl_min_inv) == offsetof(acg_chan_stats, lvl_min) &&
                  offsetof(AcgChanStats, end_sample_p1) == offsetof(acg_chan_stats, last_end_sample) &&
                  offsetof(AcgChanStats, delivered) == offsetof(acg_chan_stats, delivered),
              "device and public statistics record must have one layout");

__device__ __forceinline__ void bump(unsigned int* p, unsigned int v = 1u)
{
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(STATS_WG) void chan_stats_kernel(AcgStatsPass p, AcgLabelFilter f)
{
    const unsigned int i = blockIdx.x * STATS_WG + threadIdx.x;
    if (i >= p.n) return;
    const AcgFrameRec* r = p.frames + ((p.first + i) & (p.cap - 1));       // (cap is a power of two)
    const int chn = r->chn;
    if ((unsigned int)chn >= (unsigned int)p.nch) return;
    AcgChanStats* s = p.stats + chn;
    const unsigned int why = r->pad[0], reason = why & ACG_BLK_REASON;
    bump(&s->blocks);                                                       // acars.c:121
    if (why & ACG_BLK_F_DEL) bump(&s->miss_txt_end);                        // acars.c:326
    if (reason == ACG_BLK_SHORT) { bump(&s->too_short); return; }           // :126
    if (reason == ACG_BLK_PARITY_MANY) { bump(&s->parity_many); return; }   // :148
    if (why & ACG_BLK_F_PARITY) {                                           // :154
        bump(&s->parity_blocks);
        bump(&s->parity_errs, why >> ACG_BLK_PN_SHIFT);
    }
    if (why & ACG_BLK_F_CRC) bump(&s->crc_errors);                          // :167
    if (reason == ACG_BLK_UNFIXABLE) { bump(&s->unfixable); return; }       // :173, :185
    if (reason != ACG_BLK_PARITY_PROBLEM && reason != ACG_BLK_KEPT) return; // (a block the repair pass has not seen: only `blocks`)
    if (why & (ACG_BLK_F_PARITY | ACG_BLK_F_CRC)) bump(&s->fixed);          // :178, :190
    if (reason == ACG_BLK_PARITY_PROBLEM) { bump(&s->parity_problem); return; }   // :203
    bump(&s->kept);                                                         // :209
    const int bitcount = r->bitcount;
    if (bitcount > 0) {
        const double ratio = r->lvlsum / (double)bitcount;
        if (ratio >= 0) {                                                   // (not for a NaN: its bits order like nothing)
            const unsigned long long b = (unsigned long long)__double_as_longlong(ratio + 0.0);   // (-0 + 0 = +0)
            __hip_atomic_fetch_max(&s->lvl_min_inv, ~b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(&s->lvl_max_bits, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __hip_atomic_fetch_max(&s->end_sample_p1, r->end_sample + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // outputmsg()'s filters in the reference's order: a block is charged to the FIRST one that drops it
    if (p.filter_on) {
        const AcgMsgRec* m = p.msgs + i;
        if (!msg_keep_a(m, f)) { bump(&s->uplink_dropped); return; }        // output.c:537
        if (!msg_keep_b(m, f)) { bump(&s->label_dropped); return; }         // output.c:539
        if (!msg_keep_e(m, f)) { bump(&s->empty_dropped); return; }         // output.c:650
    }
    bump(&s->delivered);
}

extern "C" int acg_launch_chan_stats(const AcgStatsPass* p, void* stream)
{
    if (p->n == 0) return 0;
    hipLaunchKernelGGL(chan_stats_kernel, dim3((p->n + STATS_WG - 1) / STATS_WG), dim3(STATS_WG), 0, (hipStream_t)stream, *p, *p->f);
    return (int)hipGetLastError();
}
