// msg_keep.h -- the CLI's message filters (-A, -b, -e: output.c:537-540,650) as predicates over a split record, one copy for
// label.hip (the filter / compaction pass, the flight table's event extraction) and stats.hip (which filter dropped a block).
#pragma once
#include <hip/hip_runtime.h>
#include "acg_internal.h"
#include "acarsdec_amd.h"

// a record's text as the decoder sees it: bytes at or past txt_len (clamped to the row) are 0
struct Txt {
    const unsigned char* p;
    int n;
    __device__ unsigned char operator()(int i) const { return (unsigned)i < (unsigned)n ? p[i] : (unsigned char)0; }
};

__device__ __forceinline__ Txt rec_txt(const AcgMsgRec* r)
{
    int n = r->txt_len;
    n = n < 0 ? 0 : n > ACG_MSG_TXT ? ACG_MSG_TXT : n;
    return Txt{(const unsigned char*)r->txt, n};
}

// -A (output.c:537)
__device__ __forceinline__ bool msg_keep_a(const AcgMsgRec* r, const AcgLabelFilter& f)
{
    return !((f.flags & ACG_MSGF_DOWNLINK_ONLY) && !r->down);
}

// -b (output.c:539)
__device__ __forceinline__ bool msg_keep_b(const AcgMsgRec* r, const AcgLabelFilter& f)
{
    if (f.nlabels > 0) {
        // the label as a C string (label[2] is the split's terminator), packed like the normalised tokens
        const unsigned int l0 = (unsigned char)r->label[0], l1 = l0 ? (unsigned char)r->label[1] : 0u;
        const unsigned int key = l0 | (l1 << 8);
        bool hit = false;
        for (int i = 0; i < f.nlabels; ++i) hit |= (l0 != 0) & (f.tok[i] == key);
        if (!hit) return false;
    }
    return true;
}

// output.c:537-540, 650 (and outputmsg()'s callers: blocks the repair dropped never get there)
// -A and -b: what decides whether a block reaches addFlight() (output.c:537-540)
__device__ __forceinline__ bool msg_keep_ab(const AcgMsgRec* r, const AcgLabelFilter& f)
{
    if (!r->valid) return false;
    return msg_keep_a(r, f) && msg_keep_b(r, f);
}

// -e (output.c:650)
__device__ __forceinline__ bool msg_keep_e(const AcgMsgRec* r, const AcgLabelFilter& f)
{
    return !((f.flags & ACG_MSGF_SKIP_EMPTY) && rec_txt(r)(0) == 0);
}

// output.c:537-540, 650 (and outputmsg()'s callers: blocks the repair dropped never get there)
__device__ __forceinline__ bool msg_keep(const AcgMsgRec* r, const AcgLabelFilter& f)
{
    return msg_keep_ab(r, f) && msg_keep_e(r, f);
}
