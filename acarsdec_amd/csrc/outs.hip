// outs.hip -- the one launch sequence of the batch sinks: the kept records of ONE take rendered into up to ACG_OUTS_LEGS legs,
// record i of every leg the same message (acg_drain_outputs / acg_collect_outputs).  The JSON sink and the text sink
// (acg_drain_json / acg_drain_text and their collects) are this sequence with one rendered leg, launch for launch what a
// sequence of their own would be.
//   outs_keys_kernel      the (chn, end_bit) keys of the take (sink_pack.h pk_keys), once for all legs;
//   flight_sort_kernel    flight.hip's one-workgroup radix sort (acg_launch_sort_pairs), once: the serial part of a sink pass;
//   <unit>_measure_kernel json.hip's / text.hip's own kernel per rendered leg (acg_launch_json_sorted / _text_sorted): unchanged;
//   outs_sum_kernel       pk_sum, grid y = leg: per 256 ranks the bytes and records of every leg in one launch;
//   outs_offsets_kernel   pk_offsets, grid y = leg: every leg's offset table and counters in one launch;
//   <unit>_render_kernel  json.hip's / text.hip's own kernel per rendered leg: unchanged;
//   outs_gather_kernel    the MSGS leg: a wave per rank copies the record idx_s[r] and its acg_oooi to rank r of packed arrays.
// Every kernel runs on the stream of the label pass it hangs on, one behind the other; no kernel reads what another workgroup of
// the same launch wrote.
#include "sink_pack.h"

static_assert(ACG_OUTS_LEGS == ACG_OUT_LEGS_MAX, "leg count");

// what the scan reads and writes of a leg
struct OutsScanLeg {
    const unsigned int* len;
    unsigned int* off;
    unsigned int *wg_sum, *wg_cnt;
    unsigned int* counters;
};
struct OutsScan {
    const unsigned int* total;
    unsigned int nmax;
    OutsScanLeg leg[ACG_OUTS_LEGS];     // grid y indexes it: a uniform load from the kernel's arguments
};

struct OutsGather {
    const AcgMsgRec* recs;
    const unsigned char* oooi;
    const unsigned int* total;
    unsigned int nmax;
    const unsigned long long* key_s;
    const unsigned int* idx_s;
    AcgMsgRec* g_recs;
    unsigned char* g_oooi;
    unsigned int* g_count;
};

#define OUTS_GATHER_WAVES 4

__global__ __launch_bounds__(PK_WG) void outs_keys_kernel(AcgSinkPass p) { pk_keys(p); }

__global__ __launch_bounds__(PK_WG) void outs_sum_kernel(OutsScan s)
{
    __shared__ unsigned int sum_s;
    const OutsScanLeg& l = s.leg[blockIdx.y];
    pk_sum(&sum_s, l.len, l.wg_sum, l.wg_cnt, s.nmax, s.total);
}

__global__ __launch_bounds__(PK_WG) void outs_offsets_kernel(OutsScan s)
{
    __shared__ unsigned int base_s, cnt_s;
    __shared__ unsigned int wave_n[PK_WG / 64];
    const OutsScanLeg& l = s.leg[blockIdx.y];
    pk_offsets(&base_s, &cnt_s, wave_n, l.len, l.off, l.wg_sum, l.wg_cnt, l.counters, s.nmax, s.total);
}

// pk_load's access pattern, global to global: 80 + 10 dwords per record.  Kept records sort in front of dropped ones (pk_key), so
// the rank behind the last kept one is their count; rank 0 says 0 when there is none.
__global__ __launch_bounds__(64 * OUTS_GATHER_WAVES) void outs_gather_kernel(OutsGather g)
{
    const int lane = threadIdx.x & 63;
    const unsigned int r = blockIdx.x * OUTS_GATHER_WAVES + (threadIdx.x >> 6);  // wave-uniform
    const unsigned int n = *g.total < g.nmax ? *g.total : g.nmax;
    if (r >= n || g.key_s[r] == ~0ull) {
        if (r == 0 && lane == 0) *g.g_count = 0;
        return;
    }
    // the count first: whatever happens to this rank's copy, the host never reads the previous take's.  (A kept record on channel
    // number 2^20 - 1 with end_bit 2^44 - 1 has the key ~0 of a dropped one: the corner json.hip and text.hip have too, pk_key.)
    if (lane == 0 && (r + 1 == n || g.key_s[r + 1] == ~0ull)) *g.g_count = r + 1;
    const unsigned int idx = g.idx_s[r];
    if (idx >= g.nmax) return;                                                   // (cannot happen: the sort permutes [0, n))
    const unsigned int* src = (const unsigned int*)(g.recs + idx);
    unsigned int* dst = (unsigned int*)(g.g_recs + r);
    dst[lane] = src[lane];
    if (lane < 16) dst[64 + lane] = src[64 + lane];
    if (lane < 10) ((unsigned int*)(g.g_oooi + (size_t)r * sizeof(acg_oooi)))[lane] = ((const unsigned int*)(g.oooi + (size_t)idx * sizeof(acg_oooi)))[lane];
}

extern "C" int acg_launch_outs(const AcgOutsPass* o, void* stream)
{
    const unsigned int nmax = o->order.nmax;
    if (nmax == 0) return 0;
    if (o->nrender > ACG_OUTS_LEGS) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const unsigned int g = (nmax + PK_WG - 1) / PK_WG;
    hipLaunchKernelGGL(outs_keys_kernel, dim3(g), dim3(PK_WG), 0, s, o->order);
    int e = acg_launch_sort_pairs(o->order.key, o->order.idx, o->order.key_s, o->order.idx_s, o->order.total, 0u, stream);
    if (e) return e;
    for (unsigned int l = 0; l < o->nrender; ++l) {
        e = o->is_json[l] ? acg_launch_json_sorted(&o->leg[l], ACG_SORTED_MEASURE, stream) : acg_launch_text_sorted(&o->leg[l], ACG_SORTED_MEASURE, stream);
        if (e) return e;
    }
    if (o->nrender) {
        OutsScan sc;
        sc.total = o->order.total;
        sc.nmax = nmax;
        for (unsigned int l = 0; l < ACG_OUTS_LEGS; ++l) {
            const AcgSinkPass& p = o->leg[l < o->nrender ? l : 0];
            sc.leg[l] = OutsScanLeg{p.len, p.off, p.wg_sum, p.wg_cnt, p.counters};
        }
        hipLaunchKernelGGL(outs_sum_kernel, dim3(g, o->nrender), dim3(PK_WG), 0, s, sc);
        hipLaunchKernelGGL(outs_offsets_kernel, dim3(g, o->nrender), dim3(PK_WG), 0, s, sc);
    }
    for (unsigned int l = 0; l < o->nrender; ++l) {
        e = o->is_json[l] ? acg_launch_json_sorted(&o->leg[l], ACG_SORTED_RENDER, stream) : acg_launch_text_sorted(&o->leg[l], ACG_SORTED_RENDER, stream);
        if (e) return e;
    }
    if (o->g_recs) {
        const OutsGather ga{o->order.recs, o->order.oooi, o->order.total, nmax, o->order.key_s, o->order.idx_s, o->g_recs, o->g_oooi, o->g_count};
        hipLaunchKernelGGL(outs_gather_kernel, dim3((nmax + OUTS_GATHER_WAVES - 1) / OUTS_GATHER_WAVES), dim3(64 * OUTS_GATHER_WAVES), 0, s, ga);
    }
    return (int)hipGetLastError();
}
