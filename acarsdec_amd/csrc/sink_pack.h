// sink_pack.h -- what the device renderers of the batch sink (json.hip, text.hip) have in common: a record and its acg_oooi into a
// wave's LDS, the (chn, end_bit) sort key, the level's float and its guard, the two-launch exclusive scan of the record lengths
// in sorted order, the seam-safe flush of a wave's LDS row to its packed place in the output, and the skeleton of the passes.
// Every device function is inlined into the kernels of the unit that includes it, so each unit keeps kernels of its own: json.hip
// and text.hip a measure and a render kernel each; outs.hip the keys kernel and the scan's two, which it launches around them
// (acg_launch_outs, the one launch sequence of the sinks and the outputs); flight_text.hip scan kernels over its own pass.
//
// THE SEAM.  Records are packed without padding, so two neighbours share a 16-byte chunk where they meet, and another wave writes
// the neighbour.  No chunk is ever read back and merged: the row holds the record at the same offset mod 16 as its place in the
// output, the first bytes up to the next 16-byte boundary and the last bytes behind the last one leave as BYTE stores, and only
// chunks that lie wholly inside the record leave as 16-byte stores (LDS 16-byte reads, both sides aligned).
//
// THE SKELETON.  The bodies of the keys, measure and render kernels are here too (pk_keys, pk_measure<F>, pk_render<F>), written
// once over a format F that supplies
//   F::REC_MAX                                   the longest record, a multiple of 64;
//   F::record<W>(R, row, pass, lane, &near_mid)  the record's length; with W, its bytes at row (json_line, text_record);
//   F::row_at(rows, wv, off)                     rows[wv] + off % 16: where wave wv's record starts in its row.  The same two
//                                                operations in every unit; the order they are written in decides the order of two
//                                                independent instructions of the render kernel, and each unit keeps its own.
// A unit keeps its two __global__ kernels as thin wrappers (and with them its own names and __shared__ footprint; the measure
// kernel also its two early-outs, see pk_measure) and its extern "C" launcher (pk_launch_sorted).
#pragma once
#include <hip/hip_runtime.h>
#include "acg_internal.h"
#include "acarsdec_amd.h"

#define PK_WG 256                           // threads of the keys / sum / offsets kernels
#define PK_REC 384                          // the record (320 B) and its acg_oooi (40 B)
#define PK_WAVES 2                          // independent waves (one record each) of a measure / render workgroup

static_assert(sizeof(AcgMsgRec) == 320 && sizeof(acg_oooi) == 40 && sizeof(AcgMsgRec) + sizeof(acg_oooi) <= PK_REC, "record layout");

// a literal of at most 16 characters as two immediates: lane j takes byte j, nothing is loaded
struct PkLit {
    unsigned long long lo, hi;
    unsigned int n;
};

constexpr PkLit pk_lit(const char* s)
{
    PkLit l{0, 0, 0};
    for (; s[l.n]; ++l.n) {
        if (l.n < 8) l.lo |= (unsigned long long)(unsigned char)s[l.n] << (8 * l.n);
        else l.hi |= (unsigned long long)(unsigned char)s[l.n] << (8 * (l.n - 8));
    }
    return l;
}

// the record at recs[idx] and its acg_oooi into the wave's LDS: 80 + 10 dwords
__device__ __forceinline__ void pk_load(unsigned char* R, const AcgMsgRec* recs, const unsigned char* oooi, unsigned int idx, int lane)
{
    const unsigned int* src = (const unsigned int*)(recs + idx);
    unsigned int* dst = (unsigned int*)R;
    dst[lane] = src[lane];
    if (lane < 16) dst[64 + lane] = src[64 + lane];
    if (lane < 10) dst[80 + lane] = ((const unsigned int*)(oooi + (size_t)idx * sizeof(acg_oooi)))[lane];
    // (LDS operations of one wave execute in order; the fence keeps the compiler from moving them across each other)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the number handed out for the record's channel (acg_set_channel_numbers; no map: the slot).  It goes into the sort key and the
// channel tokens; whatever is a table per slot (the frequency token) keeps the slot.  A wave-uniform load, kept in a register.
__device__ __forceinline__ int pk_chn(const AcgSinkPass& p, int slot)
{
    return p.nmap && (unsigned int)slot < p.nmap ? p.chmap[slot] : slot;
}

// records the block repair dropped (none passes label.hip's filter) would sort last and render nothing
__device__ __forceinline__ unsigned long long pk_key(const AcgMsgRec* r, const AcgSinkPass& p)
{
    return r->valid ? (((unsigned long long)(unsigned int)pk_chn(p, r->chn) & 0xfffffull) << 44) | ((unsigned long long)r->end_bit & ((1ull << 44) - 1ull)) : ~0ull;
}

// the float of acars.c:351 (or the record's own, lab entries).  *near_mid: the one inexact step -- another log10 may land on the
// other side of a float rounding boundary when the double lies next to one.  A float midpoint is a double whose low 29 mantissa
// bits are 1 << 28 (normal floats).
__device__ __forceinline__ float pk_level(const AcgMsgRec* r, int lvl_from_rec, bool* near_mid)
{
    float lvl = r->lvl;
    *near_mid = false;
    if (!lvl_from_rec) {
        const double d = 10.0 * log10(r->lvlsum / (double)r->bitcount);
        lvl = (float)d;
        const long long low = (long long)((unsigned long long)__double_as_longlong(d) & ((1ull << 29) - 1ull)) - (1ll << 28);
        *near_mid = d == d && d - d == 0.0 && (low < 0 ? -low : low) <= 8;
    }
    return lvl;
}

// ---- the exclusive scan of len[] in sorted order (label.hip's two-launch count / base scheme) --------------------------------
// first launch: per PK_WG ranks, the bytes and the records that have any.  sum_s: one shared word of the workgroup.
__device__ __forceinline__ void pk_sum(unsigned int* sum_s, const unsigned int* len, unsigned int* wg_sum, unsigned int* wg_cnt, unsigned int nmax,
                                       const unsigned int* total)
{
    if (threadIdx.x == 0) *sum_s = 0;
    __syncthreads();
    const unsigned int i = blockIdx.x * PK_WG + threadIdx.x;
    const unsigned int v = (i < nmax && i < *total) ? len[i] : 0u;
    if (v) atomicAdd(sum_s, v);
    const int c = __syncthreads_count(v != 0);
    if (threadIdx.x == 0) {
        wg_sum[blockIdx.x] = *sum_s;
        wg_cnt[blockIdx.x] = (unsigned int)c;
    }
}

// second launch: every rank's byte offset; counters[0] = the pass's bytes, counters[1] = its records.  base_s, cnt_s: a shared word
// each; wave_n: PK_WG / 64 shared words.
__device__ __forceinline__ void pk_offsets(unsigned int* base_s, unsigned int* cnt_s, unsigned int* wave_n, const unsigned int* len, unsigned int* off, const unsigned int* wg_sum,
                                           const unsigned int* wg_cnt, unsigned int* counters, unsigned int nmax, const unsigned int* total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) { *base_s = 0; *cnt_s = 0; }
    __syncthreads();
    unsigned int s = 0, c = 0;
    for (unsigned int j = threadIdx.x; j < blockIdx.x; j += PK_WG) { s += wg_sum[j]; c += wg_cnt[j]; }
    if (s) atomicAdd(base_s, s);
    if (c) atomicAdd(cnt_s, c);
    const unsigned int i = blockIdx.x * PK_WG + threadIdx.x;
    const unsigned int v = (i < nmax && i < *total) ? len[i] : 0u;
    unsigned int incl = v;                                                       // inclusive scan within the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned int t = (unsigned int)__shfl((int)incl, lane >= o ? lane - o : lane);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wave_n[wv] = incl;
    __syncthreads();
    unsigned int before = *base_s;
    for (int w = 0; w < wv; ++w) before += wave_n[w];
    if (i < nmax) off[i] = before + incl - v;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        unsigned int t = *base_s;
        for (int w = 0; w < PK_WG / 64; ++w) t += wave_n[w];
        counters[0] = t;
        counters[1] = *cnt_s + wg_cnt[blockIdx.x];
    }
}

// ---- out.  The wave's row holds the record at row[a, a + len), a = off & 15; row byte x <-> output byte (off - a) + x;
// chunk c = row[16 c, 16 c + 16).  The caller has fenced the row's LDS writes and checked off + len against the output.
__device__ __forceinline__ void pk_flush_row(const unsigned char* row, unsigned char* out, unsigned int off, unsigned int len, int lane)
{
    const unsigned int a = off & 15u;
    unsigned char* dst = out + (off - a);                                        // 16-byte aligned
    const unsigned int end = a + len;
    const unsigned int c0 = (a + 15u) >> 4, c1 = end >> 4;                       // whole chunks: [c0, c1)
    const unsigned int head_end = c1 > c0 ? 16u * c0 : end;                      // no whole chunk: everything leaves as bytes
    const unsigned int tail_beg = c1 > c0 ? 16u * c1 : end;
    for (unsigned int x = a + lane; x < head_end; x += 64) dst[x] = row[x];      // (< 16 bytes, or < 31 when no chunk is whole)
    for (unsigned int x = tail_beg + lane; x < end; x += 64) dst[x] = row[x];
    for (unsigned int c = c0 + lane; c < c1; c += 64) ((uint4*)dst)[c] = ((const uint4*)row)[c];
}

// ---- the passes' bodies.  recs: PK_WAVES records of LDS; rows: PK_WAVES rows of F::REC_MAX + 16 bytes (the record at its output
// offset mod 16), both 16-byte aligned and the calling kernel's own.
__device__ __forceinline__ void pk_keys(const AcgSinkPass& p)
{
    const unsigned int i = blockIdx.x * PK_WG + threadIdx.x;
    if (i >= p.nmax || i >= *p.total) return;
    p.key[i] = pk_key(p.recs + i, p);
    p.idx[i] = i;
}

// the wave's rank r has passed the kernel's own early-outs (out of range; a dropped record: length 0).  They stay in the kernel:
// as returns inside an inlined function the compiler merges the two stores to len[r] and the kernel comes out longer.
template <class F>
__device__ __forceinline__ void pk_measure(unsigned char (*recs)[PK_REC], const AcgSinkPass& p, unsigned int r)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    pk_load(recs[wv], p.recs, p.oooi, p.idx_s[r], lane);
    bool nm;
    const unsigned int n = F::template record<false>(recs[wv], nullptr, p, lane, &nm);
    if (lane == 0) p.len[r] = n > F::REC_MAX ? F::REC_MAX : n;
}

template <class F>
__device__ __forceinline__ void pk_render(unsigned char (*recs)[PK_REC], unsigned char (*rows)[F::REC_MAX + 16], const AcgSinkPass& p)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned int r = blockIdx.x * PK_WAVES + wv;                           // wave-uniform
    if (r >= p.nmax || r >= *p.total) return;
    const unsigned int len = p.len[r], off = p.off[r];
    if (len == 0 || len > F::REC_MAX || off > p.out_cap || len > p.out_cap - off) return;
    pk_load(recs[wv], p.recs, p.oooi, p.idx_s[r], lane);
    bool near_mid;
    const unsigned int n = F::template record<true>(recs[wv], F::row_at(rows, wv, off), p, lane, &near_mid);
    if (n != len) return;                                                        // (cannot happen: one function measures and renders)
    if (near_mid && lane == 0) atomicAdd(&p.counters[2], 1u);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    pk_flush_row(rows[wv], p.out, off, len, lane);
}

// A unit's part of the launch sequence (outs.hip, acg_launch_outs, which has ordered the take once for all its formats: key_s /
// idx_s are filled), on the stream of the label pass it hangs on.  One of the unit's two wave-per-record kernels per call --
// measure, then render -- because the scan between them runs over all the caller's formats at once.
typedef void (*PkKernel)(AcgSinkPass);
static inline int pk_launch_sorted(const AcgSinkPass* p, void* stream, int phase, PkKernel measure, PkKernel render)
{
    if (p->nmax == 0) return 0;
    const unsigned int gw = (p->nmax + PK_WAVES - 1) / PK_WAVES;
    hipLaunchKernelGGL(phase == ACG_SORTED_MEASURE ? measure : render, dim3(gw), dim3(64 * PK_WAVES), 0, (hipStream_t)stream, *p);
    return (int)hipGetLastError();
}
