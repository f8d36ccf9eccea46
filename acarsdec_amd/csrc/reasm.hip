// reasm.hip -- reassembly of multi-block messages for the batch sink: the reference's call site of la_reasm_fragment_add()
// (output.c:33-101, 528-531, 552-559, 579-626, the HAVE_LIBACARS build) as a table kept on the device across calls.  The table's
// rule is tests/reasm_model.py, a plain dict walk: it follows libacars' documented behaviour from that call site outward and has
// not been run against libacars.  The H1 sublabel / MFI prefix that libacars strips per fragment is NOT stripped.
//
// One pass handles all records a drain / collect consumes, with the flight table's machinery (flight.hip):
//   reasm_extract_kernel   a thread per record: a record that did not pass -A / -b, a squitter (bid == 0) or bs == ETX is SKIPPED at
//                          once; the others become events (exact key of 12 characters in two words, seq, flags, tv_us, record
//                          index), compacted through a counter, with the time key (end_sample, chn);
//   acg_launch_sort_pairs  the events in time order;
//   reasm_gather_kernel    the upper key word in that order;      acg_launch_sort_pairs   stable by it;
//   reasm_gather_kernel    the lower key word in that order;      acg_launch_sort_pairs   stable by it: one contiguous segment per
//                          EXACT key, time order inside (a 64-bit hash would not do: keys differ in one character);
//   reasm_heads_kernel     a thread per event: a segment's first event looks its key up (linear probing, RS_PROBE slots, the full
//                          key compared), marks the slot as used by this pass and queues the segment;
//   reasm_walk_kernel      one WAVE per segment (below);
//   reasm_finish_kernel    G = the largest tv seen; the counters are re-armed.
//
// THE WALK.  The entry's header is wave-uniform state; the segment's events are loaded 64 at a time, one per lane, and applied one
// after the other (a segment is a handful of events).  A key that is absent claims a slot only when some event of its segment can
// create an entry; the claim is flight.hip's: the first slot on the probe path that was never used, or whose entry is idle or
// expired by more than 2 s against G, and that this pass has not marked -- one compare-and-swap on `touch`, the loser probes on.  tv
// runs backwards by less than a block in (end_sample, chn) order, so a reclaimed entry could not have been continued by anybody
// (tests/test_reasm_model.py proves it on the model).  A slot keeps its key as its own tombstone; a key that finds no slot is walked
// as if every creation failed (UNKNOWN on its creating events) and counted in `dropped` once.
//
// THE TEXT.  A fragment is appended by the 64 lanes through LDS: the record's text is read as aligned dwords, laid into LDS behind
// the bytes of the row's last incomplete dword (kept in the header: `tail`), and written to the row as whole aligned dwords.  No
// byte ever goes to global memory on its own and nothing is read back to merge a seam.  A COMPLETE copies the row in 16-byte chunks
// to the text queue and a fixed record to the record queue, tagged (pass, time key) for the host's final order.
#include <hip/hip_runtime.h>
#include <limits.h>
#include "acg_internal.h"
#include "acarsdec_amd.h"
#include "msg_keep.h"

#define RS_WG 256
#define RS_WAVES (RS_WG / 64)
#define RS_PROBE 128u                                                    // == flight.hip's FL_PROBE

static_assert(sizeof(AcgReasmEv) == 48 && sizeof(AcgReasmSlot) == 64 && sizeof(AcgReasmDone) == 96, "device layouts");
static_assert(sizeof(acg_reasm_msg) == 80 && offsetof(acg_reasm_msg, text_off) == 40 && offsetof(acg_reasm_msg, addr) == 53 &&
                  offsetof(acg_reasm_msg, msn) == 64,
              "acg_reasm_msg layout");
static_assert(offsetof(AcgMsgRec, txt) == 74 && sizeof(AcgMsgRec) % 8 == 0 && sizeof(AcgMsgRec) >= 72 + 62 * 4, "the append reads the record as aligned dwords from byte 72");

__device__ __forceinline__ unsigned int rs_hash(unsigned long long a, unsigned long long b)
{
    unsigned long long k = a ^ (b * 0x9e3779b97f4a7c15ull);
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (unsigned int)k;
}

// nb bytes as a word, a C string: nothing behind its NUL counts
__device__ __forceinline__ unsigned long long rs_cstr(const char* s, int nb)
{
    unsigned long long v = 0;
    bool open = true;
    for (int b = 0; b < nb; ++b) {
        const unsigned long long c = (unsigned char)s[b];
        open = open && c != 0;
        if (open) v |= c << (8 * b);
    }
    return v;
}

__device__ __forceinline__ long long rs_shfl64(long long v, int src)
{
    const unsigned int lo = (unsigned int)__shfl((int)(unsigned int)(unsigned long long)v, src);
    const unsigned int hi = (unsigned int)__shfl((int)(unsigned int)((unsigned long long)v >> 32), src);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

__global__ __launch_bounds__(RS_WG) void reasm_extract_kernel(const AcgMsgRec* recs, unsigned int n, AcgLabelFilter f, AcgReasmPass p)
{
    const unsigned int i = blockIdx.x * RS_WG + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const AcgMsgRec* r = recs + i;
    const bool ev = i < n && msg_keep_ab(r, f) && r->bs != 0x03 && r->bid != 0;
    if (i < n) p.status[i] = ev ? 0xffu : (unsigned int)ACG_REASM_SKIPPED;      // (an event's status: the walk's)
    const unsigned long long m = __ballot(ev);
    if (!m) return;
    unsigned int base = 0;
    if (lane == 0) base = atomicAdd(&p.st->m, (unsigned int)__popcll(m));
    base = (unsigned int)__shfl((int)base, 0);
    long long tv = LLONG_MIN;
    if (ev) {
        const unsigned int at = base + (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
        AcgReasmEv* e = p.ev + at;
        const bool down = r->bid >= '0' && r->bid <= '9';
        const bool final_ = r->be != 0x17;
        const int seq = (int)(signed char)(down ? r->no[3] : r->bid) - 65;
        const unsigned int wrap = down ? 0u : (r->mode == '2' ? 26u : 23u);
        const unsigned long long label = rs_cstr(r->label, 2);
        const long long soh = r->end_sample - (long long)r->soh_back;
        int len = r->txt_len;
        len = len < 0 ? 0 : len > ACG_MSG_TXT ? ACG_MSG_TXT : len;
        tv = p.t0_us + soh * 80ll;
        e->k0 = rs_cstr(r->addr, 7) | ((label & 0xffull) << 56);
        e->k1 = (label >> 8) | ((down ? rs_cstr(r->no, 3) : 0ull) << 8) | (1ull << 63);
        e->tv_us = tv;
        e->soh_sample = soh;
        e->rec = i;
        e->seq = seq;
        e->flags = (down ? ACG_RS_F_DOWN : 0u) | (final_ ? ACG_RS_F_FINAL : 0u) | (!final_ && (!down || seq == 0) ? ACG_RS_F_CREATES : 0u) |
                   (wrap << ACG_RS_WRAP_SHIFT);
        e->txt_len = (unsigned int)len;
        const int chn = p.chmap && (unsigned int)r->chn < p.nmap ? p.chmap[r->chn] : r->chn;
        p.ka[at] = (((unsigned long long)r->end_sample & ((1ull << 43) - 1ull)) << 20) | ((unsigned long long)(unsigned int)chn & 0xfffffull);
        p.va[at] = at;
    }
    // the pass's largest tv: one atomic per wave
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const long long o = rs_shfl64(tv, lane ^ off);
        tv = o > tv ? o : tv;
    }
    if (lane == 0) __hip_atomic_fetch_max(&p.st->Gnext, tv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the events' key word `hi ? k1 : k0` in the order the last sort left (vb), with the event index as the value
__global__ __launch_bounds__(RS_WG) void reasm_gather_kernel(AcgReasmPass p, int hi)
{
    const unsigned int q = blockIdx.x * RS_WG + threadIdx.x;
    if (q >= p.st->m) return;
    const unsigned int e = p.vb[q];
    p.ka[q] = hi ? p.ev[e].k1 : p.ev[e].k0;
    p.va[q] = e;
}

__global__ __launch_bounds__(RS_WG) void reasm_heads_kernel(AcgReasmPass p, unsigned int n)
{
    const unsigned int q = blockIdx.x * RS_WG + threadIdx.x;
    if (q >= n || q >= p.st->m) return;
    const AcgReasmEv* e = p.ev + p.vb[q];
    const unsigned long long k0 = e->k0, k1 = e->k1;
    if (q > 0) {
        const AcgReasmEv* b = p.ev + p.vb[q - 1];
        if (b->k0 == k0 && b->k1 == k1) return;
    }
    int slot = -1;
    unsigned int h = rs_hash(k0, k1) & (p.cap - 1);
    const unsigned int reach = p.cap < RS_PROBE ? p.cap : RS_PROBE;
    for (unsigned int t = 0; t < reach; ++t, h = (h + 1) & (p.cap - 1)) {
        const unsigned long long s1 = p.slots[h].k1;
        if (s1 == k1 && p.slots[h].k0 == k0) {
            slot = (int)h;
            p.slots[h].touch = p.pass;                                   // nobody may take this slot over during this pass
            break;
        }
        if (s1 == 0) break;
    }
    const unsigned int at = atomicAdd(&p.st->nseg, 1u);
    p.segs[at] = make_uint2(q, (unsigned int)slot);
}

// lane 0: the first slot on the key's probe path that is unused, idle or long expired, and not used by this pass; -1 = none
__device__ int reasm_claim(const AcgReasmPass& p, unsigned long long k0, unsigned long long k1, long long G)
{
    unsigned int h = rs_hash(k0, k1) & (p.cap - 1);
    const unsigned int reach = p.cap < RS_PROBE ? p.cap : RS_PROBE;
    for (unsigned int t = 0; t < reach; ++t, h = (h + 1) & (p.cap - 1)) {
        AcgReasmSlot* s = p.slots + h;
        const unsigned int touch = __hip_atomic_load(&s->touch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (touch == p.pass) continue;
        const unsigned long long s1 = __hip_atomic_load(&s->k1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned int live = __hip_atomic_load(&s->live, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const long long fu = __hip_atomic_load(&s->first_us, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const long long to = __hip_atomic_load(&s->timeout_us, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (s1 != 0 && live && !(G > fu + to + 2000000ll)) continue;     // in use
        if (atomicCAS(&s->touch, touch, p.pass) != touch) continue;      // another wave took it
        __hip_atomic_store(&s->k0, k0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&s->k1, k1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return (int)h;
    }
    return -1;
}

// the entry a wave walks its segment through: wave-uniform values
struct RsEntry {
    bool live;
    int prev;
    unsigned int text_len, nfrag, tail;
    long long first_us, timeout_us, first_soh;
};

#define RS_LDS_WAVE 256          // bytes per wave: up to 3 seam bytes + 242 of text, zero padded to whole dwords

__global__ __launch_bounds__(RS_WG) void reasm_walk_kernel(const AcgMsgRec* recs, AcgReasmPass p)
{
    __shared__ unsigned int stage[RS_WAVES][RS_LDS_WAVE / 4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned int* lds = stage[wv];
    unsigned char* ldsb = (unsigned char*)lds;
    const unsigned int nwaves = gridDim.x * RS_WAVES;
    const unsigned int m = p.st->m, nseg = p.st->nseg;
    const long long G = p.st->G;                                         // before this pass (reasm_finish_kernel moves it)
    for (unsigned int seg = blockIdx.x * RS_WAVES + (unsigned int)wv; seg < nseg; seg += nwaves) {
        const uint2 sg = p.segs[seg];
        const unsigned int q0 = sg.x;
        const AcgReasmEv* head = p.ev + p.vb[q0];
        const unsigned long long k0 = head->k0, k1 = head->k1;
        int slot = (int)sg.y;
        const bool found = slot >= 0;
        if (!found) {
            // does any event of the segment create an entry?  (only then is a slot worth taking)
            bool any = false;
            for (unsigned int base = q0; !any; base += 64) {
                const unsigned int q = base + (unsigned int)lane;
                bool valid = false, cr = false;
                if (q < m) {
                    const AcgReasmEv* e = p.ev + p.vb[q];
                    valid = e->k0 == k0 && e->k1 == k1;
                    cr = valid && (e->flags & ACG_RS_F_CREATES);
                }
                any = __ballot(cr) != 0ull;
                if (__popcll(__ballot(valid)) < 64) break;
            }
            if (any) {
                if (lane == 0) {
                    slot = reasm_claim(p, k0, k1, G);
                    if (slot < 0) atomicAdd(&p.st->dropped, 1u);
                }
                slot = __builtin_amdgcn_readfirstlane(slot);
            }
        }
        AcgReasmSlot* S = slot >= 0 ? p.slots + slot : nullptr;
        unsigned char* row = slot >= 0 ? p.rows + (size_t)slot * p.max_text : nullptr;
        RsEntry E;
        E.live = false; E.prev = ACG_RS_PREV_NONE; E.text_len = E.nfrag = E.tail = 0;
        E.first_us = E.timeout_us = E.first_soh = 0;
        if (found) {                                                     // (every lane reads the same words: broadcast)
            E.live = S->live != 0; E.prev = S->prev; E.text_len = S->text_len; E.nfrag = S->nfrag; E.tail = S->tail;
            E.first_us = S->first_us; E.timeout_us = S->timeout_us; E.first_soh = S->first_soh;
        }
        for (unsigned int base = q0;; base += 64) {
            const unsigned int q = base + (unsigned int)lane;
            bool valid = false;
            unsigned int rec = 0, flags = 0, tlen = 0, mine = 0;
            int seq = 0;
            long long tv = 0, soh = 0;
            if (q < m) {
                const AcgReasmEv* e = p.ev + p.vb[q];
                valid = e->k0 == k0 && e->k1 == k1;
                rec = e->rec; flags = e->flags; tlen = e->txt_len; seq = e->seq; tv = e->tv_us; soh = e->soh_sample;
            }
            const int cnt = __popcll(__ballot(valid));                   // (a prefix of the lanes: the segment is contiguous)
            for (int j = 0; j < cnt; ++j) {
                const unsigned int fl = (unsigned int)__shfl((int)flags, j), len = (unsigned int)__shfl((int)tlen, j);
                const unsigned int rj = (unsigned int)__shfl((int)rec, j);
                const int sq = __shfl(seq, j);
                const long long t = rs_shfl64(tv, j);
                const bool down = fl & ACG_RS_F_DOWN, final_ = fl & ACG_RS_F_FINAL;
                const int wrap = (int)((fl >> ACG_RS_WRAP_SHIFT) & 0xffu);
                unsigned int s;
                if (slot >= 0 && E.live && t > E.first_us + E.timeout_us) E.live = false;       // strict; the ENTRY's time-out
                if (!E.live && down && sq != 0) s = ACG_REASM_OUT_OF_SEQUENCE;
                else if (!E.live && final_) s = ACG_REASM_SKIPPED;
                else if (slot < 0) s = ACG_REASM_UNKNOWN;                // the key found no slot: the creation fails
                else {
                    if (!E.live) {
                        E.live = true; E.prev = ACG_RS_PREV_NONE; E.text_len = 0; E.nfrag = 0; E.tail = 0;
                        E.first_us = t; E.timeout_us = (down ? 660ll : 90ll) * 1000000ll; E.first_soh = rs_shfl64(soh, j);
                    }
                    if (wrap && sq == 0 && E.prev != ACG_RS_PREV_NONE && E.prev + 1 == wrap) E.prev = -1;
                    if (E.prev != ACG_RS_PREV_NONE && sq == E.prev) s = ACG_REASM_DUPLICATE;
                    else if (E.prev != ACG_RS_PREV_NONE && sq != E.prev + 1) { E.live = false; s = ACG_REASM_OUT_OF_SEQUENCE; }
                    else if (E.text_len + len > p.max_text) { E.live = false; s = ACG_REASM_OVERFLOW; }
                    else {
                        // ---- the append: [seam bytes | text] laid into LDS from the row's last dword boundary, stored as dwords
                        const unsigned int sh = E.text_len & 3u, a0 = E.text_len - sh, tot = sh + len;
                        if (len) {
                            lds[lane] = lane == 0 ? E.tail : 0u;
                            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                            if (lane < 62) {
                                const unsigned int w = ((const unsigned int*)((const unsigned char*)(recs + rj) + 72))[lane];
#pragma unroll
                                for (int k = 0; k < 4; ++k) {
                                    const int ti = 4 * lane + k - 2;     // the text's index of this byte
                                    if (ti >= 0 && ti < (int)len) ldsb[sh + (unsigned int)ti] = (unsigned char)(w >> (8 * k));
                                }
                            }
                            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                            const unsigned int nd = (tot + 3u) >> 2;     // <= 62; a0 + 4 nd <= max_text (a multiple of 16)
                            if ((unsigned int)lane < nd) ((unsigned int*)(row + a0))[lane] = lds[lane];
                            E.tail = (tot & 3u) ? lds[tot >> 2] : 0u;
                            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                        }
                        E.text_len += len; E.nfrag += 1; E.prev = sq;
                        s = ACG_REASM_IN_PROGRESS;
                        if (final_) {
                            E.live = false;
                            s = ACG_REASM_COMPLETE;
                            const unsigned int len16 = (E.text_len + 15u) & ~15u;
                            unsigned int at = 0;
                            unsigned long long toff = 0;
                            if (lane == 0) {
                                at = atomicAdd(&p.st->ndone, 1u);
                                toff = atomicAdd(&p.st->tbytes, (unsigned long long)len16);
                            }
                            at = (unsigned int)__shfl((int)at, 0);
                            toff = (unsigned long long)rs_shfl64((long long)toff, 0);
                            if (at < p.done_cap && toff + len16 <= p.text_cap) {
                                __threadfence();                         // the row's dwords, other lanes' stores among them
                                const uint4* src = (const uint4*)row;
                                uint4* dst = (uint4*)(p.texts + toff);
                                for (unsigned int c = (unsigned int)lane; c < len16 / 16u; c += 64u) dst[c] = src[c];
                                if (lane == 0) {
                                    const AcgMsgRec* r = recs + rj;
                                    const int chn = p.chmap && (unsigned int)r->chn < p.nmap ? p.chmap[r->chn] : r->chn;
                                    AcgReasmDone* D = p.done + at;
                                    unsigned long long* w = (unsigned long long*)D->r;
                                    const unsigned long long ad = k0 & 0x00ffffffffffffffull;
                                    D->tkey = (((unsigned long long)r->end_sample & ((1ull << 43) - 1ull)) << 20) | ((unsigned long long)(unsigned int)chn & 0xfffffull);
                                    D->pass = p.pass;
                                    D->pad_ = 0u;
                                    w[0] = (unsigned long long)(unsigned int)chn | ((unsigned long long)E.nfrag << 32);
                                    w[1] = (unsigned long long)r->end_bit;
                                    w[2] = (unsigned long long)r->end_sample;
                                    w[3] = (unsigned long long)(r->end_sample - (long long)r->soh_back);
                                    w[4] = (unsigned long long)E.first_soh;
                                    w[5] = toff;
                                    w[6] = (unsigned long long)E.text_len | ((unsigned long long)(down ? 1u : 0u) << 32) | ((ad & 0xffffffull) << 40);
                                    w[7] = (ad >> 24) | ((k0 >> 56) << 40) | ((k1 & 0xffull) << 48);
                                    w[8] = (k1 >> 8) & 0xffffffull;
                                    w[9] = 0ull;
                                }
                            } else if (lane == 0) {
                                atomicAdd(&p.st->qfull, 1u);
                            }
                        }
                    }
                }
                if (lane == j) mine = s;
            }
            if (valid) p.status[rec] = mine;
            if (cnt < 64) break;
        }
        if (S && lane == 0) {
            S->live = E.live ? 1u : 0u; S->prev = E.prev; S->text_len = E.text_len; S->nfrag = E.nfrag; S->tail = E.tail;
            S->first_us = E.first_us; S->timeout_us = E.timeout_us; S->first_soh = E.first_soh;
        }
    }
}

__global__ void reasm_finish_kernel(AcgReasmPass p)
{
    if (p.st->Gnext > p.st->G) p.st->G = p.st->Gnext;
    p.st->m = 0;
    p.st->nseg = 0;
}

extern "C" int acg_launch_reasm_pass(const AcgMsgRec* recs, unsigned int n, const AcgLabelFilter* f, const AcgReasmPass* p, void* stream)
{
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const unsigned int g = (n + RS_WG - 1) / RS_WG;
    const unsigned int* m = (const unsigned int*)&p->st->m;
    hipLaunchKernelGGL(reasm_extract_kernel, dim3(g), dim3(RS_WG), 0, s, recs, n, *f, *p);
    int e = acg_launch_sort_pairs(p->ka, p->va, p->kb, p->vb, m, 0u, stream);                     // time order
    if (e) return e;
    hipLaunchKernelGGL(reasm_gather_kernel, dim3(g), dim3(RS_WG), 0, s, *p, 1);
    e = acg_launch_sort_pairs(p->ka, p->va, p->kb, p->vb, m, 0u, stream);                         // stable by the upper key word
    if (e) return e;
    hipLaunchKernelGGL(reasm_gather_kernel, dim3(g), dim3(RS_WG), 0, s, *p, 0);
    e = acg_launch_sort_pairs(p->ka, p->va, p->kb, p->vb, m, 0u, stream);                         // ... and by the lower: exact-key segments
    if (e) return e;
    hipLaunchKernelGGL(reasm_heads_kernel, dim3(g), dim3(RS_WG), 0, s, *p, n);
    unsigned int wgs = (n + RS_WAVES - 1) / RS_WAVES;                    // at most one wave per record, at most 1024 waves (flight.hip)
    wgs = wgs > 256 ? 256 : wgs;
    hipLaunchKernelGGL(reasm_walk_kernel, dim3(wgs), dim3(RS_WG), 0, s, recs, *p);
    hipLaunchKernelGGL(reasm_finish_kernel, dim3(1), dim3(1), 0, s, *p);
    return (int)hipGetLastError();
}
