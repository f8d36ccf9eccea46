// flight.hip -- addFlight() and routejson() (output.c:361-456) for the batch sink: the flight table that the monitor (-o 3) and
// the route records (-o 5) are printed from, kept on the device across calls.
//
// The reference walks a move-to-front list once per message.  Here one pass handles all messages a drain / collect consumes:
//   flight_extract_kernel (label.hip)  a thread per record: the messages that reach addFlight() become events (aircraft key,
//                                      tv, fid, decoded OOOI fields, "passes -e") with the sort key (end_sample, chn);
//   fl_events_import_kernel            only at the owner of a table shared by several contexts, when events of the others
//                                      are queued: they join the pass's events (a peer's pass ends here instead:
//                                      fl_events_export_kernel hands its events out and nothing below runs);
//   flight_sort_kernel                 the events in time order;
//   flight_order_kernel                tv_sec in that order and its inclusive running maximum seeded with the table's G:
//                                      pmax[r - 1] is the newest second any message BEFORE event r carried;
//   flight_sort_kernel                 stable by aircraft key: one contiguous segment per aircraft, time order inside;
//   flight_heads_kernel                a thread per event: a segment's first event looks its aircraft up in the table (a
//                                      probe per aircraft, all in parallel), marks the slot as used by this pass and queues
//                                      the segment;
//   flight_walk_kernel                 one WAVE per segment, 64 events at a time (below);
//   flight_finish_kernel               G = the pass's last running maximum; the counters are re-armed.
//
// THE LAZY EXPIRY RULE.  The reference deletes, after every message, each entry with tl.tv_sec < tv.tv_sec - mdly.  Here an
// entry is live iff tl_sec + mdly >= G, G being the largest tv_sec seen so far, and event r restarts its aircraft's entry when
// pmax[r - 1] > tl_sec + mdly (tl_sec of the aircraft's previous event, or of the stored entry).  The two differ only if a
// message is processed after one whose tv_sec is more than mdly larger; in (end_sample, chn) order tv runs backwards by less
// than a block (< 0.87 s), tv_sec by at most 1, and mdly >= 1 (tests/test_flight_model.py pins this against the list walk).
//
// THE WALK.  The wave keeps the entry in registers (every lane the same values).  Per 64 events: the restart decisions of all
// lanes are one ballot; between two restarts (rare) lies a range that is folded into the entry without a loop over its events
// -- nbm += its length, chm |= an OR reduction, fid / tl = its last event's, each OOOI field = the value of the LAST lane that
// has one (ballot + find-last), the route = the FIRST lane that passes -e, has a fid and knows sa and da at or before it
// (ballot + find-first).  An aircraft that carries a third of all traffic costs its segment length / 64 such steps, not one
// dependent memory round trip per message.
//
// THE TABLE.  Open addressing, linear probing, keyed by the 64-bit addr word.  A slot never becomes empty again, so a probe
// chain is never cut: an expired entry keeps its key (its aircraft finds it and restarts it in place) and is its own
// tombstone.  An aircraft that is NOT in the table takes the first slot on its probe path that is empty or expired -- expired
// with respect to G before the pass AND not used by this pass (flight_heads_kernel has marked every slot whose aircraft has
// events in this pass before any insertion starts, so no wave can be working on the slot that is taken over).  The claim is
// one compare-and-swap on the slot's `touch` word; the loser probes on.  Lookup and search end after FL_PROBE (128) slots
// or, the lookup, at an empty slot: an aircraft that finds no such slot within them is counted in `dropped`, so a table filled
// to its last slots can drop an aircraft before it is completely full.
//
// Routes go to a queue through a counter, tagged (pass, rank of the triggering event); the host orders them by that tag when
// it hands them out.  The snapshot compacts the live slots through a counter and sorts their (~seq, slot) pairs.
//
// THE SORT is the pass's own: a few thousand keys per call do not need a library's tuned multi-kernel sort (rocPRIM's
// instantiations for these three uses are 4 MB of code objects, three times the rest of the library).  flight_sort_kernel is
// ONE workgroup: a stable least-significant-digit radix sort, 8 bits per pass, a pass = an LDS histogram, then tiles of 1024
// keys in order, each key ranked among its wave's equal digits by eight ballots.  A digit that is the same in every key costs
// its histogram only: of the 64 bits of (end_sample, chn) the samples of one call and the channel number differ in three or
// four digits, an addr in seven.
#include <hip/hip_runtime.h>
#include <limits.h>
#include "acg_internal.h"
#include "acarsdec_amd.h"

#define FL_WG 256
#define FL_WAVES (FL_WG / 64)

static_assert(sizeof(acg_flight) == 120 && offsetof(acg_flight, chm) == 32 && offsetof(acg_flight, da) == 80, "acg_flight layout");
static_assert(sizeof(acg_route) == 56 && offsetof(acg_route, fid) == 24 && offsetof(acg_route, addr) == 41, "acg_route layout");
static_assert(sizeof(AcgFlightSlot) == 120 && sizeof(AcgFlightEv) == 88, "device layouts");

// An aircraft lives within FL_PROBE slots of its hash: a lookup that misses, and the search for a slot to take, end there (or at
// an empty slot), so neither grows with the table's age or size -- slots never become empty again, and without the bound a table
// that has seen many aircraft would send every new one round the whole table.
#define FL_PROBE 128u

__device__ __forceinline__ unsigned int fl_hash(unsigned long long k)
{
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (unsigned int)k;
}

__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int src)
{
    const unsigned int lo = (unsigned int)__shfl((int)(unsigned int)v, src);
    const unsigned int hi = (unsigned int)__shfl((int)(unsigned int)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned int shfl32(unsigned int v, int src) { return (unsigned int)__shfl((int)v, src); }

__device__ __forceinline__ unsigned long long lanes_upto(int lane)     // bits 0 .. lane
{
    return lane >= 63 ? ~0ull : ((2ull << lane) - 1ull);
}

__device__ __forceinline__ int last_bit(unsigned long long m) { return 63 - __clzll((long long)m); }
__device__ __forceinline__ int first_bit(unsigned long long m) { return __ffsll((unsigned long long)m) - 1; }

#define RS_WG 1024
#define RS_WAVES (RS_WG / 64)

// Stable LSD radix sort of n (key, value) pairs by one workgroup; n = *n_ptr (a device counter) or n_fixed.  The pairs start in
// (ka, va), passes go back and forth between (ka, va) and (kb, vb), and the result always ends in (kb, vb).
__global__ __launch_bounds__(RS_WG) void flight_sort_kernel(unsigned long long* ka, unsigned int* va, unsigned long long* kb, unsigned int* vb,
                                                            const unsigned int* n_ptr, unsigned int n_fixed)
{
    __shared__ unsigned int hist[256];
    __shared__ unsigned int wcnt[RS_WAVES][256];
    __shared__ unsigned int same[2];                                     // (two: a pass re-arms the NEXT pass's flag)
    const unsigned int n = n_ptr ? *n_ptr : n_fixed;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid < 2) same[tid] = 0;
    unsigned long long *ks = ka, *kd = kb;
    unsigned int *vs = va, *vd = vb;
    for (int shift = 0; shift < 64; shift += 8) {
        if (tid < 256) hist[tid] = 0;
        const int par = (shift >> 3) & 1;
        __syncthreads();
        // (behind the pass's first barrier: every wave has read the previous pass's flag, which is this word, by now)
        if (tid == 0) same[par ^ 1] = 0;
        for (unsigned int i = tid; i < n; i += RS_WG) atomicAdd(&hist[(unsigned int)(ks[i] >> shift) & 255u], 1u);
        __syncthreads();
        if (tid < 256 && hist[tid] == n) same[par] = 1;                       // every key has this digit: the pass would move nothing
        __syncthreads();
        if (same[par]) continue;
        if (tid == 0) {                                                  // digit -> first position (256 LDS words: not worth a scan)
            unsigned int run = 0;
            for (int d = 0; d < 256; ++d) {
                const unsigned int c = hist[d];
                hist[d] = run;
                run += c;
            }
        }
        for (unsigned int t0 = 0; t0 < n; t0 += RS_WG) {
            const unsigned int i = t0 + (unsigned int)tid;
            const bool valid = i < n;
            unsigned long long key = 0;
            unsigned int val = 0, d = 0;
            if (valid) {
                key = ks[i];
                val = vs[i];
                d = (unsigned int)(key >> shift) & 255u;
            }
            // the lanes of this wave with the same digit, and this lane's rank among them (input order: the sort is stable)
            unsigned long long peers = __ballot(valid);
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const unsigned long long bm = __ballot(valid && ((d >> b) & 1u));
                peers &= ((d >> b) & 1u) ? bm : ~bm;
            }
            const unsigned int rank = (unsigned int)__popcll(peers & ((1ull << lane) - 1ull));
#pragma unroll
            for (int q = 0; q < 4; ++q) wcnt[wv][lane + 64 * q] = 0;
            __syncthreads();                                             // (also: hist's positions are written)
            if (valid && rank == 0) wcnt[wv][d] = (unsigned int)__popcll(peers);
            __syncthreads();
            if (tid < 256) {                                             // per digit: where each wave's keys go, and the next tile's start
                unsigned int run = hist[tid];
                for (int w = 0; w < RS_WAVES; ++w) {
                    const unsigned int c = wcnt[w][tid];
                    wcnt[w][tid] = run;
                    run += c;
                }
                hist[tid] = run;
            }
            __syncthreads();
            if (valid) {
                const unsigned int at = wcnt[wv][d] + rank;
                kd[at] = key;
                vd[at] = val;
            }
            __syncthreads();
        }
        unsigned long long* kt = ks; ks = kd; kd = kt;
        unsigned int* vt = vs; vs = vd; vd = vt;
        __threadfence_block();
        __syncthreads();
    }
    if (ks != kb)                                                        // an even number of passes: the result lies in (ka, va)
        for (unsigned int i = tid; i < n; i += RS_WG) {
            kb[i] = ks[i];
            vb[i] = vs[i];
        }
}

// One workgroup: tv_sec of the events in time order and its inclusive running maximum, seeded with G; the aircraft keys and
// the time ranks for the second sort.
__global__ __launch_bounds__(RS_WG) void flight_order_kernel(AcgFlightPass p)
{
    __shared__ long long wtot[RS_WAVES];
    __shared__ long long carry_s;
    const unsigned int m = p.st->m;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) carry_s = p.st->G;
    __syncthreads();
    for (unsigned int t0 = 0; t0 < m; t0 += RS_WG) {
        const unsigned int r = t0 + (unsigned int)tid;
        long long sec = LLONG_MIN;
        if (r < m) {
            const AcgFlightEv* e = p.ev + p.idx1s[r];
            sec = e->sec;
            p.key2[r] = e->key;
            p.rank2[r] = r;
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const long long o = (long long)shfl64((unsigned long long)sec, lane >= off ? lane - off : lane);
            if (lane >= off && o > sec) sec = o;
        }
        if (lane == 63) wtot[wv] = sec;
        __syncthreads();
        long long before = carry_s;
        for (int w = 0; w < wv; ++w) before = wtot[w] > before ? wtot[w] : before;
        if (before > sec) sec = before;
        if (r < m) p.pmax[r] = sec;
        __syncthreads();
        if (tid == RS_WG - 1) carry_s = sec;
        __syncthreads();
    }
}

__global__ __launch_bounds__(FL_WG) void flight_heads_kernel(AcgFlightPass p, unsigned int n)
{
    const unsigned int q = blockIdx.x * FL_WG + threadIdx.x;
    if (q >= n || q >= p.st->m) return;                                   // (n = the records of the pass >= its events)
    const unsigned long long key = p.key2s[q];
    if (q > 0 && p.key2s[q - 1] == key) return;
    int slot = -1;
    unsigned int h = fl_hash(key) & (p.cap - 1);
    const unsigned int reach = p.cap < FL_PROBE ? p.cap : FL_PROBE;
    for (unsigned int t = 0; t < reach; ++t, h = (h + 1) & (p.cap - 1)) {
        const unsigned long long k = p.slots[h].key;
        if (k == key) {
            slot = (int)h;
            p.slots[h].touch = p.pass;                                  // nobody may take this slot over during this pass
            break;
        }
        if (k == 0) break;
    }
    const unsigned int at = atomicAdd(&p.st->nseg, 1u);
    p.segs[at] = make_uint2(q, (unsigned int)slot);
}

// the entry a wave folds its segment into: wave-uniform values
struct FlEntry {
    bool exists;
    unsigned long long seq, fid, chm;
    long long ts_sample, tl_sample, ts_sec, tl_sec;
    int ts_usec, tl_usec, first_chn, last_chn, nbm;
    unsigned int rt;
    unsigned int fld[7];
};

enum { FL_DA = 0, FL_SA = 1 };                                          // acg_oooi's field order

// lane 0: the first slot on the key's probe path that is empty or expired and not used by this pass; -1 = none within reach
__device__ int flight_claim(const AcgFlightPass& p, unsigned long long key, long long G)
{
    unsigned int h = fl_hash(key) & (p.cap - 1);
    const unsigned int reach = p.cap < FL_PROBE ? p.cap : FL_PROBE;
    for (unsigned int t = 0; t < reach; ++t, h = (h + 1) & (p.cap - 1)) {
        AcgFlightSlot* s = p.slots + h;
        const unsigned int touch = __hip_atomic_load(&s->touch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (touch == p.pass) continue;
        const unsigned long long k = __hip_atomic_load(&s->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const long long tl = __hip_atomic_load(&s->tl_sec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k != 0 && tl + (long long)p.mdly >= G) continue;             // live
        if (atomicCAS(&s->touch, touch, p.pass) != touch) continue;      // another wave took it (or its owner turned up)
        __hip_atomic_store(&s->key, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return (int)h;
    }
    return -1;
}

__global__ __launch_bounds__(FL_WG) void flight_walk_kernel(AcgFlightPass p)
{
    const int lane = threadIdx.x & 63;
    const unsigned int nwaves = gridDim.x * FL_WAVES;
    const unsigned int m = p.st->m, nseg = p.st->nseg;
    const long long G = p.st->G;                                         // before this pass (flight_finish_kernel moves it)
    const long long mdly = p.mdly;
    for (unsigned int seg = blockIdx.x * FL_WAVES + (threadIdx.x >> 6); seg < nseg; seg += nwaves) {
        const uint2 sg = p.segs[seg];
        const unsigned int q0 = sg.x;
        const unsigned long long key = p.key2s[q0];
        int slot = (int)sg.y;
        FlEntry E;
        E.exists = slot >= 0;
        if (slot < 0) {
            if (lane == 0) slot = flight_claim(p, key, G);
            slot = __builtin_amdgcn_readfirstlane(slot);
            if (slot < 0) {
                if (lane == 0) atomicAdd(&p.st->dropped, 1u);
                continue;
            }
        }
        AcgFlightSlot* S = p.slots + slot;
        E.seq = 0; E.fid = 0; E.chm = 0;
        E.ts_sample = E.tl_sample = E.ts_sec = E.tl_sec = 0;
        E.ts_usec = E.tl_usec = E.first_chn = E.last_chn = E.nbm = 0;
        E.rt = 0;
#pragma unroll
        for (int f = 0; f < 7; ++f) E.fld[f] = 0;
        if (E.exists) {                                                  // (every lane reads the same words: broadcast)
            E.seq = S->seq; E.fid = S->fid; E.chm = S->chm;
            E.ts_sample = S->ts_sample; E.tl_sample = S->tl_sample; E.ts_sec = S->ts_sec; E.tl_sec = S->tl_sec;
            E.ts_usec = S->ts_usec; E.tl_usec = S->tl_usec; E.first_chn = S->first_chn; E.last_chn = S->last_chn;
            E.nbm = S->nbm; E.rt = S->rt;
#pragma unroll
            for (int f = 0; f < 7; ++f) E.fld[f] = S->fld[f];
        }
        for (unsigned int base = q0;; base += 64) {
            const unsigned int q = base + (unsigned int)lane;
            const bool valid = q < m && p.key2s[q] == key;
            const unsigned long long vm = __ballot(valid);               // (a prefix of the lanes: the segment is contiguous)
            const int cnt = __popcll(vm);
            if (cnt == 0) break;
            // ---- this lane's event
            unsigned int r = 0, e_ok = 0, fld[7] = {0, 0, 0, 0, 0, 0, 0};
            long long sec = 0, soh = 0, before = 0;
            int usec = 0, chn = 0;
            unsigned long long fid = 0;
            if (valid) {
                r = p.rank2s[q];
                const AcgFlightEv* e = p.ev + p.idx1s[r];
                sec = e->sec; soh = e->soh_sample; usec = e->usec; chn = e->chn; fid = e->fid; e_ok = e->e_ok;
#pragma unroll
                for (int f = 0; f < 7; ++f) {
                    const unsigned char* b = e->oooi + 5 * f;
                    fld[f] = (unsigned int)b[0] | ((unsigned int)b[1] << 8) | ((unsigned int)b[2] << 16) | ((unsigned int)b[3] << 24);
                }
                before = r ? p.pmax[r - 1] : G;                          // the newest second any earlier message carried
            }
            // ---- restarts: the previous event's tl (lane 0: the entry's)
            long long prev_tl = (long long)shfl64((unsigned long long)sec, lane ? lane - 1 : 0);
            bool prev_exists = true;
            if (lane == 0) { prev_tl = E.tl_sec; prev_exists = E.exists; }
            const bool restart = valid && (!prev_exists || before > prev_tl + mdly);
            const unsigned long long rm = __ballot(restart);
            for (int a = 0; a < cnt;) {
                const unsigned long long higher = a >= 63 ? 0ull : (rm & ~((2ull << a) - 1ull));
                const int b = higher ? first_bit(higher) : cnt;          // the range [a, b)
                if ((rm >> a) & 1ull) {                                  // a new entry, created by event a (output.c:374-384)
                    E.exists = true;
                    E.ts_sample = (long long)shfl64((unsigned long long)soh, a);
                    E.ts_sec = (long long)shfl64((unsigned long long)sec, a);
                    E.ts_usec = (int)shfl32((unsigned int)usec, a);
                    E.first_chn = (int)shfl32((unsigned int)chn, a);
                    E.nbm = 0; E.chm = 0; E.rt = 0; E.fid = 0;
#pragma unroll
                    for (int f = 0; f < 7; ++f) E.fld[f] = 0;
                }
                const bool inr = lane >= a && lane < b;
                // ---- the route (output.c:433): the first event that passed -e, has a fid, and knows sa and da by then
                const unsigned long long sam = __ballot(inr && (fld[FL_SA] & 0xffu)), dam = __ballot(inr && (fld[FL_DA] & 0xffu));   // (sa[0], da[0]: output.c:392-393)
                const unsigned long long upto = lanes_upto(lane);
                const bool cand = inr && e_ok && (fid & 0xffull) && ((E.fld[FL_SA] & 0xffu) || (sam & upto)) && ((E.fld[FL_DA] & 0xffu) || (dam & upto));
                const unsigned long long cm = __ballot(cand);
                if (E.rt == 0 && cm) {
                    const int k = first_bit(cm);
                    const unsigned long long uk = lanes_upto(k);
                    const unsigned int sa_k = shfl32(fld[FL_SA], (sam & uk) ? last_bit(sam & uk) : 0);
                    const unsigned int da_k = shfl32(fld[FL_DA], (dam & uk) ? last_bit(dam & uk) : 0);
                    const unsigned int sa = (sam & uk) ? sa_k : E.fld[FL_SA], da = (dam & uk) ? da_k : E.fld[FL_DA];
                    if (lane == k) {
                        const unsigned int at = atomicAdd(&p.st->nroutes, 1u);
                        if (at < p.route_cap) {
                            AcgRouteRec* R = p.routes + at;
                            unsigned long long* w = (unsigned long long*)R->r;
                            R->order = ((unsigned long long)p.pass << 32) | r;
                            w[0] = (unsigned long long)soh;
                            w[1] = (unsigned long long)sec;
                            w[2] = (unsigned long long)(unsigned int)usec | ((unsigned long long)(unsigned int)chn << 32);
                            // bytes 24..55: fid[7] sa[5] da[5] addr[8] reserved[7]
                            const unsigned long long sa5 = sa, da5 = da, ad = key & 0x00ffffffffffffffull;
                            w[3] = fid | (sa5 << 56);                               // fid 24..30, sa[0] 31
                            w[4] = (sa5 >> 8) | (da5 << 32);                        // sa[1..4] 32..35, da[0..3] 36..39
                            w[5] = (ad << 8);                                       // da[4] 40 (NUL), addr[0..6] 41..47
                            w[6] = 0ull;                                            // addr[7] 48, reserved
                        }
                    }
                    E.rt = 1;
                }
                // ---- the range folded into the entry (output.c:386-399)
                E.nbm += b - a;
                unsigned long long bits = inr ? 1ull << (chn & 63) : 0ull;
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) bits |= shfl64(bits, lane ^ off);
                E.chm |= bits;
                E.fid = shfl64(fid, b - 1);
#pragma unroll
                for (int f = 0; f < 7; ++f) {
                    const unsigned long long fm = __ballot(inr && (fld[f] & 0xffu));         // a field counts when its FIRST byte is not NUL
                    const unsigned int v = shfl32(fld[f], fm ? last_bit(fm) : 0);
                    if (fm) E.fld[f] = v;
                }
                E.tl_sample = (long long)shfl64((unsigned long long)soh, b - 1);
                E.tl_sec = (long long)shfl64((unsigned long long)sec, b - 1);
                E.tl_usec = (int)shfl32((unsigned int)usec, b - 1);
                E.last_chn = (int)shfl32((unsigned int)chn, b - 1);
                E.seq = ((unsigned long long)p.pass << 32) | shfl32(r, b - 1);
                a = b;
            }
            if (cnt < 64) break;
        }
        if (lane == 0) {
            S->seq = E.seq; S->fid = E.fid; S->chm = E.chm;
            S->ts_sample = E.ts_sample; S->tl_sample = E.tl_sample; S->ts_sec = E.ts_sec; S->tl_sec = E.tl_sec;
            S->ts_usec = E.ts_usec; S->tl_usec = E.tl_usec; S->first_chn = E.first_chn; S->last_chn = E.last_chn;
            S->nbm = E.nbm; S->rt = E.rt;
#pragma unroll
            for (int f = 0; f < 7; ++f) S->fld[f] = E.fld[f];
        }
    }
}

__global__ void flight_finish_kernel(AcgFlightPass p)
{
    const unsigned int m = p.st->m;
    if (m) p.st->G = p.pmax[m - 1];
    p.st->m = 0;
    p.st->nseg = 0;
}

// ---- the table across contexts: a peer's events leave (export), the owner takes them in (import) ------------------------------
static_assert(sizeof(acg_flight_event) == 88 && offsetof(acg_flight_event, chn) == 28 && offsetof(acg_flight_event, addr) == 32 &&
                  offsetof(acg_flight_event, e_ok) == 47 && offsetof(acg_flight_event, oooi) == 48 && offsetof(AcgFlightEv, oooi) == 40,
              "acg_flight_event layout");

// a 7-byte C string as a word: nothing behind its NUL counts (as the extraction reads addr and fid)
__device__ __forceinline__ unsigned long long fl_cstr7(unsigned long long v)
{
    v &= 0x00ffffffffffffffull;
    for (int b = 1; b < 7; ++b)
        if (((v >> (8 * (b - 1))) & 0xff) == 0) v &= (1ull << (8 * b)) - 1ull;
    return v;
}

// Export: a thread per extracted event (event i has the key key1[i]: the extraction writes idx1[i] = i).  The events are appended
// to the queue through its counter, one atomic per wave as in the extraction; an event without an address has no record.  The
// last workgroup out re-arms the pass's counters (nseg counts the workgroups here: the pass has no segments).
__global__ __launch_bounds__(FL_WG) void fl_events_export_kernel(AcgFlightPass p)
{
    const unsigned int m = p.st->m;
    const unsigned int i = blockIdx.x * FL_WG + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const AcgFlightEv* e = p.ev + i;
    const bool go = i < m && (e->key & 0xffull) != 0;
    const unsigned long long bm = __ballot(go);
    if (bm) {
        unsigned int base = 0;
        if (lane == 0) base = atomicAdd(&p.st->nexport, (unsigned int)__popcll(bm));
        base = (unsigned int)__shfl((int)base, 0);
        const unsigned int at = base + (unsigned int)__popcll(bm & ((1ull << lane) - 1ull));
        if (go && at < p.xq_cap) {
            unsigned long long* w = (unsigned long long*)((acg_flight_event*)p.xq + at);
            const unsigned long long* o = (const unsigned long long*)e->oooi;
            w[0] = p.key1[i] >> 20;                                          // end_sample
            w[1] = (unsigned long long)e->soh_sample;
            w[2] = (unsigned long long)e->sec;
            w[3] = (unsigned long long)(unsigned int)e->usec | ((unsigned long long)(unsigned int)e->chn << 32);
            w[4] = e->key & 0x00ffffffffffffffull;                           // addr[8]
            w[5] = e->fid | ((unsigned long long)(e->e_ok ? 1u : 0u) << 56); // fid[7], e_ok
#pragma unroll
            for (int k = 0; k < 5; ++k) w[6 + k] = o[k];
        }
    }
    __syncthreads();                                                         // (every wave of this workgroup has read m)
    if (threadIdx.x == 0 && atomicAdd(&p.st->nseg, 1u) == gridDim.x - 1) {
        p.st->m = 0;
        p.st->nseg = 0;
    }
}

// Import: a thread per uploaded event, appended to the pass's events behind (or among: the counter decides) the extracted ones,
// with the key of the time sort.  Runs between the extraction and the first sort.
__global__ __launch_bounds__(FL_WG) void fl_events_import_kernel(AcgFlightPass p)
{
    const unsigned int i = blockIdx.x * FL_WG + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool go = i < p.n_import;
    const unsigned long long bm = __ballot(go);
    if (!bm) return;
    unsigned int base = 0;
    if (lane == 0) base = atomicAdd(&p.st->m, (unsigned int)__popcll(bm));
    base = (unsigned int)__shfl((int)base, 0);
    if (!go) return;
    const unsigned int at = base + (unsigned int)__popcll(bm & ((1ull << lane) - 1ull));
    const unsigned long long* w = (const unsigned long long*)((const acg_flight_event*)p.imp + i);
    AcgFlightEv* e = p.ev + at;
    const unsigned int chn = (unsigned int)(w[3] >> 32);
    e->key = fl_cstr7(w[4]) | (1ull << 63);
    e->soh_sample = (long long)w[1];
    e->sec = (long long)w[2];
    e->usec = (int)(unsigned int)w[3];
    e->chn = (int)chn;
    e->fid = fl_cstr7(w[5]);
    unsigned long long* o = (unsigned long long*)e->oooi;
#pragma unroll
    for (int k = 0; k < 5; ++k) o[k] = w[6 + k];
    e->e_ok = (w[5] >> 56) & 0xffull ? 1u : 0u;
    e->pad_ = 0u;
    p.key1[at] = ((w[0] & ((1ull << 43) - 1ull)) << 20) | ((unsigned long long)chn & 0xfffffull);
    p.idx1[at] = at;
}

extern "C" int acg_launch_flight_pass(const AcgMsgRec* recs, unsigned int n, const AcgLabelFilter* f, const AcgFlightPass* p, void* stream)
{
    const unsigned int tot = n + p->n_import;                                // (the host keeps imports away from an exporting context)
    if (tot == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (n) {
        const int e = acg_launch_flight_extract(recs, n, f, p, stream);
        if (e) return e;
    }
    const unsigned int g = (tot + FL_WG - 1) / FL_WG;
    if (p->xq) {
        hipLaunchKernelGGL(fl_events_export_kernel, dim3(g), dim3(FL_WG), 0, s, *p);
        return (int)hipGetLastError();
    }
    if (p->n_import) hipLaunchKernelGGL(fl_events_import_kernel, dim3((p->n_import + FL_WG - 1) / FL_WG), dim3(FL_WG), 0, s, *p);
    hipLaunchKernelGGL(flight_sort_kernel, dim3(1), dim3(RS_WG), 0, s, p->key1, p->idx1, p->key1s, p->idx1s, (const unsigned int*)&p->st->m, 0u);
    hipLaunchKernelGGL(flight_order_kernel, dim3(1), dim3(RS_WG), 0, s, *p);
    hipLaunchKernelGGL(flight_sort_kernel, dim3(1), dim3(RS_WG), 0, s, p->key2, p->rank2, p->key2s, p->rank2s, (const unsigned int*)&p->st->m, 0u);
    hipLaunchKernelGGL(flight_heads_kernel, dim3(g), dim3(FL_WG), 0, s, *p, tot);
    // a wave per segment, the waves looping.  The host does not know the pass's events or segments (no round trip), only its n
    // records and imported events >= both: at most one wave per record, at most 1024 waves (as the block repair: what such a pass
    // costs beside the down-converter is workgroups finding a place, not the segments a wave takes in turn)
    unsigned int wgs = (tot + FL_WAVES - 1) / FL_WAVES;
    wgs = wgs > 256 ? 256 : wgs;
    hipLaunchKernelGGL(flight_walk_kernel, dim3(wgs), dim3(FL_WG), 0, s, *p);
    hipLaunchKernelGGL(flight_finish_kernel, dim3(1), dim3(1), 0, s, *p);
    return (int)hipGetLastError();
}

extern "C" int acg_launch_sort_pairs(unsigned long long* ka, unsigned int* va, unsigned long long* kb, unsigned int* vb, const unsigned int* n_ptr,
                                     unsigned int n_fixed, void* stream)
{
    hipLaunchKernelGGL(flight_sort_kernel, dim3(1), dim3(RS_WG), 0, (hipStream_t)stream, ka, va, kb, vb, n_ptr, n_fixed);
    return (int)hipGetLastError();
}

// ---- the snapshot: printmonitor()'s walk from the list head (output.c:467-481) = the live entries, latest update first
__global__ __launch_bounds__(FL_WG) void flight_snapkeys_kernel(AcgFlightPass p, unsigned long long* skey, unsigned int* sval)
{
    // the live slots, compacted through the counter (their order does not matter: seq is distinct), keyed ~seq so that the
    // ascending sort puts the latest update first; only these are sorted, however large the table is
    const unsigned int h = blockIdx.x * FL_WG + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const AcgFlightSlot* S = p.slots + h;
    const bool live = h < p.cap && S->key != 0 && S->seq != 0 && S->tl_sec + (long long)p.mdly >= p.st->G;
    const unsigned long long m = __ballot(live);
    if (!m) return;
    unsigned int base = 0;
    if (lane == 0) base = atomicAdd(&p.st->nlive, (unsigned int)__popcll(m));
    base = (unsigned int)__shfl((int)base, 0);
    if (!live) return;
    const unsigned int at = base + (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
    skey[at] = ~S->seq;
    sval[at] = h;
}

__global__ __launch_bounds__(FL_WG) void flight_snapshot_kernel(AcgFlightPass p, const unsigned long long* skey, const unsigned int* sval, unsigned char* out)
{
    const unsigned int i = blockIdx.x * FL_WG + threadIdx.x;
    if (i >= p.st->nlive) return;
    const AcgFlightSlot* S = p.slots + sval[i];
    unsigned long long* w = (unsigned long long*)(out + (size_t)i * sizeof(acg_flight));
    w[0] = S->key & 0x00ffffffffffffffull;                                           // addr[8]
    w[1] = S->fid | ((unsigned long long)(S->rt ? 1u : 0u) << 56);                    // fid[7], rt
    w[2] = (unsigned long long)(unsigned int)S->nbm | ((unsigned long long)(unsigned int)S->first_chn << 32);
    w[3] = (unsigned long long)(unsigned int)S->last_chn;                            // last_chn, reserved1
    w[4] = S->chm;
    w[5] = (unsigned long long)S->ts_sample;
    w[6] = (unsigned long long)S->tl_sample;
    w[7] = (unsigned long long)S->ts_sec;
    w[8] = (unsigned long long)S->tl_sec;
    w[9] = (unsigned long long)(unsigned int)S->ts_usec | ((unsigned long long)(unsigned int)S->tl_usec << 32);
    unsigned char* b = out + (size_t)i * sizeof(acg_flight) + 80;
    for (int f = 0; f < 7; ++f) {
        const unsigned int v = S->fld[f];
        b[5 * f] = (unsigned char)v; b[5 * f + 1] = (unsigned char)(v >> 8); b[5 * f + 2] = (unsigned char)(v >> 16);
        b[5 * f + 3] = (unsigned char)(v >> 24); b[5 * f + 4] = 0;
    }
    for (int k = 35; k < 40; ++k) b[k] = 0;
}

extern "C" int acg_launch_flight_snapkeys(const AcgFlightPass* p, unsigned long long* skey, unsigned long long* skey_s, unsigned int* sval,
                                          unsigned int* sval_s, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const unsigned int g = (p->cap + FL_WG - 1) / FL_WG;
    if (hipMemsetAsync(&p->st->nlive, 0, sizeof(unsigned int), s) != hipSuccess) return (int)hipErrorUnknown;
    hipLaunchKernelGGL(flight_snapkeys_kernel, dim3(g), dim3(FL_WG), 0, s, *p, skey, sval);
    hipLaunchKernelGGL(flight_sort_kernel, dim3(1), dim3(RS_WG), 0, s, skey, sval, skey_s, sval_s, (const unsigned int*)&p->st->nlive, 0u);
    return (int)hipGetLastError();
}

extern "C" int acg_launch_flight_snapshot(const AcgFlightPass* p, unsigned long long* skey, unsigned long long* skey_s, unsigned int* sval,
                                          unsigned int* sval_s, void* out, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const unsigned int g = (p->cap + FL_WG - 1) / FL_WG;
    const int e = acg_launch_flight_snapkeys(p, skey, skey_s, sval, sval_s, stream);
    if (e) return e;
    hipLaunchKernelGGL(flight_snapshot_kernel, dim3(g), dim3(FL_WG), 0, s, *p, (const unsigned long long*)skey_s, (const unsigned int*)sval_s, (unsigned char*)out);
    return (int)hipGetLastError();
}
