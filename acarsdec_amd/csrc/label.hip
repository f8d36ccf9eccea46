// label.hip -- the rest of outputmsg() for the batch sink: the CLI's message filters (-A, -b, -e: output.c:537-540,650) and
// label.c's DecodeLabel() (departure / destination, ETA, OOOI times), over the records msg_split_kernel (blk.hip) wrote for one
// drain / collect, then compacted in ring order so that only kept records cross to the host.
//
// Two launches over the call's `take` records, a thread per record (thousands of records per call, not millions):
//   msg_keep_count_kernel   the filter decision of every record, counted per workgroup;
//   msg_compact_kernel      each workgroup sums the counts of the workgroups before it (its base), ranks its kept records with
//                           a ballot per wave, copies them and their decoded labels to base + rank, and the last workgroup
//                           publishes the total.  The decision is the same function in both kernels: nothing is stored between.
// Deterministic: positions follow the input order whatever order the workgroups run in.
// With the flight table on (acg_flights_enable) a third launch, flight_extract_kernel, turns the same records into the events
// of flight.hip's pass, which follows on the same stream.
//
// The decoder is TABLE-DRIVEN: per label a list of guards (bytes at an offset equal one of at most two strings) and a list of
// copies (field <- 4 bytes at an offset), applied in order (label 44 writes eta twice: the later copy wins).  Success = every
// guard passes; on failure the record is all zero (the reference discards a partial fill).  Label 44's optional "00" prefix
// shifts every offset by 2; labels 26 and RB share a routine of their own (a scan for newlines and '/').
// Bytes at or past txt_len read as 0 (see acarsdec_amd.h, acg_oooi).
#include <hip/hip_runtime.h>
#include "acg_internal.h"
#include "acarsdec_amd.h"
#include "msg_keep.h"

#define LBL_WG 256
#define LBL_NG 7                // guards per label (44 has 7)
#define LBL_NC 6                // copies per label (Q1 has 6)

enum { F_da = 1, F_sa, F_eta, F_gout, F_gin, F_woff, F_won };     // oooi_t field index + 1 (0 ends a copy list)

struct LblGuard {
    unsigned char off, len;     // len 0 ends the list
    char alt[2][6];             // the bytes must equal alt[0] or (if not empty) alt[1]
};
struct LblCopy {
    unsigned char field, off;
};
struct LblEntry {
    char l0, l1;
    unsigned char scan26;       // 1: label 26's routine instead of the lists
    char opt[2];                // optional prefix: txt[0] == opt[0] requires txt[1] == opt[1] and shifts offsets by 2
    LblGuard g[LBL_NG];
    LblCopy c[LBL_NC];
};

#define G(off, s) {off, sizeof(s) - 1, {s, ""}}
#define G2(off, s, t) {off, sizeof(s) - 1, {s, t}}
#define C(f, off) {F_##f, off}
#define PLAIN 0, {0, 0}

// DecodeLabel()'s dispatch (label.c), one entry per label it decodes
__constant__ LblEntry k_labels[] = {
    {'1', '0', PLAIN, {G(0, "ARR01")}, {C(da, 12), C(eta, 16)}},
    {'1', '1', PLAIN, {G(13, "/DS "), G(21, "/ETA ")}, {C(da, 17), C(eta, 26)}},
    {'1', '2', PLAIN, {G(4, ",")}, {C(sa, 0), C(da, 5)}},
    {'1', '5', PLAIN, {G(0, "FST01")}, {C(sa, 5), C(da, 9)}},
    {'1', '7', PLAIN, {G(0, "ETA "), G(8, ","), G(13, ",")}, {C(eta, 4), C(sa, 9), C(da, 14)}},
    {'1', 'G', PLAIN, {G(4, ",")}, {C(sa, 0), C(da, 5)}},
    {'2', '0', PLAIN, {G(0, "RST")}, {C(sa, 22), C(da, 26)}},
    {'2', '1', PLAIN, {G(6, ","), G(11, ",")}, {C(sa, 7), C(da, 12)}},
    {'2', '6', 1, {0, 0}, {}, {}},
    {'2', 'N', PLAIN, {G(0, "TKO01"), G(11, "/")}, {C(sa, 20), C(da, 24)}},
    {'2', 'Z', PLAIN, {}, {C(da, 0)}},
    {'3', '3', PLAIN, {G(0, ","), G(20, ","), G(25, ",")}, {C(sa, 21), C(da, 26)}},
    {'3', '9', PLAIN, {G(0, "GTA01"), G(15, "/")}, {C(sa, 24), C(da, 28)}},
    {'4', '4', 0, {'0', '0'}, {G2(0, "POS0", "ETA0"), G2(4, "2", "3"), G(23, ","), G(28, ","), G(33, ","), G(38, ","), G(43, ",")},
     {C(da, 24), C(eta, 29), C(eta, 44)}},
    {'4', '5', PLAIN, {G(0, "A")}, {C(da, 1)}},
    {'8', '0', PLAIN, {G(6, "/DEST")}, {C(da, 12)}},                  // (only 5 bytes of "/DEST/" are compared)
    {'8', '3', PLAIN, {G(4, ",")}, {C(sa, 0), C(da, 5)}},
    {'8', 'D', PLAIN, {G(4, ","), G(35, ","), G(40, ",")}, {C(sa, 36), C(da, 41)}},
    {'8', 'E', PLAIN, {G(4, ",")}, {C(da, 0), C(eta, 5)}},
    {'8', 'S', PLAIN, {G(4, ",")}, {C(da, 0), C(eta, 5)}},
    {'R', 'B', 1, {0, 0}, {}, {}},                                     // label 26's decoder
    {'Q', '1', PLAIN, {}, {C(sa, 0), C(gout, 4), C(woff, 8), C(won, 12), C(gin, 16), C(da, 24)}},
    {'Q', '2', PLAIN, {}, {C(sa, 0), C(eta, 4)}},
    {'Q', 'A', PLAIN, {}, {C(sa, 0), C(gout, 4)}},
    {'Q', 'B', PLAIN, {}, {C(sa, 0), C(woff, 4)}},
    {'Q', 'C', PLAIN, {}, {C(sa, 0), C(won, 4)}},
    {'Q', 'D', PLAIN, {}, {C(sa, 0), C(gin, 4)}},
    {'Q', 'E', PLAIN, {}, {C(sa, 0), C(gout, 4), C(da, 8)}},
    {'Q', 'F', PLAIN, {}, {C(sa, 0), C(woff, 4), C(da, 8)}},
    {'Q', 'G', PLAIN, {}, {C(sa, 0), C(gout, 4), C(gin, 8)}},
    {'Q', 'H', PLAIN, {}, {C(sa, 0), C(gout, 4)}},
    {'Q', 'K', PLAIN, {}, {C(sa, 0), C(won, 4), C(da, 8)}},
    {'Q', 'L', PLAIN, {}, {C(da, 0), C(gin, 8), C(sa, 13)}},
    {'Q', 'M', PLAIN, {}, {C(da, 0), C(sa, 8)}},
    {'Q', 'N', PLAIN, {}, {C(da, 4), C(eta, 8)}},
    {'Q', 'P', PLAIN, {}, {C(sa, 0), C(da, 4), C(gout, 8)}},
    {'Q', 'Q', PLAIN, {}, {C(sa, 0), C(da, 4), C(woff, 8)}},
    {'Q', 'R', PLAIN, {}, {C(sa, 0), C(da, 4), C(won, 8)}},
    {'Q', 'S', PLAIN, {}, {C(sa, 0), C(da, 4), C(gin, 8)}},
    {'Q', 'T', PLAIN, {}, {C(sa, 0), C(da, 4), C(gout, 8), C(gin, 12)}},
};
#define NLABELS ((int)(sizeof(k_labels) / sizeof(k_labels[0])))

static_assert(sizeof(acg_oooi) == 40 && offsetof(acg_oooi, decoded) == 35, "acg_oooi layout (oooi_t + decoded + padding)");
static_assert(ACG_MSG_TXT == ACG_MSGTXTMAX, "text row");

// (the record's text view and the three keep predicates: msg_keep.h, shared with stats.hip)

__device__ __forceinline__ int find_byte(const Txt& t, int from, unsigned char c)   // strchr: stops at the first NUL
{
    for (int i = from; i <= ACG_MSG_TXT; ++i) {
        const unsigned char b = t(i);
        if (b == c) return i;
        if (b == 0) return -1;
    }
    return -1;
}

__device__ __forceinline__ bool equals_at(const Txt& t, int at, const char* s, int len)
{
    bool eq = true;
    for (int k = 0; k < len; ++k) eq &= t(at + k) == (unsigned char)s[k];
    return eq;
}

// label.c DecodeLabel() into o (40 bytes, zeroed here first)
__device__ void decode_label(const AcgMsgRec* r, unsigned char* o)
{
    for (int i = 0; i < 10; ++i) ((unsigned int*)o)[i] = 0u;
    const char l0 = r->label[0], l1 = r->label[1];
    int e = -1;
    for (int i = 0; i < NLABELS; ++i)
        if (k_labels[i].l0 == l0 && k_labels[i].l1 == l1) e = i;
    if (e < 0) return;
    const LblEntry& L = k_labels[e];
    const Txt t = rec_txt(r);
    // every field copy is (field, text position): collected first, written only if every check passes
    int cf[LBL_NC], cp[LBL_NC], nc = 0;
    if (L.scan26) {
        // VER/077 \n SCH/ ... / sa(4) . da(4) ... [\n ETA/ eta(4)]
        if (!equals_at(t, 0, "VER/077", 7)) return;
        int p = find_byte(t, 0, '\n');
        if (p < 0) return;
        ++p;
        if (!equals_at(t, p, "SCH/", 4)) return;
        p = find_byte(t, p + 4, '/');
        if (p < 0) return;
        cf[0] = F_sa; cp[0] = p + 1;
        cf[1] = F_da; cp[1] = p + 6;
        nc = 2;
        p = find_byte(t, p, '\n');
        if (p >= 0) {
            ++p;
            if (!equals_at(t, p, "ETA/", 4)) return;
            cf[2] = F_eta; cp[2] = p + 4;
            nc = 3;
        }
    } else {
        int base = 0;
        if (L.opt[0] && t(0) == (unsigned char)L.opt[0]) {
            if (t(1) != (unsigned char)L.opt[1]) return;
            base = 2;
        }
        for (int g = 0; g < LBL_NG && L.g[g].len; ++g) {
            const LblGuard& G_ = L.g[g];
            const bool a0 = equals_at(t, base + G_.off, G_.alt[0], G_.len);
            const bool a1 = G_.alt[1][0] && equals_at(t, base + G_.off, G_.alt[1], G_.len);
            if (!a0 && !a1) return;
        }
        for (int c = 0; c < LBL_NC && L.c[c].field; ++c) {
            cf[nc] = L.c[c].field;
            cp[nc] = base + L.c[c].off;
            ++nc;
        }
    }
    for (int c = 0; c < nc; ++c) {
        unsigned char* d = o + 5 * (cf[c] - 1);
        for (int k = 0; k < 4; ++k) d[k] = t(cp[c] + k);
    }
    o[35] = 1;                                                          // decoded
}

__global__ __launch_bounds__(LBL_WG) void msg_keep_count_kernel(const AcgMsgRec* recs, unsigned int n, AcgLabelFilter f,
                                                                unsigned int* wg_count)
{
    const unsigned int i = blockIdx.x * LBL_WG + threadIdx.x;
    const int k = i < n && msg_keep(recs + i, f);
    const int c = __syncthreads_count(k);
    if (threadIdx.x == 0) wg_count[blockIdx.x] = (unsigned int)c;
}

__global__ __launch_bounds__(LBL_WG) void msg_compact_kernel(const AcgMsgRec* recs, unsigned int n, AcgLabelFilter f,
                                                             const unsigned int* wg_count, AcgMsgRec* out, acg_oooi* oooi,
                                                             unsigned int* total, unsigned char* keep_out)
{
    __shared__ unsigned int base_s;
    __shared__ unsigned int wave_n[LBL_WG / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) base_s = 0;
    __syncthreads();
    unsigned int s = 0;
    for (unsigned int j = threadIdx.x; j < blockIdx.x; j += LBL_WG) s += wg_count[j];
    if (s) atomicAdd(&base_s, s);
    const unsigned int i = blockIdx.x * LBL_WG + threadIdx.x;
    const bool k = i < n && msg_keep(recs + i, f);
    const unsigned long long m = __ballot(k);
    if (lane == 0) wave_n[wv] = (unsigned int)__popcll(m);
    __syncthreads();
    unsigned int pos = base_s + (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wv; ++w) pos += wave_n[w];
    if (k) {
        const uint4* src = (const uint4*)(recs + i);
        uint4* dst = (uint4*)(out + pos);
#pragma unroll
        for (int q = 0; q < (int)(sizeof(AcgMsgRec) / 16); ++q) dst[q] = src[q];
        decode_label(recs + i, (unsigned char*)(oooi + pos));
    }
    if (keep_out && i < n) keep_out[i] = k ? 1 : 0;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        unsigned int t = base_s;
        for (int w = 0; w < LBL_WG / 64; ++w) t += wave_n[w];
        *total = t;
    }
}

// The flight table's event extraction (flight.hip does the rest): a thread per record.  A record reaches addFlight() when it
// passed -A / -b and is a downlink with bs != 0x03 (output.c:545-567,647); -e is tested after addFlight() and only noted here.
// The events are compacted as they are found (a counter, one atomic per wave; their order does not matter: the time sort's keys
// (end_sample, chn) are distinct).  tv = t0 + soh_sample / 12500 s in integers: a sample is exactly 80 us.
__global__ __launch_bounds__(LBL_WG) void flight_extract_kernel(const AcgMsgRec* recs, unsigned int n, AcgLabelFilter f, AcgFlightPass p)
{
    const unsigned int i = blockIdx.x * LBL_WG + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const AcgMsgRec* r = recs + i;
    const bool ev = i < n && msg_keep_ab(r, f) && r->down && r->bs != 0x03;
    const unsigned long long m = __ballot(ev);
    if (!m) return;
    unsigned int base = 0;
    if (lane == 0) base = atomicAdd(&p.st->m, (unsigned int)__popcll(m));
    base = (unsigned int)__shfl((int)base, 0);
    if (!ev) return;
    const unsigned int at = base + (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
    AcgFlightEv* e = p.ev + at;
    unsigned long long a = 0;
    for (int b = 0; b < 7; ++b) a |= (unsigned long long)(unsigned char)r->addr[b] << (8 * b);
    for (int b = 1; b < 7; ++b)                                          // a C string: nothing behind its NUL counts
        if (((a >> (8 * (b - 1))) & 0xff) == 0) a &= (1ull << (8 * b)) - 1ull;
    unsigned long long fid = 0;
    for (int b = 0; b < 7; ++b) fid |= (unsigned long long)(unsigned char)r->fid[b] << (8 * b);
    for (int b = 1; b < 7; ++b)
        if (((fid >> (8 * (b - 1))) & 0xff) == 0) fid &= (1ull << (8 * b)) - 1ull;
    const long long soh = r->end_sample - (long long)r->soh_back;
    const long long us = (long long)p.t0_usec + soh * 80ll;
    long long q = us / 1000000ll, rem = us % 1000000ll;
    if (rem < 0) { rem += 1000000ll; --q; }
    e->key = a | (1ull << 63);
    e->soh_sample = soh;
    e->sec = p.t0_sec + q;
    e->usec = (int)rem;
    // the number the table records for this channel (acg_flights_set_channels: a shard's channels under their global numbers)
    const int chn = p.chmap && (unsigned int)r->chn < p.nmap ? p.chmap[r->chn] : r->chn;
    e->chn = chn;
    e->fid = fid;
    decode_label(r, e->oooi);
    e->e_ok = msg_keep_e(r, f) ? 1u : 0u;
    e->pad_ = 0u;
    p.key1[at] = (((unsigned long long)r->end_sample & ((1ull << 43) - 1ull)) << 20) | ((unsigned long long)(unsigned int)chn & 0xfffffull);
    p.idx1[at] = at;
}

extern "C" int acg_launch_flight_extract(const AcgMsgRec* recs, unsigned int n, const AcgLabelFilter* f, const AcgFlightPass* p, void* stream)
{
    hipLaunchKernelGGL(flight_extract_kernel, dim3((n + LBL_WG - 1) / LBL_WG), dim3(LBL_WG), 0, (hipStream_t)stream, recs, n, *f, *p);
    return (int)hipGetLastError();
}

extern "C" int acg_launch_msg_labels(const AcgMsgRec* recs, unsigned int n, const AcgLabelPass* p, void* stream)
{
    if (n == 0) return 0;
    const unsigned int g = (n + LBL_WG - 1) / LBL_WG;
    hipLaunchKernelGGL(msg_keep_count_kernel, dim3(g), dim3(LBL_WG), 0, (hipStream_t)stream, recs, n, *p->f, p->wg_count);
    hipLaunchKernelGGL(msg_compact_kernel, dim3(g), dim3(LBL_WG), 0, (hipStream_t)stream, recs, n, *p->f, (const unsigned int*)p->wg_count,
                       p->kept, (acg_oooi*)p->oooi, p->total, p->keep_out);
    const int e = (int)hipGetLastError();
    if (e || !p->flights) return e;
    return acg_launch_flight_pass(recs, n, p->f, p->flights, stream);
}
