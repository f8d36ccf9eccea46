// flight_text.hip -- the two outputs of outputmsg() that print from the flight table (flight.hip), rendered on the device like
// the per-message formats of json.hip and text.hip:
//   the monitor screen  printmonitor()  output.c:458-484   what -o 3 prints per kept message: cls(), the title with printtime(tv),
//                                                          the column header, one row per live entry, latest update first;
//   the route line      routejson()     output.c:428-456   what -o 5 prints once per entry: {"timestamp":T[,"station_id":".."],
//                                                          "flight":"..","depa":"..","dsta":".."} and '\n' (cJSON, fmt = 0).
// What leaves is text: the frame's bytes, or the queued routes' lines packed back to back, and four counters.
//
// THE MONITOR PASS, behind flight.hip's flight_snapkeys_kernel + flight_sort_kernel (the live slots in snapshot order):
//   flight_text_mon_measure_kernel   one WAVE per row, the waves looping: the row's length (70 while nbm <= 999: "%3d" grows);
//   flight_text_sum_kernel / flight_text_offsets_kernel   sink_pack.h's exclusive scan of the lengths: every row's offset behind
//                                    the header, the frame's bytes and rows;
//   flight_text_mon_render_kernel    one wave per row: the slot (30 dwords) into LDS, the row assembled in a per-wave LDS row,
//                                    flushed seam-safe; wave 0 of workgroup 0 writes the header first, and the table's `dropped`
//                                    beside the scan's two counters.
// THE ROUTE PASS: flight_text_route_keys_kernel (AcgRouteRec::order, the (pass, rank) tag of the triggering message),
// flight.hip's sort (acg_launch_sort_pairs), flight_text_route_measure_kernel, the same scan, flight_text_route_render_kernel.
//
// House style as json.hip / text.hip: lane j computes character j (flight_text_num.h, text_num.h, json_num.h); a C string's end
// is a ballot and a find-first; "%-8s", "%-7s", "%4s" and "%3d" pad and never cut; measure and render run the SAME function
// (ft_row / ft_line <false / true>); no scratch, no per-byte global traffic of whole records.  sink_pack.h's pieces are used as
// they are (PkLit, pk_sum, pk_offsets, pk_flush_row).  Its pk_measure / pk_render are written over AcgSinkPass and a message
// record, so this unit has loop bodies and a launch sequence of its own.  The row writers and the escape's rules (cJSON.c:858-877) are the
// sinks' own, sink_put.h; what only the monitor row uses ("%-Ns", the OOOI field, printtime()) is here and stores through pk_st,
// and so is the one round a route's short strings need (ft_str_json, over the shared classes and escaped byte).
#include "sink_put.h"
#include "flight_text_num.h"

#define FT_ROW_BUF 128                      // a wave's LDS row: the monitor's header (110) and its rows (<= 78)
#define FT_LINE_BUF 384                     // ... and a route line (<= 363)
#define FT_MAX_WG 1024                      // workgroups of a measure / render launch: the waves loop over the ranks

static_assert(ACG_FT_ROW_MAX == ACG_MONITOR_ROW_MAX && ACG_FT_LINE_MAX == ACG_ROUTE_LINE_MAX && ACG_FT_HDR_LEN == ACG_MONITOR_HDR_LEN, "record bounds");
static_assert(ACG_FT_ROW_MAX <= FT_ROW_BUF && ACG_FT_HDR_LEN <= FT_ROW_BUF && ACG_FT_LINE_MAX <= FT_LINE_BUF, "row buffers");
static_assert(sizeof(AcgFlightSlot) == 120 && sizeof(AcgRouteRec) == 64 && offsetof(AcgFlightSlot, fld) == 92 && offsetof(AcgFlightSlot, fid) == 16, "layouts");

#define FT_LIT(s) PK_PUT_LIT(B, s)

// "%-<width>s": left-justified to at least width, never cut
template <bool W, unsigned int B>
__device__ __forceinline__ unsigned int ft_str_left(unsigned char* row, unsigned int pos, const unsigned char* s, int maxlen, int width, int lane)
{
    unsigned int b;
    const int n = pk_strlen(s, maxlen, lane, &b);
    const int pad = width > n ? width - n : 0;
    if (W) {
        if (lane < n) pk_st<W, B>(row, pos + lane, (unsigned char)b);
        if (lane < pad) pk_st<W, B>(row, pos + n + lane, ' ');
    }
    return pos + (unsigned int)(n + pad);
}

// " %4s " of an OOOI field (4 characters, the fifth is always NUL), or six spaces when its first byte is NUL (output.c:475-477)
template <bool W, unsigned int B>
__device__ __forceinline__ unsigned int ft_field(unsigned char* row, unsigned int pos, const unsigned char* s, int lane)
{
    unsigned int b;
    const int n = pk_strlen(s, 4, lane, &b);
    const int j = lane - (5 - n);                                  // place `lane` of the six shows the string's byte j: 5 - n spaces in front
    if (W && lane < 6) pk_st<W, B>(row, pos + lane, (unsigned char)(j >= 0 && j < n ? s[j] : ' '));
    return pos + 6;
}

// printtime(): "hh:mm:ss.mmm"
template <bool W, unsigned int B>
__device__ __forceinline__ unsigned int ft_time(unsigned char* row, unsigned int pos, long long sec, int usec, int lane)
{
    const TnDate d = tn_date(sec, usec);
    if (W && lane < FTN_TIME_LEN) pk_st<W, B>(row, pos + lane, ftn_time_char(d, lane));
    return pos + FTN_TIME_LEN;
}

// One row.  S: the slot (LDS); row: where the row's first byte goes (W) or unused.  output.c:471-478
template <bool W>
__device__ __forceinline__ unsigned int ft_row(const unsigned char* S, unsigned char* row, int nbch, int lane)
{
    constexpr unsigned int B = ACG_FT_ROW_MAX;
    const AcgFlightSlot* s = (const AcgFlightSlot*)S;
    unsigned int pos = 0;
    pos = pk_fill<W, B>(row, pos, ' ', 1, lane);
    pos = ft_str_left<W, B>(row, pos, S + offsetof(AcgFlightSlot, key), 7, 8, lane);      // " %-8s": the key's low 7 bytes are the addr
    pos = pk_fill<W, B>(row, pos, ' ', 1, lane);
    pos = ft_str_left<W, B>(row, pos, S + offsetof(AcgFlightSlot, fid), 7, 7, lane);      // " %-7s"
    pos = pk_fill<W, B>(row, pos, ' ', 1, lane);
    const FtnInt3 nb = ftn_int3(s->nbm);                                                  // " %3d "
    if (W && lane < nb.len) pk_st<W, B>(row, pos + lane, ftn_int3_char(nb, lane));
    pos += (unsigned int)nb.len;
    pos = pk_fill<W, B>(row, pos, ' ', 1, lane);
    const unsigned int chm = (unsigned int)s->chm;                                       // output.c:472-473: nbch columns, padded to 16
    if (W && lane < 16) pk_st<W, B>(row, pos + lane, (unsigned char)(lane >= nbch ? ' ' : ((chm >> lane) & 1u) ? 'x' : '.'));
    pos += 16;
    pos = pk_fill<W, B>(row, pos, ' ', 1, lane);
    pos = ft_time<W, B>(row, pos, s->ts_sec, s->ts_usec, lane);
    const unsigned char* f = S + offsetof(AcgFlightSlot, fld);                            // da sa eta ...: the screen shows sa, da, eta
    pos = ft_field<W, B>(row, pos, f + 4, lane);
    pos = ft_field<W, B>(row, pos, f + 0, lane);
    pos = ft_field<W, B>(row, pos, f + 8, lane);
    pos = pk_fill<W, B>(row, pos, '\n', 1, lane);
    return pos;
}

// The header: cls(), the title, printtime(tv), the column line (output.c:462-465)
__device__ __forceinline__ unsigned int ft_header(unsigned char* row, long long sec, int usec, int lane)
{
    constexpr bool W = true;
    constexpr unsigned int B = ACG_FT_HDR_LEN;
    unsigned int pos = 0;
    FT_LIT("\x1b[H\x1b[2J");
    FT_LIT("             Acarsdec monitor ");
    pos = ft_time<W, B>(row, pos, sec, usec, lane);
    FT_LIT("\n Aircraft Flight   Nb Channels     First    DEP   ARR   ETA\n");
    return pos;
}

// "<C string at s, at most maxlen < 64 bytes>" escaped: pk_put_str's one round over the shared length, classes and escaped byte,
// without pk_put_round's "no NUL among the 64 lanes" case (with pk_put_str the route pass over 16 384 routes measured 0.295-0.296 ms
// against the parent's 0.293-0.295 in two sessions, outside its run-to-run range; this spelling 0.294: LEDGER)
template <bool W, unsigned int B>
__device__ __forceinline__ unsigned int ft_str_json(unsigned char* row, unsigned int pos, const unsigned char* s, int maxlen, int lane)
{
    unsigned int b;
    const int n = pk_strlen(s, maxlen, lane, &b);
    const bool live = lane < n;
    const bool two = live && pk_two(b), six = live && b < 32u && !two;
    const unsigned long long m2 = __ballot(two), m6 = __ballot(six), below = (1ull << lane) - 1ull;
    const unsigned int esc = (unsigned int)n + (unsigned int)__popcll(m2) + 5u * (unsigned int)__popcll(m6);
    if (lane == 0) pk_st<W, B>(row, pos, '"');
    if (live) pk_put_escaped<W, B>(row, pos + 1 + (unsigned int)lane + (unsigned int)__popcll(m2 & below) + 5u * (unsigned int)__popcll(m6 & below), b, two, six);
    if (lane == 0) pk_st<W, B>(row, pos + 1 + esc, '"');
    return pos + esc + 2;
}

// One line.  R: the AcgRouteRec (LDS); row: where the line's first byte goes (W) or unused.  output.c:442-447,680
template <bool W>
__device__ __forceinline__ unsigned int ft_line(const unsigned char* R, unsigned char* row, const AcgFlightTextDev* cfg, int lane)
{
    constexpr unsigned int B = ACG_FT_LINE_MAX;
    const unsigned char* r = R + offsetof(AcgRouteRec, r);
    unsigned int pos = 0;
    FT_LIT("{\"timestamp\":");
    pos = pk_put_tok<W, B>(row, pos, jn_timestamp(*(const long long*)(r + offsetof(acg_route, sec)), *(const int*)(r + offsetof(acg_route, usec))), lane);
    const unsigned int pre_len = cfg->pre_len > ACG_JS_PRE_MAX ? ACG_JS_PRE_MAX : cfg->pre_len;
    pos = pk_put_words<W, B>(row, pos, cfg->pre, pre_len, lane);                         // ,"station_id":".." or nothing
    FT_LIT(",\"flight\":");
    pos = ft_str_json<W, B>(row, pos, r + offsetof(acg_route, fid), 7, lane);
    FT_LIT(",\"depa\":");
    pos = ft_str_json<W, B>(row, pos, r + offsetof(acg_route, sa), 4, lane);
    FT_LIT(",\"dsta\":");
    pos = ft_str_json<W, B>(row, pos, r + offsetof(acg_route, da), 4, lane);
    FT_LIT("}\n");
    return pos;
}

// nd dwords at src into the wave's LDS record
__device__ __forceinline__ void ft_load(unsigned char* R, const void* src, int nd, int lane)
{
    // (LDS operations of one wave execute in order; the fences keep the compiler from moving them across each other, also across
    //  the turns of a wave's loop over its ranks)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < nd) ((unsigned int*)R)[lane] = ((const unsigned int*)src)[lane];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ unsigned int ft_total(const AcgFlightTextPass& p)
{
    const unsigned int t = *p.total;
    return t < p.nmax ? t : p.nmax;
}

// the wave's row to its place: bounds, then the seam-safe flush
__device__ __forceinline__ void ft_flush(const AcgFlightTextPass& p, const unsigned char* rowbuf, unsigned int off, unsigned int len, int lane)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    pk_flush_row(rowbuf, p.out, off, len, lane);
}

// ---- the monitor pass ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * PK_WAVES) void flight_text_mon_measure_kernel(AcgFlightTextPass p)
{
    __shared__ __attribute__((aligned(16))) unsigned char recs[PK_WAVES][128];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned int total = ft_total(p);
    const int nbch = p.cfg->nbch;
    for (unsigned int r = blockIdx.x * PK_WAVES + wv; r < total; r += gridDim.x * PK_WAVES) {      // (wave-uniform)
        ft_load(recs[wv], p.slots + p.idx_s[r], (int)(sizeof(AcgFlightSlot) / 4), lane);
        const unsigned int n = ft_row<false>(recs[wv], nullptr, nbch, lane);
        if (lane == 0) p.len[r] = n > ACG_FT_ROW_MAX ? ACG_FT_ROW_MAX : n;
    }
}

__global__ __launch_bounds__(64 * PK_WAVES) void flight_text_mon_render_kernel(AcgFlightTextPass p)
{
    __shared__ __attribute__((aligned(16))) unsigned char recs[PK_WAVES][128];
    __shared__ __attribute__((aligned(16))) unsigned char rows[PK_WAVES][FT_ROW_BUF + 16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned int total = ft_total(p);
    const int nbch = p.cfg->nbch;
    if (blockIdx.x == 0 && wv == 0 && p.base == ACG_FT_HDR_LEN && p.out_cap >= ACG_FT_HDR_LEN) {
        // the header's tv: the caller's message, or the newest live entry's tl, or (an empty table) t0
        long long sec = p.t0_sec;
        int usec = p.t0_usec;
        if (p.hdr_soh >= 0) {
            const long long us = (long long)p.t0_usec + p.hdr_soh * 80ll;
            sec = p.t0_sec + us / 1000000ll;
            usec = (int)(us % 1000000ll);
        } else if (total) {
            const AcgFlightSlot* s = p.slots + p.idx_s[0];
            sec = s->tl_sec;
            usec = s->tl_usec;
        }
        const unsigned int n = ft_header(rows[0], sec, usec, lane);                      // (offset 0: the row starts at its buffer's start)
        if (n == ACG_FT_HDR_LEN) ft_flush(p, rows[0], 0u, n, lane);
        if (lane == 0) p.counters[2] = p.st->dropped;
    }
    for (unsigned int r = blockIdx.x * PK_WAVES + wv; r < total; r += gridDim.x * PK_WAVES) {
        const unsigned int len = p.len[r], off = p.base + p.off[r];
        if (len == 0 || len > ACG_FT_ROW_MAX || off < p.base || off > p.out_cap || len > p.out_cap - off) continue;
        ft_load(recs[wv], p.slots + p.idx_s[r], (int)(sizeof(AcgFlightSlot) / 4), lane);
        const unsigned int n = ft_row<true>(recs[wv], rows[wv] + (off & 15u), nbch, lane);
        if (n != len) continue;                                                          // (cannot happen: one function measures and renders)
        ft_flush(p, rows[wv], off, len, lane);
    }
}

// ---- the route pass -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PK_WG) void flight_text_route_keys_kernel(AcgFlightTextPass p)
{
    const unsigned int i = blockIdx.x * PK_WG + threadIdx.x;
    if (i == 0) p.counters[3] = p.nmax;                                                  // the lines of this pass: what *p.total reads
    if (i >= p.nmax) return;
    p.key[i] = p.routes[i].order;
    p.idx[i] = i;
}

__global__ __launch_bounds__(64 * PK_WAVES) void flight_text_route_measure_kernel(AcgFlightTextPass p)
{
    __shared__ __attribute__((aligned(16))) unsigned char recs[PK_WAVES][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned int total = ft_total(p);
    for (unsigned int r = blockIdx.x * PK_WAVES + wv; r < total; r += gridDim.x * PK_WAVES) {
        const unsigned int i = p.idx_s[r];
        if (i >= p.nmax) { if (lane == 0) p.len[r] = 0; continue; }
        ft_load(recs[wv], p.routes + i, (int)(sizeof(AcgRouteRec) / 4), lane);
        const unsigned int n = ft_line<false>(recs[wv], nullptr, p.cfg, lane);
        if (lane == 0) p.len[r] = n > ACG_FT_LINE_MAX ? ACG_FT_LINE_MAX : n;
    }
}

__global__ __launch_bounds__(64 * PK_WAVES) void flight_text_route_render_kernel(AcgFlightTextPass p)
{
    __shared__ __attribute__((aligned(16))) unsigned char recs[PK_WAVES][64];
    __shared__ __attribute__((aligned(16))) unsigned char rows[PK_WAVES][FT_LINE_BUF + 16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned int total = ft_total(p);
    for (unsigned int r = blockIdx.x * PK_WAVES + wv; r < total; r += gridDim.x * PK_WAVES) {
        const unsigned int len = p.len[r], off = p.base + p.off[r], i = p.idx_s[r];
        if (i >= p.nmax || len == 0 || len > ACG_FT_LINE_MAX || off < p.base || off > p.out_cap || len > p.out_cap - off) continue;
        ft_load(recs[wv], p.routes + i, (int)(sizeof(AcgRouteRec) / 4), lane);
        const unsigned int n = ft_line<true>(recs[wv], rows[wv] + (off & 15u), p.cfg, lane);
        if (n != len) continue;
        ft_flush(p, rows[wv], off, len, lane);
    }
}

// ---- the scan (sink_pack.h), shared by both passes ------------------------------------------------------------------------------
__global__ __launch_bounds__(PK_WG) void flight_text_sum_kernel(AcgFlightTextPass p)
{
    __shared__ unsigned int sum_s;
    pk_sum(&sum_s, p.len, p.wg_sum, p.wg_cnt, p.nmax, p.total);
}

__global__ __launch_bounds__(PK_WG) void flight_text_offsets_kernel(AcgFlightTextPass p)
{
    __shared__ unsigned int base_s, cnt_s;
    __shared__ unsigned int wave_n[PK_WG / 64];
    pk_offsets(&base_s, &cnt_s, wave_n, p.len, p.off, p.wg_sum, p.wg_cnt, p.counters, p.nmax, p.total);
}

static unsigned int ft_wave_grid(unsigned int n)
{
    const unsigned int g = (n + PK_WAVES - 1) / PK_WAVES;
    return g < 1 ? 1 : g > FT_MAX_WG ? FT_MAX_WG : g;
}

static int ft_measure_scan_render(const AcgFlightTextPass* p, hipStream_t s, void (*measure)(AcgFlightTextPass), void (*render)(AcgFlightTextPass))
{
    const unsigned int g = (p->nmax + PK_WG - 1) / PK_WG, gw = ft_wave_grid(p->nmax);
    hipLaunchKernelGGL(measure, dim3(gw), dim3(64 * PK_WAVES), 0, s, *p);
    hipLaunchKernelGGL(flight_text_sum_kernel, dim3(g), dim3(PK_WG), 0, s, *p);
    hipLaunchKernelGGL(flight_text_offsets_kernel, dim3(g), dim3(PK_WG), 0, s, *p);
    hipLaunchKernelGGL(render, dim3(gw), dim3(64 * PK_WAVES), 0, s, *p);
    return (int)hipGetLastError();
}

extern "C" int acg_launch_flight_monitor_text(const AcgFlightTextPass* p, void* stream)
{
    if (p->nmax == 0) return (int)hipErrorInvalidValue;                                   // (a table has at least one slot)
    return ft_measure_scan_render(p, (hipStream_t)stream, flight_text_mon_measure_kernel, flight_text_mon_render_kernel);
}

extern "C" int acg_launch_flight_route_text(const AcgFlightTextPass* p, unsigned int n, void* stream)
{
    if (n == 0 || n != p->nmax) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(flight_text_route_keys_kernel, dim3((n + PK_WG - 1) / PK_WG), dim3(PK_WG), 0, (hipStream_t)stream, *p);
    const int e = acg_launch_sort_pairs(p->key, p->idx, p->key_s, p->idx_s, nullptr, n, stream);
    if (e) return e;
    return ft_measure_scan_render(p, (hipStream_t)stream, flight_text_route_measure_kernel, flight_text_route_render_kernel);
}
