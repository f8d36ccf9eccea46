// json.hip -- the last step of outputmsg() for the batch sink: buildjson() + cJSON_PrintPreallocated(.., fmt = 0)
// (output.c:227-324, cJSON.c print_object / print_string_ptr / print_number) for the build without libacars, over the records
// label.hip kept and compacted for one drain / collect.  What leaves is what `-o 4` prints: one JSON object per message, each
// ended by '\n', packed back to back in (chn, end_bit) order; the host copies bytes and two counters, no records.
//
// This unit's two kernels, launched by outs.hip's sequence (acg_launch_outs: keys, sort, measure, scan, render -- the JSON sink
// is that sequence with one leg) through acg_launch_json_sorted, on the stream of the label pass they hang on:
//   json_measure_kernel  one WAVE per record, in sorted order: the line's length.  The escape class of every string byte is
//                        decided by the lanes in parallel (the text: four rounds of 64 lanes), a C string's end is a ballot and a
//                        find-first, the length is popcounts;
//   json_render_kernel   one wave per record: the line assembled in a per-wave LDS row, then stored to the packed offset the
//                        scan between the two gave it.
//
// A string byte's place in the line is its index + the two-character escapes before it + 5 x the \u00xx escapes before it: two
// ballots and two popcounts, never a lane walking the text.  Numbers are integer arithmetic (json_num.h): lane j computes the
// j-th character of a token.  Measure and render run the SAME function (json_line<false / true>): the length a line was given
// room for is the length it is rendered with.
//
// THE SEAM, the record load, the level's float and the bodies of the measure / render kernels are shared with the text renderer
// (text.hip): sink_pack.h.  The row writers (bounded store, literal, number token, dword copy, the string escape) are shared with
// text.hip and flight_text.hip: sink_put.h.  This unit supplies json_line and keeps its two kernels as wrappers.
//
// No scratch (no indexed private array: a record's fields are read out of LDS, digits are computed, not stored), no per-byte
// global traffic (a record comes in as 80 + 10 dword loads, the constant stretches as dwords, a line leaves as 16-byte stores and < 30 byte stores), two
// independent waves per workgroup (2 x 2 944 B of LDS): these passes run beside a down-converter that saturates HBM.
#include "sink_put.h"

static_assert(ACG_JS_LINE_MAX == ACG_JSON_LINE_MAX && ACG_JS_LINE_MAX % 64 == 0, "line bound");

#define PUT_LIT(s) PK_PUT_LIT(B, s)

// One line.  R: the record and, at R + 320, its acg_oooi (LDS); row: where the line's first byte goes (W) or unused.
template <bool W>
__device__ __forceinline__ unsigned int json_line(const unsigned char* R, unsigned char* row, const AcgSinkPass& p, int lane, bool* near_mid)
{
    constexpr unsigned int B = ACG_JS_LINE_MAX;
    const AcgMsgRec* r = (const AcgMsgRec*)R;
    const AcgJsonDev* cfg = (const AcgJsonDev*)p.cfg;
    unsigned int pos = 0;
    // ---- "timestamp": tv = t0 + soh_sample / 12500 s in integers (a sample is exactly 80 us), as flight_extract_kernel
    const long long soh = r->end_sample - (long long)r->soh_back;
    const long long us = (long long)cfg->t0_usec + soh * 80ll;
    long long q = us / 1000000ll, rem = us % 1000000ll;
    if (rem < 0) { rem += 1000000ll; --q; }
    PUT_LIT("{\"timestamp\":");
    pos = pk_put_tok<W, B>(row, pos, jn_timestamp(cfg->t0_sec + q, (int)rem), lane);
    pos = pk_put_words<W, B>(row, pos, cfg->pre, cfg->pre_len, lane);                   // ,"station_id":".." or nothing
    const int chn = r->chn;                                                      // the slot: the frequency token's index
    PUT_LIT(",\"channel\":");
    pos = pk_put_tok<W, B>(row, pos, jn_int(pk_chn(p, chn)), lane);                   // the number handed out (acg_set_channel_numbers)
    PUT_LIT(",\"freq\":");
    if ((unsigned int)chn < (unsigned int)cfg->nch) {
        const unsigned long long ft = ((const unsigned long long*)p.freq)[chn];    // 7 characters and their count: one load
        const unsigned int fn = (unsigned int)(ft >> 56) & 7u;
        if (W && (unsigned int)lane < fn) pk_st<W, B>(row, pos + lane, (unsigned char)(ft >> (8 * lane)));
        pos += fn;
    } else {
        PUT_LIT("0.000");
    }
    // ---- "level": the float of acars.c:351, then "%2.1f" cut to 7 characters (json_num.h)
    const float lvl = pk_level(r, p.lvl_from_rec, near_mid);
    PUT_LIT(",\"level\":");
    pos = pk_put_tok<W, B>(row, pos, jn_level(lvl), lane);
    PUT_LIT(",\"error\":");
    pos = pk_put_tok<W, B>(row, pos, jn_int(r->err), lane);
    PUT_LIT(",\"mode\":");
    pos = pk_put_str<W, B>(row, pos, R + offsetof(AcgMsgRec, mode), 1, lane);           // "%c": a NUL gives ""
    PUT_LIT(",\"label\":");
    pos = pk_put_str<W, B>(row, pos, R + offsetof(AcgMsgRec, label), 2, lane);
    const char bid = r->bid;
    if (bid) {
        PUT_LIT(",\"block_id\":");
        pos = pk_put_str<W, B>(row, pos, R + offsetof(AcgMsgRec, bid), 1, lane);
        if (r->ack == '!') {
            PUT_LIT(",\"ack\":false");
        } else {
            PUT_LIT(",\"ack\":");
            pos = pk_put_str<W, B>(row, pos, R + offsetof(AcgMsgRec, ack), 1, lane);
        }
        PUT_LIT(",\"tail\":");
        pos = pk_put_str<W, B>(row, pos, R + offsetof(AcgMsgRec, addr), 7, lane);
        if (bid >= '0' && bid <= '9') {                                          // IS_DOWNLINK_BLK, output.c:31,269
            PUT_LIT(",\"flight\":");
            pos = pk_put_str<W, B>(row, pos, R + offsetof(AcgMsgRec, fid), 6, lane);
            PUT_LIT(",\"msgno\":");
            pos = pk_put_str<W, B>(row, pos, R + offsetof(AcgMsgRec, no), 4, lane);
        }
    }
    // ---- "text": a C string within txt_len bytes, four rounds of 64 lanes
    int tl = r->txt_len;
    tl = tl < 0 ? 0 : tl > ACG_MSG_TXT ? ACG_MSG_TXT : tl;
    const unsigned char* txt = R + offsetof(AcgMsgRec, txt);
    if (tl > 0 && txt[0]) {
        PUT_LIT(",\"text\":\"");
        for (int rd = 0; rd < 4; ++rd) {
            const int i = 64 * rd + lane;
            const unsigned int b = i < tl ? txt[i] : 0u;
            bool more;
            pos += pk_put_round<W, B>(row, pos, b, lane, &more);
            if (!more) break;                                                    // (wave-uniform)
        }
        PUT_LIT("\"");
    }
    if (r->be == 0x17) PUT_LIT(",\"end\":true");
    // ---- the OOOI keys in buildjson's order (output.c:280-295): sa da eta gout gin woff won of {da sa eta gout gin woff won}
    const unsigned char* O = R + sizeof(AcgMsgRec);
    if (O[35]) {
        if (O[5]) { PUT_LIT(",\"depa\":"); pos = pk_put_str<W, B>(row, pos, O + 5, 4, lane); }
        if (O[0]) { PUT_LIT(",\"dsta\":"); pos = pk_put_str<W, B>(row, pos, O + 0, 4, lane); }
        if (O[10]) { PUT_LIT(",\"eta\":"); pos = pk_put_str<W, B>(row, pos, O + 10, 4, lane); }
        if (O[15]) { PUT_LIT(",\"gtout\":"); pos = pk_put_str<W, B>(row, pos, O + 15, 4, lane); }
        if (O[20]) { PUT_LIT(",\"gtin\":"); pos = pk_put_str<W, B>(row, pos, O + 20, 4, lane); }
        if (O[25]) { PUT_LIT(",\"wloff\":"); pos = pk_put_str<W, B>(row, pos, O + 25, 4, lane); }
        if (O[30]) { PUT_LIT(",\"wlin\":"); pos = pk_put_str<W, B>(row, pos, O + 30, 4, lane); }
    }
    pos = pk_put_words<W, B>(row, pos, cfg->post, cfg->post_len, lane);                 // ,"app":{"name":"..","ver":".."}}\n
    return pos;
}

// what this unit gives the passes' skeleton (sink_pack.h)
struct JsonFmt {
    static constexpr unsigned int REC_MAX = ACG_JS_LINE_MAX;
    template <bool W>
    static __device__ __forceinline__ unsigned int record(const unsigned char* R, unsigned char* row, const AcgSinkPass& p, int lane, bool* near_mid)
    {
        return json_line<W>(R, row, p, lane, near_mid);
    }
    static __device__ __forceinline__ unsigned char* row_at(unsigned char (*rows)[REC_MAX + 16], int wv, unsigned int off)
    {
        const unsigned int a = off & 15u;                         // the row mirrors the output's alignment (written in this order: sink_pack.h)
        return rows[wv] + a;
    }
};

// the passes (sink_pack.h): the kernels and their LDS are this unit's own
__global__ __launch_bounds__(64 * PK_WAVES) void json_measure_kernel(AcgSinkPass p)
{
    __shared__ __attribute__((aligned(16))) unsigned char recs[PK_WAVES][PK_REC];
    const unsigned int r = blockIdx.x * PK_WAVES + (threadIdx.x >> 6);        // wave-uniform
    if (r >= p.nmax || r >= *p.total) return;                                    // (the early-outs are the kernel's: sink_pack.h, pk_measure)
    if (p.key_s[r] == ~0ull) {
        if ((threadIdx.x & 63) == 0) p.len[r] = 0;
        return;
    }
    pk_measure<JsonFmt>(recs, p, r);
}

__global__ __launch_bounds__(64 * PK_WAVES) void json_render_kernel(AcgSinkPass p)
{
    __shared__ __attribute__((aligned(16))) unsigned char recs[PK_WAVES][PK_REC];
    __shared__ __attribute__((aligned(16))) unsigned char rows[PK_WAVES][JsonFmt::REC_MAX + 16];
    pk_render<JsonFmt>(recs, rows, p);
}

extern "C" int acg_launch_json_sorted(const AcgSinkPass* p, int phase, void* stream)
{
    return pk_launch_sorted(p, stream, phase, json_measure_kernel, json_render_kernel);
}
