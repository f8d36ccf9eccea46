// text.hip -- the reference's per-message TEXT formats for the batch sink, over the records label.hip kept and compacted for one
// drain / collect, beside json.hip:
//   ACG_TEXT_ONELINE  printoneline()  output.c:327-346   what -o 1 prints
//   ACG_TEXT_STD      printmsg()      output.c:162-224   what -o 2 (the default) prints, the build without libacars
//   ACG_TEXT_PP       Netoutpp()      netout.c:101-120   the planeplotter datagram (-N)
//   ACG_TEXT_SV       Netoutsv()      netout.c:122-140   the native datagram (-n)
// What leaves is the records' bytes packed back to back in (chn, end_bit) order and the table of their offsets: a record may hold
// any byte ("%1c" of a NUL mode, a '\n' inside a text), so there is nothing to split it by.
//
// This unit's two kernels are launched as json.hip's, by outs.hip's sequence (acg_launch_outs; the text sink is that sequence with
// one leg) through acg_launch_text_sorted, on the stream of the label pass they hang on: text_measure_kernel (one WAVE per record:
// its length) and, behind the scan in sorted order that makes the offset table, text_render_kernel (one wave per record: the
// record assembled in a per-wave LDS row, flushed seam-safe).  Flush, record load, the level's float and the kernels' bodies are
// shared with json.hip (sink_pack.h), the row writers (bounded store, literal, fill, number token) with json.hip and
// flight_text.hip (sink_put.h); this unit supplies text_record, keeps its kernels as wrappers and what only these formats use
// (tx_*).  Measure and render run the SAME function (text_record<false / true>).
//
// "%Ns" is a ballot and a find-first (the C string's end) and max(0, N - len) spaces in front; the text is four rounds of 64 lanes,
// byte i at place i; lane j computes character j of a number or of the date (json_num.h, text_num.h).  No lane walks anything, no
// scratch (fields are read out of LDS, digits are computed), no per-byte global traffic (a record comes in as 80 + 10 dword
// loads, the channel's "F:" token as two quadwords, the station as dwords; a record leaves as 16-byte stores and < 30 byte stores).
#include "sink_put.h"
#include "text_num.h"

static_assert(ACG_TX_REC_MAX == ACG_TEXT_REC_MAX && ACG_TX_REC_MAX % 64 == 0, "record bound");

constexpr unsigned int TX_B = ACG_TX_REC_MAX;                     // the row's bound (sink_put.h)
#define TX_LIT(s) PK_PUT_LIT(TX_B, s)

// one and two characters
template <bool W>
__device__ __forceinline__ unsigned int tx_ch(unsigned char* row, unsigned int pos, unsigned int c, int lane)
{
    if (W && lane == 0) pk_st<W, TX_B>(row, pos, (unsigned char)c);
    return pos + 1;
}

template <bool W>
__device__ __forceinline__ unsigned int tx_ch2(unsigned char* row, unsigned int pos, unsigned int c0, unsigned int c1, int lane)
{
    if (W && lane < 2) pk_st<W, TX_B>(row, pos + lane, (unsigned char)(lane ? c1 : c0));
    return pos + 2;
}

// the first n characters of printdate()'s text
template <bool W>
__device__ __forceinline__ unsigned int tx_date(unsigned char* row, unsigned int pos, const TnDate& d, int n, int lane)
{
    if (W && lane < n) pk_st<W, TX_B>(row, pos + lane, tn_date_char(d, lane));
    return pos + (unsigned int)n;
}

template <bool W>
__device__ __forceinline__ unsigned int tx_level(unsigned char* row, unsigned int pos, float lvl, int lane)
{
    const TnLevel l = tn_level(lvl);
    if (W && lane < l.len) pk_st<W, TX_B>(row, pos + lane, tn_level_char(l, lane));
    return pos + (unsigned int)l.len;
}

// "%<width>s" of the C string at s (at most maxlen < 64 bytes): right-justified to at least width, never cut
template <bool W>
__device__ __forceinline__ unsigned int tx_str(unsigned char* row, unsigned int pos, const unsigned char* s, int maxlen, int width, int lane)
{
    const unsigned int b = lane < maxlen ? s[lane] : 0u;          // (written out: through pk_strlen text_render_kernel moves, 6796 -> 6717)
    const unsigned long long nul = __ballot(b == 0);              // (never 0: maxlen < 64)
    const int n = __ffsll((unsigned long long)nul) - 1;
    const int pad = width > n ? width - n : 0;
    if (W) {
        if (lane < pad) pk_st<W, TX_B>(row, pos + lane, ' ');
        if (lane < n) pk_st<W, TX_B>(row, pos + pad + lane, (unsigned char)b);
    }
    return pos + (unsigned int)(pad + n);
}

// the C string within the first `limit` bytes of the text, byte i at place i; subst: '\n' and '\r' become a space
template <bool W>
__device__ __forceinline__ unsigned int tx_text(unsigned char* row, unsigned int pos, const unsigned char* txt, int limit, bool subst, int lane)
{
    for (int rd = 0; rd < 4; ++rd) {
        const int i = 64 * rd + lane;
        unsigned int b = i < limit ? txt[i] : 0u;
        const unsigned long long nul = __ballot(b == 0);
        const int n = nul ? __ffsll((unsigned long long)nul) - 1 : 64;
        if (subst && (b == '\n' || b == '\r')) b = ' ';
        if (W && lane < n) pk_st<W, TX_B>(row, pos + lane, (unsigned char)b);
        pos += (unsigned int)n;
        if (n < 64) break;                                         // (wave-uniform)
    }
    return pos;
}

// n <= 32 bytes the host prepared (SV's station), 4-byte aligned: a dword load per lane
// (one guarded load, not pk_put_words' 256-byte loop: with the loop text_render_kernel moves, 6796 -> 6825 instructions)
template <bool W>
__device__ __forceinline__ unsigned int tx_words(unsigned char* row, unsigned int pos, const unsigned char* src, unsigned int n, int lane)
{
    if (W && 4u * lane < n) {
        const unsigned int w = *(const unsigned int*)(src + 4u * lane);
#pragma unroll
        for (unsigned int k = 0; k < 4; ++k)
            if (4u * lane + k < n) pk_st<W, TX_B>(row, pos + 4u * lane + k, (unsigned char)(w >> (8 * k)));
    }
    return pos + n;
}

// " <label line> : <field>\n" of printmsg()'s OOOI part
#define TX_OOOI(at, s) do { if (O[at]) { TX_LIT(s); pos = tx_str<W>(row, pos, O + at, 4, 0, lane); pos = tx_ch<W>(row, pos, '\n', lane); } } while (0)

// One record.  R: the message and, at R + 320, its acg_oooi (LDS); row: where the record's first byte goes (W) or unused.
template <bool W>
__device__ __forceinline__ unsigned int text_record(const unsigned char* R, unsigned char* row, const AcgSinkPass& p, int lane, bool* near_mid)
{
    const AcgMsgRec* r = (const AcgMsgRec*)R;
    const AcgTextDev* cfg = (const AcgTextDev*)p.cfg;
    const int format = cfg->format;                               // (wave-uniform, as everything read from cfg and R)
    const unsigned int flags = cfg->flags;
    unsigned int pos = 0;
    // ---- tv = t0 + soh_sample / 12500 s in integers (a sample is exactly 80 us), as json.hip
    const long long soh = r->end_sample - (long long)r->soh_back;
    const long long us = (long long)cfg->t0_usec + soh * 80ll;
    long long q = us / 1000000ll, rem = us % 1000000ll;
    if (rem < 0) { rem += 1000000ll; --q; }
    const TnDate date = tn_date(cfg->t0_sec + q, (int)rem);
    const int chn = r->chn;                                       // the slot: the "F:" token's index
    const int num = pk_chn(p, chn);                               // the number handed out (acg_set_channel_numbers)
    *near_mid = false;
    const float lvl = format == ACG_TEXT_PP ? 0.0f : pk_level(r, p.lvl_from_rec, near_mid);
    int tl = r->txt_len;
    tl = tl < 0 ? 0 : tl > ACG_MSG_TXT ? ACG_MSG_TXT : tl;
    const unsigned char* txt = R + offsetof(AcgMsgRec, txt);
    const unsigned int mode = (unsigned char)r->mode, ack = (unsigned char)r->ack, bid = (unsigned char)r->bid;
    const unsigned char *addr = R + offsetof(AcgMsgRec, addr), *label = R + offsetof(AcgMsgRec, label), *no = R + offsetof(AcgMsgRec, no),
                        *fid = R + offsetof(AcgMsgRec, fid);

    if (format == ACG_TEXT_ONELINE) {                             // output.c:338-344
        pos = tx_ch<W>(row, pos, '#', lane);
        pos = pk_put_tok<W, TX_B>(row, pos, jn_int((long long)num + 1), lane);
        TX_LIT(" (L:");
        pos = tx_level<W>(row, pos, lvl, lane);
        TX_LIT(" E:");
        pos = pk_put_tok<W, TX_B>(row, pos, jn_int(r->err), lane);
        TX_LIT(") ");
        if (flags & ACG_TEXT_F_DATE) pos = tx_date<W>(row, pos, date, TN_DATE_LEN, lane);
        pos = tx_ch<W>(row, pos, ' ', lane);
        pos = tx_str<W>(row, pos, addr, 7, 7, lane);
        pos = tx_ch<W>(row, pos, ' ', lane);
        pos = tx_str<W>(row, pos, fid, 6, 6, lane);
        pos = tx_ch2<W>(row, pos, ' ', mode, lane);
        pos = tx_ch<W>(row, pos, ' ', lane);
        pos = tx_str<W>(row, pos, label, 2, 2, lane);
        pos = tx_ch<W>(row, pos, ' ', lane);
        pos = tx_str<W>(row, pos, no, 4, 4, lane);
        pos = tx_ch<W>(row, pos, ' ', lane);
        pos = tx_text<W>(row, pos, txt, tl < 59 ? tl : 59, true, lane);          // strncpy(txt, msg->txt, 59)
        pos = tx_ch<W>(row, pos, '\n', lane);
        return pos;
    }
    if (format == ACG_TEXT_STD) {                                 // output.c:166-215
        TX_LIT("\n[#");
        pos = pk_put_tok<W, TX_B>(row, pos, jn_int((long long)num + 1), lane);
        TX_LIT(" (");
        if (flags & ACG_TEXT_F_FREQ) {
            if ((unsigned int)chn < (unsigned int)cfg->nch) {
                const unsigned long long* ft = (const unsigned long long*)(p.freq + (size_t)chn * ACG_TX_FREQ_SLOT);
                const unsigned long long lo = ft[0], hi = ft[1];
                const unsigned int fn = (unsigned int)(hi >> 56) & 15u;
                if (W && (unsigned int)lane < fn) pk_st<W, TX_B>(row, pos + lane, (unsigned char)((lane < 8 ? lo : hi) >> (8 * (lane & 7))));
                pos += fn;
            } else {                                              // (no caller gets here: the entry points keep chn < nch.  It only
                TX_LIT("F:0.000 ");                               //  keeps the token table's load in bounds and the record well formed)
            }
        }
        TX_LIT("L:");
        pos = tx_level<W>(row, pos, lvl, lane);
        TX_LIT(" E:");
        pos = pk_put_tok<W, TX_B>(row, pos, jn_int(r->err), lane);
        TX_LIT(") ");
        if (flags & ACG_TEXT_F_DATE) pos = tx_date<W>(row, pos, date, TN_DATE_LEN, lane);
        pos = tx_ch<W>(row, pos, ' ', lane);
        pos = pk_fill<W, TX_B>(row, pos, '-', 32, lane);
        TX_LIT("\nMode : ");
        pos = tx_ch<W>(row, pos, mode, lane);
        TX_LIT(" Label : ");
        pos = tx_str<W>(row, pos, label, 2, 2, lane);
        pos = tx_ch<W>(row, pos, ' ', lane);
        if (bid) {
            TX_LIT("Id : ");
            pos = tx_ch2<W>(row, pos, bid, ' ', lane);
            if (ack == '!') {
                TX_LIT("Nak\n");
            } else {
                TX_LIT("Ack : ");
                pos = tx_ch2<W>(row, pos, ack, '\n', lane);
            }
            TX_LIT("Aircraft reg: ");
            pos = tx_str<W>(row, pos, addr, 7, 0, lane);
            pos = tx_ch<W>(row, pos, ' ', lane);
            if (bid >= '0' && bid <= '9') {                       // IS_DOWNLINK_BLK, output.c:31,185
                TX_LIT("Flight id: ");
                pos = tx_str<W>(row, pos, fid, 6, 0, lane);
                TX_LIT("\nNo: ");
                pos = tx_str<W>(row, pos, no, 4, 4, lane);
            }
        }
        pos = tx_ch<W>(row, pos, '\n', lane);
        if (tl > 0 && txt[0]) {
            pos = tx_text<W>(row, pos, txt, tl, false, lane);
            pos = tx_ch<W>(row, pos, '\n', lane);
        }
        if (r->be == 0x17) TX_LIT("ETB\n");
        const unsigned char* O = R + sizeof(AcgMsgRec);          // oooi_t: da sa eta gout gin woff won, then `decoded`
        if (O[35]) {
            pos = pk_fill<W, TX_B>(row, pos, '#', 26, lane);
            pos = tx_ch<W>(row, pos, '\n', lane);
            TX_OOOI(0, "Destination Airport : ");
            TX_OOOI(5, "Departure Airport : ");
            TX_OOOI(10, "Estimation Time of Arrival : ");
            TX_OOOI(15, "Gate out Time : ");
            TX_OOOI(20, "Gate in Time : ");
            TX_OOOI(25, "Wheels off Tme : ");
            TX_OOOI(30, "Wheels on Time : ");
        }
        return pos;
    }
    // ---- the two datagrams: "<head>%1c %7s %1c %2s %1c %4s %6s %s" (netout.c:112-114,131-135)
    if (format == ACG_TEXT_SV) {
        pos = tx_words<W>(row, pos, cfg->station, cfg->station_len, lane);
        pos = tx_ch<W>(row, pos, ' ', lane);
        pos = pk_put_tok<W, TX_B>(row, pos, jn_int((long long)num + 1), lane);
        pos = tx_ch<W>(row, pos, ' ', lane);
        pos = tx_date<W>(row, pos, date, TN_DATE_SV_LEN, lane);
        pos = tx_ch<W>(row, pos, ' ', lane);
        pos = pk_put_tok<W, TX_B>(row, pos, jn_int(r->err), lane);
        pos = tx_ch<W>(row, pos, ' ', lane);
        pos = pk_put_tok<W, TX_B>(row, pos, tn_int0(tn_trunc_int(lvl), 3), lane);
        pos = tx_ch<W>(row, pos, ' ', lane);
    } else {
        TX_LIT("AC");
    }
    pos = tx_ch2<W>(row, pos, mode, ' ', lane);
    pos = tx_str<W>(row, pos, addr, 7, 7, lane);
    pos = tx_ch<W>(row, pos, ' ', lane);
    pos = tx_ch2<W>(row, pos, ack, ' ', lane);
    pos = tx_str<W>(row, pos, label, 2, 2, lane);
    pos = tx_ch<W>(row, pos, ' ', lane);
    pos = tx_ch2<W>(row, pos, bid ? bid : '.', ' ', lane);
    pos = tx_str<W>(row, pos, no, 4, 4, lane);
    pos = tx_ch<W>(row, pos, ' ', lane);
    pos = tx_str<W>(row, pos, fid, 6, 6, lane);
    pos = tx_ch<W>(row, pos, ' ', lane);
    pos = tx_text<W>(row, pos, txt, tl, format == ACG_TEXT_PP, lane);            // Netoutpp substitutes, Netoutsv does not
    return pos;
}

// what this unit gives the passes' skeleton (sink_pack.h)
struct TextFmt {
    static constexpr unsigned int REC_MAX = ACG_TX_REC_MAX;
    template <bool W>
    static __device__ __forceinline__ unsigned int record(const unsigned char* R, unsigned char* row, const AcgSinkPass& p, int lane, bool* near_mid)
    {
        return text_record<W>(R, row, p, lane, near_mid);
    }
    static __device__ __forceinline__ unsigned char* row_at(unsigned char (*rows)[REC_MAX + 16], int wv, unsigned int off)
    {
        return rows[wv] + (off & 15u);                            // the row mirrors the output's alignment (written in this order: sink_pack.h)
    }
};

// the passes (sink_pack.h): the kernels and their LDS are this unit's own
__global__ __launch_bounds__(64 * PK_WAVES) void text_measure_kernel(AcgSinkPass p)
{
    __shared__ __attribute__((aligned(16))) unsigned char recs[PK_WAVES][PK_REC];
    const unsigned int r = blockIdx.x * PK_WAVES + (threadIdx.x >> 6);        // wave-uniform
    if (r >= p.nmax || r >= *p.total) return;                                    // (the early-outs are the kernel's: sink_pack.h, pk_measure)
    if (p.key_s[r] == ~0ull) {
        if ((threadIdx.x & 63) == 0) p.len[r] = 0;
        return;
    }
    pk_measure<TextFmt>(recs, p, r);
}

__global__ __launch_bounds__(64 * PK_WAVES) void text_render_kernel(AcgSinkPass p)
{
    __shared__ __attribute__((aligned(16))) unsigned char recs[PK_WAVES][PK_REC];
    __shared__ __attribute__((aligned(16))) unsigned char rows[PK_WAVES][TextFmt::REC_MAX + 16];
    pk_render<TextFmt>(recs, rows, p);
}

extern "C" int acg_launch_text_sorted(const AcgSinkPass* p, int phase, void* stream)
{
    return pk_launch_sorted(p, stream, phase, text_measure_kernel, text_render_kernel);
}
