// acg_internal.h -- device-side data layout shared by the HIP kernels and the C-ABI host code.
// Not installed; the public surface is include/acarsdec_amd.h.
#pragma once
#include <stdint.h>
#include <stddef.h>

#define ACG_WG_FIR 256          // FIR workgroup: 4 waves, one 64-window tile, taps split over waves
#define ACG_TILE_WIN 64         // windows (12.5 kHz outputs) per FIR tile = one per lane
#define ACG_MSG_TXT 242         // text bytes of a split message (== ACG_MSGTXTMAX of the public header)
#define ACG_WG_MSK 64           // one MSK wave: 64/LPC channels (LPC lanes per channel); 1 or 4 waves per workgroup

// Per-channel demodulator + framing state, resident in HBM across calls.
// Mirrors the MSK/ACARS fields of channel_t (acarsdec.h:76-89) plus bookkeeping.
struct AcgChan {
    double phi;                 // MskPhi
    double df;                  // MskDf
    double lvlsum;              // MskLvlSum
    float clk;                  // MskClk
    int bitcount;               // MskBitCount
    unsigned int S;             // MskS
    unsigned int idx;           // idx
    float inb[22];              // inb[11] complex
    int nbits;                  // nbits
    int astate;                 // Acarsstate
    int blen;                   // blk->len
    int berr;                   // blk->err
    unsigned int outbits;       // outbits
    unsigned int crc0;          // blk->crc[0] (held between CRC1 and CRC2)
    long long nbit_total;       // bits produced since reset
    long long nsamp_total;      // 12.5 kHz samples consumed since reset
    unsigned int soh32;         // low 32 bits of the sample index at which the block's SOH byte completed (acars.c:290 stamps blk->tv there)
    unsigned int pad_;
};

// One queued block (device layout; converted to acg_frame on the host).
struct AcgFrameRec {
    int chn;
    int len;
    int err;
    int bitcount;               // MskBitCount at acars.c:351
    double lvlsum;              // MskLvlSum at acars.c:351 (host takes 10*log10(lvlsum/bitcount))
    long long end_bit;
    long long end_sample;
    unsigned char crc[2];
    unsigned char status;       // 0 raw (as queued by decodeAcars), 1 processed + kept, 2 processed + dropped
    unsigned char pad[1];       // what the repair pass made of the block: ACG_BLK_* below (0 while status is 0); no public record has it
    int soh_back;               // end_sample - (sample at which the SOH byte completed): where the reference stamps blk->tv (acars.c:290)
    unsigned char txt[256];     // 16-byte aligned, 16-byte multiples for vector copies
};

// AcgFrameRec::pad[0], written by blk_repair_kernel beside `status` and read by stats.hip: the exit the block took through
// acars.c:123-207 and what the reference printed on the way
#define ACG_BLK_SHORT 1u            // acars.c:124
#define ACG_BLK_PARITY_MANY 2u      // :145
#define ACG_BLK_UNFIXABLE 3u        // :171, :183
#define ACG_BLK_PARITY_PROBLEM 4u   // :202
#define ACG_BLK_KEPT 5u             // :209
#define ACG_BLK_REASON 7u
#define ACG_BLK_F_PARITY 8u         // "parity error(s): k" (:154), k = 1 .. 3 in bits 6-7
#define ACG_BLK_F_CRC 16u           // "crc error" (:167)
#define ACG_BLK_F_DEL 32u           // queued by the DEL rule (:324-332)
#define ACG_BLK_PN_SHIFT 6

// One channel's statistics on the device: the public acg_chan_stats field for field, except that the last three are encoded so
// that an all-zero record means "nothing yet" and every update is an integer atomic MAX: the bit pattern of a non-negative double
// orders like the double, so lvl_max_bits is the greatest ratio's pattern, lvl_min_inv the COMPLEMENT of the least ratio's, and
// end_sample_p1 the newest kept block's end_sample + 1.  acg_stats_read decodes them.
struct AcgChanStats {
    unsigned int blocks, too_short, parity_many, parity_blocks, parity_errs, crc_errors, unfixable, fixed, parity_problem, kept,
        miss_txt_end, uplink_dropped, label_dropped, empty_dropped, delivered, reserved;
    unsigned long long lvl_min_inv, lvl_max_bits;
    long long end_sample_p1;
};

// One pass of stats.hip over blocks [first, first + n) of the ring
struct AcgMsgRec;
struct AcgLabelFilter;
struct AcgStatsPass {
    const AcgFrameRec* frames;
    unsigned int cap, first, n;
    const AcgMsgRec* msgs;      // message entry points: the split's records of the same blocks (read only when filter_on); else null
    const AcgLabelFilter* f;    // HOST pointer to the context's filter (the launcher passes it by value)
    int filter_on;              // 1: a message entry point with a filter set (kept = the filters' drops + delivered); 0: every
                                // kept block is delivered (a frame entry point, or no filter)
    AcgChanStats* stats;        // [nch]
    int nch;
};

// One split message on the device: the public acg_msg (include/acarsdec_amd.h) field for field, with the two
// operands of the level in place of the padding the host overwrites.
struct AcgMsgRec {
    int chn;
    int err;
    float lvl;                  // filled in on the host: 10*log10(lvlsum/bitcount), acars.c:351
    int txt_len;
    long long end_bit;
    long long end_sample;
    double lvlsum;              // (acg_msg: reserved)
    int bitcount;               // (acg_msg: reserved)
    char valid;                 // (acg_msg: reserved) 0 = dropped by the block repair
    char mode;
    char addr[8];
    char ack;
    char label[3];
    char bid;
    char no[5];
    char fid[7];
    char bs, be;
    char down;
    char txt[ACG_MSG_TXT];
    int soh_back;               // (acg_msg: the host turns it into soh_sample) end_sample - sample of the SOH byte
};

// The batch sink's filters as the device takes them (label.hip): acg_msg_filter with every token packed into one word, its chars
// from the low byte up and zero behind the NUL, so that a label compares as one word (acg_set_msg_filter normalises).
#define ACG_LBL_MAXTOK 64       // == ACG_MSGF_MAXLABELS of the public header
struct AcgLabelFilter {
    unsigned int flags;         // ACG_MSGF_*
    int nlabels;                // 0 = no label filter
    unsigned int tok[ACG_LBL_MAXTOK];
};

// ---- the flight table (flight.hip, flights.cpp): addFlight() / routejson() of output.c:361-456 over a call's split records ----
// One event = one message that reaches addFlight(), extracted by label.hip beside the filter pass (input order)
struct AcgFlightEv {
    unsigned long long key;     // addr (7 bytes) | 1 << 63: never 0 (an empty slot)
    long long soh_sample;
    long long sec;              // tv = t0 + soh_sample / 12500 s
    int usec;
    int chn;
    unsigned long long fid;     // 7 bytes
    unsigned char oooi[40];     // acg_oooi: all zero when the decode failed
    unsigned int e_ok;          // passes -e (routejson() runs only then)
    unsigned int pad_;
};

// One slot of the open-addressing table (HBM, resident across calls); snapshot_kernel turns it into an acg_flight
struct AcgFlightSlot {
    unsigned long long key;     // 0 = never used
    unsigned long long seq;     // (pass << 32) | rank of the latest event in its pass: the move-to-front order
    unsigned long long fid, chm;
    long long ts_sample, tl_sample, ts_sec, tl_sec;
    int ts_usec, tl_usec, first_chn, last_chn;
    int nbm;
    unsigned int rt;
    unsigned int touch;         // the pass that last used or claimed the slot (the claim word of an insertion)
    unsigned int fld[7];        // da sa eta gout gin woff won, 4 chars each (the fifth is always NUL)
};

struct AcgFlightState {
    long long G;                // the largest tv_sec any event has carried
    unsigned int m;             // events of the pass in flight
    unsigned int nseg;          // ... and its aircraft segments
    unsigned int nroutes;       // routes queued
    unsigned int dropped;       // new aircraft that found no slot
    unsigned int nlive;         // snapshot: live entries
    unsigned int nexport;       // export queue: events queued (acg_flights_export)
};

struct AcgRouteRec {
    unsigned long long order;   // (pass << 32) | rank of the triggering event
    unsigned char r[56];        // acg_route
};

struct AcgFlightPass {
    long long t0_sec;
    int t0_usec, mdly;
    unsigned int pass;          // 1, 2, ...: this pass
    unsigned int cap;           // table slots (a power of two)
    AcgFlightSlot* slots;
    AcgFlightState* st;
    AcgRouteRec* routes;
    unsigned int route_cap;
    // per-pass work space, each for at least the pass's n records
    AcgFlightEv* ev;
    unsigned long long *key1, *key1s, *key2, *key2s;
    unsigned int *idx1, *idx1s, *rank2, *rank2s;
    long long* pmax;
    uint2* segs;
    // ---- the table across contexts (acg_flights_set_channels / _export / _import); all null / 0 unless those are used
    const int* chmap;           // or null: the channel number an event records for local channel l, [nmap]
    unsigned int nmap;
    unsigned int n_import;      // events of other contexts uploaded for this pass, applied with its own
    const void* imp;            // acg_flight_event[n_import]
    void* xq;                   // or null: export is on -- the pass ends behind the extraction, its events go to this queue
    unsigned int xq_cap;        // acg_flight_event records xq holds
};

// ---- multi-block reassembly (reasm.hip, flights.cpp): the reference's call site of la_reasm_fragment_add() (output.c:33-101,
// 579-626) over a call's split records; the table's rule is tests/reasm_model.py
#define ACG_RS_PREV_NONE 0x7fffffff
#define ACG_RS_F_DOWN 1u            // AcgReasmEv::flags: a downlink (sequence from no[3], first = 0, no wrap)
#define ACG_RS_F_FINAL 2u           // be != ETB
#define ACG_RS_F_CREATES 4u         // not final and (an uplink or seq == 0): the event can create an entry
#define ACG_RS_WRAP_SHIFT 8         // bits 8-15: the wrap (0 none, 23, 26)
// One event = one record that reaches the table, extracted by reasm_extract_kernel (compacted; any order)
struct AcgReasmEv {
    unsigned long long k0;      // addr (7 bytes, a C string) | label[0] << 56
    unsigned long long k1;      // label[1] | msn[0..2] << 8 (a downlink's; C strings) | 1 << 63: never 0 (an unused slot)
    long long tv_us;            // t0_us + 80 * soh_sample
    long long soh_sample;
    unsigned int rec;           // index of its record in the pass
    int seq;
    unsigned int flags;
    unsigned int txt_len;       // clamped to the record's row
};

// One slot of the open-addressing table; its text row is rows + slot * max_text
struct AcgReasmSlot {
    unsigned long long k0, k1;  // k1 == 0: never used; an idle entry keeps its key (its own tombstone)
    long long first_us, timeout_us, first_soh;
    int prev;                   // ACG_RS_PREV_NONE: no fragment yet
    unsigned int text_len, nfrag;
    unsigned int tail;          // the bytes of the row's last, incomplete dword (text_len & 3 of them), so that an append writes whole dwords
    unsigned int touch;         // the pass that last used or claimed the slot
    unsigned int live;          // 0: idle (removed)
};

struct AcgReasmState {
    long long G;                // the largest tv_us any event of an EARLIER pass carried
    long long Gnext;            // ... and of this pass so far
    unsigned int m, nseg;       // events and segments of the pass in flight
    unsigned int ndone;         // completed messages queued
    unsigned int dropped;       // (call, key) pairs whose key found no slot
    unsigned long long tbytes;  // bytes of their texts queued (each text starts on a 16-byte boundary)
    unsigned int qfull;         // completions that did not fit a queue (the host sizes them so that this stays 0)
    unsigned int pad_;
};

struct AcgReasmDone {
    unsigned long long tkey;    // the final fragment's time key (end_sample << 20 | chn) ...
    unsigned int pass, pad_;    // ... and its pass: the host's final order
    unsigned char r[80];        // acg_reasm_msg; text_off = the text's place in the device queue
};

struct AcgReasmPass {
    long long t0_us;
    unsigned int pass, cap;     // this pass; table slots (a power of two)
    unsigned int max_text;      // bytes per row, a multiple of 16
    unsigned int done_cap;      // records `done` holds
    unsigned long long text_cap;    // bytes `texts` holds
    AcgReasmSlot* slots;
    unsigned char* rows;
    AcgReasmState* st;
    AcgReasmDone* done;
    unsigned char* texts;
    // per-pass work space, each for at least the pass's n records
    AcgReasmEv* ev;
    unsigned long long *ka, *kb;
    unsigned int *va, *vb;
    uint2* segs;
    unsigned int* status;       // [n]: ACG_REASM_* per record of the pass (a word each: no byte stores)
    unsigned char* keep;        // [n]: the label pass's decision per record (AcgLabelPass::keep_out), for the host's index map
    const int* chmap;           // or null: the channel number recorded for local channel l, [nmap]
    unsigned int nmap;
};

// ---- the JSON line renderer (json.hip): buildjson() + cJSON_PrintPreallocated (output.c:227-324) over a call's kept records ----
#define ACG_JS_LINE_MAX 2496    // == ACG_JSON_LINE_MAX of the public header (derived there)
#define ACG_JS_PRE_MAX 224      // ,"station_id":"<escaped>"            (15 + 32 * 6 + 1 = 208)
#define ACG_JS_POST_MAX 224     // ,"app":{"name":"..","ver":".."}}\n    (16 + 96 + 9 + 96 + 3 + 1 = 221)
// What acg_json_enable renders once on the host: the two constant stretches of every line, already escaped
struct AcgJsonDev {
    long long t0_sec;
    int t0_usec;
    int nch;                    // freq tokens
    unsigned int pre_len, post_len;
    unsigned char pre[ACG_JS_PRE_MAX];
    unsigned char post[ACG_JS_POST_MAX];
};

// ---- the text renderer (text.hip): printoneline() / printmsg() (output.c:162-224,327-346), Netoutpp() / Netoutsv() (netout.c:101-140)
#define ACG_TX_REC_MAX 704      // == ACG_TEXT_REC_MAX of the public header (derived there)
#define ACG_TX_FREQ_SLOT 16     // "F:%3.3f " of a channel: at most 12 characters ("F:-2147.484 "), their count in byte 15
// What acg_text_enable renders once on the host
struct AcgTextDev {
    long long t0_sec;
    int t0_usec;
    int nch;                    // freq tokens
    int format;                 // ACG_TEXT_*
    unsigned int flags;         // ACG_TEXT_F_*
    unsigned int station_len;   // SV: "%8s" of the station id, 8 .. 32 characters
    unsigned int pad_;
    unsigned char station[32];
};

// ---- one pass of a device renderer (json.hip, text.hip; the skeleton: sink_pack.h) over a call's kept records
struct AcgSinkPass {
    const AcgMsgRec* recs;      // label.hip's kept records ...
    const unsigned char* oooi;  // ... their acg_oooi ...
    const unsigned int* total;  // ... and how many (a device word: the host does not know it when it launches)
    unsigned int nmax;          // >= *total: what the grids and the work space are sized for
    const void* cfg;            // the unit's own AcgJsonDev / AcgTextDev
    const unsigned char* freq;  // the channel's frequency token: [nch][8] "%3.3f" (<= 7 chars, length in byte 7) / [nch][ACG_TX_FREQ_SLOT]
    int lvl_from_rec;           // lab entry: the level is the record's lvl, not 10 log10(lvlsum / bitcount)
    unsigned long long *key, *key_s;    // (chn, end_bit) and the sorted keys
    unsigned int *idx, *idx_s;          // record index, and in sorted order
    unsigned int *len, *off;            // per sorted rank: record length, byte offset (text: the offset table handed out)
    unsigned int *wg_sum, *wg_cnt;      // per 256 ranks: bytes, records
    unsigned int* counters;     // [0] bytes, [1] records of this pass; [2] level guard (accumulates); [3] unused
    unsigned char* out;         // nmax * (the format's record bound) bytes, 16-byte aligned
    unsigned int out_cap;
    unsigned int nmap;          // acg_set_channel_numbers: the number handed out for slot l is chmap[l], l < nmap; 0 / null: the slot's own.
    const int* chmap;           // The key and the channel tokens take it; the frequency token stays the slot's
};

// ---- the combined outputs pass (outs.hip): one take of kept records, ordered once, rendered into several legs
#define ACG_OUTS_LEGS 4         // == ACG_OUT_LEGS_MAX of the public header
struct AcgOutsPass {
    AcgSinkPass order;          // recs, oooi, total, nmax, the channel map and key / idx / key_s / idx_s: the one order of all legs
    unsigned int nrender;       // rendered legs (JSON, text); each names the same records and the same key_s / idx_s as `order`
    int is_json[ACG_OUTS_LEGS]; // leg l: json.hip's kernels (1) or text.hip's (0)
    AcgSinkPass leg[ACG_OUTS_LEGS];
    AcgMsgRec* g_recs;          // the MSGS leg, or null: the records in sorted order, rank r at g_recs[r] ...
    unsigned char* g_oooi;      // ... their acg_oooi ...
    unsigned int* g_count;      // ... and how many were kept (they sort in front of dropped ones)
};

// ---- the flight table's text (flight_text.hip): printmonitor()'s screen (output.c:458-484) and routejson()'s line (output.c:428-456)
#define ACG_FT_ROW_MAX 78       // == ACG_MONITOR_ROW_MAX of the public header (derived there)
#define ACG_FT_LINE_MAX 363     // == ACG_ROUTE_LINE_MAX of the public header (derived there)
#define ACG_FT_HDR_LEN 110      // cls() 7 + "             Acarsdec monitor " 30 + printtime() 12 + the column header line 61
// What acg_flight_text_enable renders once on the host
struct AcgFlightTextDev {
    int nbch;                   // mask columns shown, 0 .. 16
    unsigned int pre_len;
    unsigned char pre[ACG_JS_PRE_MAX];      // ,"station_id":"<escaped>" or nothing, as AcgJsonDev's
};

// One pass of flight_text.hip: the monitor frame over the live slots in snapshot order, or the route lines over the queue
struct AcgFlightTextPass {
    const AcgFlightTextDev* cfg;
    long long t0_sec;
    int t0_usec;
    int pad_;
    long long hdr_soh;          // monitor: the header's message, tv = t0 + hdr_soh / 12500 s; < 0: the newest live entry's tl (none: t0)
    const AcgFlightSlot* slots; // monitor: the table ...
    const AcgFlightState* st;   // ... and its state (nlive = the rows, dropped)
    const AcgRouteRec* routes;  // routes: the queue
    const unsigned int* total;  // a device word: the rows / lines of this pass
    unsigned int nmax;          // >= *total: what the work space is sized for
    unsigned int base;          // bytes in front of the first record (the monitor's header)
    unsigned long long *key, *key_s;    // routes: the (pass, rank) tag and the sorted tags
    unsigned int *idx, *idx_s;          // routes: queue index, and in sorted order; monitor: idx_s = the slots in snapshot order
    unsigned int *len, *off;            // per sorted rank: length, byte offset behind base
    unsigned int *wg_sum, *wg_cnt;      // per 256 ranks: bytes, records
    unsigned int* counters;     // [0] bytes behind base, [1] records; [2] monitor: the table's `dropped`; [3] routes: the lines of this pass
    unsigned char* out;         // 16-byte aligned
    unsigned int out_cap;
};

struct FirArgs {
    const uint8_t* iq;          // [nstreams] rows
    size_t pitch;               // bytes between stream rows (multiple of 16)
    const int* stream_of;       // [nch]
    const float* taps;          // [nch][ntaps_pad][2]
    float* dm;                  // [nch][dm_pitch]
    size_t dm_pitch;            // floats
    int nch;
    int decim;                  // M
    int ntaps_pad;              // taps per channel, zero padded to a multiple of 8
    int ntaps;                  // taps per channel that carry values (the exact-order kernel stops there)
    int nwin;                   // outputs per channel this launch
    int nseg;                   // time segments per channel (grid = nch * nseg)
    int row_bytes;              // 2*M
    int row_stride;             // LDS row stride in bytes ((row_stride/16) odd)
    int cpr;                    // 16-byte chunks per row = row_bytes/16
    unsigned int cpr_magic;     // ceil(2^20 / cpr): c / cpr == (c * magic) >> 20 for c < 2^11
    size_t plane;               // FMT_SPLIT: byte distance from a stream's I plane to its Q plane
    const int4* groups;         // shared-stream kernel: {stream, first index into group_ch, channel count (<= 8), 0}
    const int* group_ch;        // shared-stream kernel: channel ids ordered by stream
    int ngroups;
    int s8;                     // host side only: the bytes are int8 I,Q (ACG_FMT_CS8) and the launchers take the u8 kernels' signed
                                // twins.  (It fills the padding behind ngroups: no other member moves, no kernel reads it.)
    const float* gtaps;         // shared-stream kernel: taps regrouped [group][step][channel][16]
    int wg_per_cu;              // resident down-converter workgroups per CU (0 = as many as fit, at most 5)
    int ncu;                    // CUs the launch may use (0 = the whole device; fewer on a CU-masked stream)
    int kseg;                   // format kernels: column segments per window (long windows pass through LDS in kseg slices)
    int cpr_total;              // format kernels: 16-byte chunks per whole window (cpr = chunks per slice)
    float out_scale;            // power-of-two scale applied to |D| (1, 1/32768 soapy.c:241, 1/4 sdrplay.c:225)
    unsigned int* work_counter; // run dispenser of the dynamically scheduled kernels (ACG_DISP_WORDS words per launch in flight)
    int stream_identity;        // stream_of[ch] == ch for every channel: the row base needs no lookup
    int high_prio;              // wave-private kernel: raise the wave priority (the demodulator shares its CUs and has slack)
    int run_pairs;              // wave-private kernel: two-tile bodies per dispensed run (set by the launcher)
    int shares_cus;             // demodulator workgroups run on the same CUs (no CU partition): leave them LDS
    const void* mm_img;         // matrix-pipe shared-stream kernel (fir_mm.hip): the groups' A-operand images (tap digits)
    const void* mm_chan;        // ... and MmChan[nch]
};

// fir_mm.hip: what a channel's tap table contributes besides its digits
struct MmChan {
    double scale;               // 2^(e - 30): value of one unit of the 31-bit fixed-point taps
    double dc_re, dc_im;        // (128 - 127.37f) (1 + j) sum w
    double up;                  // 2^(30 - e), 0 for an all-zero table
};

// Run dispenser of one launch in flight: words [0], [1] = {tickets, finished} of the workgroup-granular
// kernels; the wave-granular kernel uses ACG_DISP_SHARDS ticket words, one 128-byte line apart (so that the
// atomics of different shards go to different L2 channels), and a `finished` word after them.
#define ACG_SINCOS_N 128
#define ACG_DISP_SHARDS 8
#define ACG_DISP_STRIDE 32
#define ACG_DISP_WORDS ((ACG_DISP_SHARDS + 1) * ACG_DISP_STRIDE)

struct MskArgs {
    AcgChan* st;                // [nch]
    const float* dm;            // [nch][dm_pitch]
    size_t dm_pitch;
    const float* h;             // [133] matched filter prototype (msk.c:44-48)
    const double* sctab;        // [ACG_SINCOS_N][2] (cos, sin) of j * 2 pi / N (acg_host_sincos_table)
    unsigned char* txt;         // [nch][256] blk->txt being assembled
    AcgFrameRec* frames;        // queue
    unsigned int* frame_count;  // queue length (atomic)
    unsigned int frame_cap;
    float2* bits;               // [nch][bit_cap] {vo, lvl}, may be null
    int* nbits_out;             // [nch]
    int bit_cap;
    int nch;
    int len;                    // samples per channel this launch
    int bit_append;             // 0: bit records start at 0; 1: append after nbits_out[ch] (same call)
    int waves_per_group;        // 4 on a CU-masked stream (placement), else 1
    unsigned int* snap;         // host-mapped word: the last workgroup out publishes the queue length there
    unsigned int* done_ctr;     // workgroups finished (re-armed by the last one)
    int high_prio;              // raise wave priority (latency mode)
    int dm_vec_ok;              // dm rows are 16-byte aligned: the window refill may use float4 loads
    unsigned long long* stamp;  // measurement build (ACG_MSK_STAMP) only: [waves][10] phase cycle sums, else null
    int precise_mixer;          // ACG_F_PRECISE_MIXER: the < 1 ulp polynomial sin/cos instead of table + rotation
};

// pcm.hip: interleaved PCM frames [nframes][nch] -> columns [0, nframes) of the planar dm rows
struct PcmArgs {
    const void* frames;         // 4-byte aligned
    float* dm;                  // [nch][dm_pitch]
    size_t dm_pitch;            // floats, >= nframes
    int nch;
    int nframes;
    int fmt;                    // ACG_PCM_S16 / ACG_PCM_F32
};

#ifdef __cplusplus
extern "C" {
#endif
// kernel launchers (fir.hip / msk.hip / synth.hip); stream is a hipStream_t
int acg_launch_fir(const FirArgs* a, void* stream);
int acg_launch_fir_generic(const FirArgs* a, void* stream);
int acg_launch_fir_shared(const FirArgs* a, void* stream);
int acg_launch_regroup_taps(const FirArgs* a, void* stream);          // channels grouped by stream (a->groups)
size_t acg_fir_mm_image_bytes(int decim, int ngroups);               // fir_mm.hip; 0: the matrix kernel does not take this decimation
int acg_fir_mm_takes(const FirArgs* a);
int acg_launch_fir_mm_prep(const FirArgs* a, void* stream);
int acg_launch_fir_mm(const FirArgs* a, void* stream);
size_t acg_fir_mm1_image_bytes(int decim, int nch);                  // fir_mm.hip, one stream per channel: 256 B per channel and k-step
int acg_fir_mm1_takes(const FirArgs* a);
int acg_launch_fir_mm1_prep(const FirArgs* a, void* stream);
int acg_launch_fir_mm1(const FirArgs* a, void* stream);
int acg_launch_fir_fmt(const FirArgs* a, int fmt, void* stream);     // fmt: 1 CS16, 2 split int16 planes, 3 real f32, 5 complex f32
// fir_iq.hip: the recordings' formats, reached through the launchers above (a->s8 / fmt 5), never from the host runtime
int acg_launch_fir_s8(const FirArgs* a, void* stream);               // int8 I,Q, one stream per channel
int acg_launch_fir_shared_s8(const FirArgs* a, long long grid, size_t lds, void* stream);   // ... several channels per stream, vector pipe
int acg_launch_fir_cf32(const FirArgs* a, void* stream);             // complex float32
// fir.hip: the kernel family a launch of sample format fmt (1 .. 5; 4 = int8 I,Q on the u8 kernels' signed twins, a->s8) takes,
// and the streaming kernel's tile geometry.  A weak reference, as the sinks' launchers below: the host runtime is also linked
// without the device units, where the lab entry that reports this says ACG_ESTATE.
#define ACG_FIR_FAM_STREAMING 1     // wave-private streaming kernel (fir_u8_direct / fir_s8_direct / fir_fmt_direct)
#define ACG_FIR_FAM_WORKGROUP 2     // workgroup-granular fallback (fir_u8_persist / fir_s8_persist / fir_fmt_kernel)
#define ACG_FIR_FAM_MATRIX 3        // matrix pipe (fir_mm.hip)
#define ACG_FIR_FAM_SHARED 4        // shared-stream vector kernel
struct FirChoice {
    int family;
    int tile_win;               // streaming kernel: windows per tile (W)
    long long runs;             // ... dispensed runs of the launch
    long long waves;            // ... waves launched
    int wpg, pairs;             // ... waves per workgroup, two-tile bodies per run
};
__attribute__((weak)) int acg_fir_choice(const FirArgs* a, int fmt, FirChoice* out);
size_t acg_fir_lds_bytes(const FirArgs* a);
// fir.hip: per-device launch state of every down-converter unit (not exported: the version script lists the public headers' names)
int acg_fir_device_cus(int* num_cu);                                 // CUs of the current device; returns a HIP error or 0
int acg_fir_lds_optin(const void* kernel, size_t bytes);             // opts `kernel` in for `bytes` of dynamic LDS on the current device
int acg_launch_msk(const MskArgs* a, int lanes_per_channel, void* stream);
int acg_launch_msk_lean(const MskArgs* a, int lanes_per_channel, int waves_per_group, unsigned int grid, void* stream);   // msk_lean.hip: the in_callback-shaped launches, with or without a bit log
int acg_launch_msk_lean_wide(const MskArgs* a, int lanes_per_channel, int waves_per_group, unsigned int grid, void* stream);   // msk_lean_wide.hip: the same with 16 lanes per channel, four-wave workgroups
int acg_launch_msk2(const MskArgs* a, int pairs_per_group, void* stream);     // msk2.hip: the stream split over two waves (8 lanes per channel)
int acg_launch_blk_repair(AcgFrameRec* frames, unsigned int cap, const unsigned int* upto, unsigned int* done_upto,
                          unsigned int* done_ctr, const unsigned short* synd, const unsigned short* crctab, int nch, void* stream);
// blk.hip: the field split of blocks [first, first + n) of the ring into out[n]; with `labels`, label.hip's pass over those records
// follows on the same stream (frames == null: out already holds the records, only the label pass runs)
struct AcgLabelPass {
    const AcgLabelFilter* f;
    unsigned int* wg_count;     // ceil(n / 256) words of scratch
    AcgMsgRec* kept;            // the records kept, in order
    void* oooi;                 // acg_oooi[]: their labels decoded
    unsigned int* total;        // how many were kept
    unsigned char* keep_out;    // or null: the decision per input record
    const AcgFlightPass* flights;   // or null: flight.hip's pass over the same n records follows
};
int acg_launch_msg_split(const AcgFrameRec* frames, unsigned int cap, unsigned int first, unsigned int n, AcgMsgRec* out, void* stream,
                         const AcgLabelPass* labels = nullptr);
// label.hip: filter, label decoding and compaction of n split records (reached through acg_launch_msg_split)
int acg_launch_msg_labels(const AcgMsgRec* recs, unsigned int n, const AcgLabelPass* p, void* stream);
// label.hip: the events of n records (filter f: -A / -b decide, -e is only noted), compacted, with the keys of the time sort
int acg_launch_flight_extract(const AcgMsgRec* recs, unsigned int n, const AcgLabelFilter* f, const AcgFlightPass* p, void* stream);
// flight.hip: extraction, ordering, segment walk and table update for n records and p->n_import uploaded events (p->xq set:
// extraction and the hand-over of the events to the export queue, nothing else)
int acg_launch_flight_pass(const AcgMsgRec* recs, unsigned int n, const AcgLabelFilter* f, const AcgFlightPass* p, void* stream);
// flight.hip: the live entries, latest update first, as acg_flight records in out[cap]; st->nlive = how many
int acg_launch_flight_snapshot(const AcgFlightPass* p, unsigned long long* skey, unsigned long long* skey_s, unsigned int* sval,
                               unsigned int* sval_s, void* out, void* stream);
// flight.hip: the snapshot's first half -- the live slots compacted and put in snapshot order: sval_s[0 .. st->nlive)
int acg_launch_flight_snapkeys(const AcgFlightPass* p, unsigned long long* skey, unsigned long long* skey_s, unsigned int* sval,
                               unsigned int* sval_s, void* stream);
// flight_text.hip: measure, scan and render the monitor frame over the slots idx_s[0 .. *total) (behind acg_launch_flight_snapkeys);
// keys, sort, measure, scan and render the lines of the first n queued routes.  p->counters says how much.
int acg_launch_flight_monitor_text(const AcgFlightTextPass* p, void* stream);
int acg_launch_flight_route_text(const AcgFlightTextPass* p, unsigned int n, void* stream);
// flight.hip: the pass's stable radix sort of (64-bit key, 32-bit value) pairs by one workgroup, for other passes: n = *n_ptr
// (a device word) or n_fixed; the result lies in (kb, vb)
int acg_launch_sort_pairs(unsigned long long* ka, unsigned int* va, unsigned long long* kb, unsigned int* vb, const unsigned int* n_ptr,
                          unsigned int n_fixed, void* stream);
// reasm.hip: extraction, the three sorts, heads, segment walk and table update for the n records of one pass (-A / -b of f decide)
int acg_launch_reasm_pass(const AcgMsgRec* recs, unsigned int n, const AcgLabelFilter* f, const AcgReasmPass* p, void* stream);
// json.hip, text.hip: a unit's part of outs.hip's sequence, over records that are ordered (p->key_s / p->idx_s are filled): the
// measure kernel (phase ACG_SORTED_MEASURE) or the render kernel (ACG_SORTED_RENDER); the scan between them is the caller's
#define ACG_SORTED_MEASURE 0
#define ACG_SORTED_RENDER 1
int acg_launch_json_sorted(const AcgSinkPass* p, int phase, void* stream);
int acg_launch_text_sorted(const AcgSinkPass* p, int phase, void* stream);
// outs.hip: keys and sort once, every leg's measure, one scan over all legs, every leg's render, the MSGS leg's gather; each
// leg's counters say how much.  The one launch sequence of the JSON sink, the text sink (one leg each) and the outputs.
// A WEAK reference, as flights.h's: the host runtime is also linked without the device units (the sanitizer build of
// tests/test_host_logic.py, which stubs the launchers it knows); there the sinks are absent and acg_json_enable, acg_text_enable
// and acg_outputs_enable say ACG_ESTATE.
__attribute__((weak)) int acg_launch_outs(const AcgOutsPass* o, void* stream);
// stats.hip: the per-channel statistics of the blocks an entry point consumes (weak for the same reason: there acg_stats_enable
// says ACG_ESTATE)
__attribute__((weak)) int acg_launch_chan_stats(const AcgStatsPass* p, void* stream);
// pcm.hip: the de-interleave of one call (weak for the same reason: there the PCM entry points say ACG_ESTATE)
__attribute__((weak)) int acg_launch_pcm_deint(const PcmArgs* a, void* stream);
int acg_launch_sincos_selftest(const double* x, double* s, double* c, int n, const double* sctab, void* stream);
int acg_launch_div2_selftest(const double* n0, const double* n1, const double* d, double* out, int n, void* stream);
int acg_launch_synth_iq(uint8_t* iq, size_t pitch, int nrows, int nout, int decim, const float* env,
                        size_t env_pitch, const int* env_index, const float* off_hz, const float* phase,
                        float scale, float noise, uint64_t seed, void* stream);
int acg_launch_fill_random(uint8_t* dev, size_t pitch, int nrows, size_t row_bytes, uint64_t seed, void* stream);
int acg_launch_read_probe(const void* dev, size_t bytes, unsigned int* sink, int ncu, void* stream);
#ifdef __cplusplus
}
#endif
