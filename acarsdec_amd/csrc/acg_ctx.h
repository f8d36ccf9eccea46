// acg_ctx.h -- what the units of the host runtime share (tune.cpp, ctx.cpp, process.cpp, results.cpp, sinks.cpp, state.cpp,
// lab.cpp; nothing else includes it): the context, the error helpers and the few functions that cross a unit.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "acarsdec_amd.h"
#include "acarsdec_amd_lab.h"
#include "acg_internal.h"
#include "flights.h"

// host_setup.c
extern "C" void acg_host_msk_h(float* h);
extern "C" void acg_host_sincos_table(double* tab);
extern "C" float acg_host_level_db(double lvlsum, int bitcount);
extern "C" void acg_host_crc_tables(unsigned short* crc, unsigned short* synd);
extern "C" void acg_host_crc_tables_n(unsigned short* crc, unsigned short* synd, int nk);

// tune.cpp: the tuning table's look-ups
extern "C" int acg_tune_get(const char* name, int dflt);
extern "C" int acg_tune_has(const char* name);

struct EvPair { hipEvent_t a, b; };

// The *_host entry points' way to the device: TWO staging buffers and a copy stream of their own, so that the host-to-device copy
// of call i+1 runs while the kernels of call i read the other buffer (the caller's memory is free again when the call returns:
// rtl.c:314-330 / soapy.c:220-254 hand over a buffer that is only valid during the callback).  Every entry point copies into
// buf[cur] behind the buffer's last reader, runs its device path and turns the ring (process.cpp: stage_*); the carrying feeds
// keep the samples of an incomplete window at the head of buf[cur].
struct StageRing {
    void* buf[2] = {nullptr, nullptr};
    size_t bytes = 0;               // of EACH buffer
    int cur = 0;                    // the buffer the next copy goes to
    hipStream_t copy = nullptr;     // the copy stream
    hipEvent_t copied = nullptr;    // the newest copy from the caller's memory is done
    hipEvent_t free[2] = {nullptr, nullptr};    // the launches that read the buffer are done ...
    bool free_valid[2] = {false, false};        // ... recorded, and the copy stream does not wait for it yet
    int fmt = 0;                    // acg_feed_samples_host / acg_feed_rate_host: format and samples of the incomplete window carried
    size_t fill = 0;
    void reset() { cur = 0; fill = 0; free_valid[0] = free_valid[1] = false; }      // behind a device synchronise: nothing reads, nothing is carried
    void destroy()
    {
        for (auto p : buf) hipFree(p);
        if (copy) hipStreamDestroy(copy);
        if (copied) hipEventDestroy(copied);
        for (auto e : free) if (e) hipEventDestroy(e);
    }
};

struct acg_ctx {
    // ---- ctx.cpp: the configuration and what acg_create derives from it, taps and stream map, the channels' device state, channel numbers
    acg_config cfg{};
    std::string err;
    bool tile_path = true;          // decim % 8 == 0 -> LDS-tiled kernel
    bool exact_fir = false;         // ACG_F_EXACT_FIR: the exact-order down-converter (verification mode)
    int lag_max = 1;                // most calls acg_collect_* may stay behind (what frame_cap was sized for)
    int ntaps_pad = 0;
    int max_len = 0;                // max_blocks * 1024
    size_t dm_pitch = 0;
    int bit_cap = 0;
    unsigned int frame_cap = 0;
    unsigned int per_call = 0;      // most blocks one process call can queue (what frame_cap was sized from)
    int msk_lpc = 8;                // lanes per channel in the MSK kernel
    int msk_high_prio = 1;
    int msk_split = 0;              // demodulator as wave pairs (msk2.hip)
    int msk_cus_default = 0;        // CUs reserved for the demodulator (0 = no partition)
    int pipe_blocks = 1;            // 1024-output blocks per pipelined chunk (0 = no pipelining)
    float* d_taps = nullptr;
    int* d_stream_of = nullptr;
    int4* d_groups = nullptr;       // shared-stream down-converter: <= 8 channels of one stream per group
    int* d_group_ch = nullptr;
    int ngroups = 0;                // 0: every stream feeds one channel (plain kernel)
    float* d_gtaps = nullptr;       // taps regrouped for the shared-stream kernel (lazily rebuilt)
    bool gtaps_dirty = true;
    void* d_mm_img = nullptr;       // matrix-pipe shared-stream kernel (fir_mm.hip): tap digits per group, MmChan per channel
    void* d_mm_chan = nullptr;
    size_t mm_img_bytes = 0;
    bool mm_dirty = true;
    void* d_mm1_img = nullptr;      // ... and per channel for the one-stream-per-channel kernel (fir_u8_mm1_kernel), made on first use
    bool mm1_dirty = true;
    bool stream_identity = true;        // channel c reads stream c
    AcgChan* d_st = nullptr;
    float* d_h = nullptr;
    double* d_sctab = nullptr;      // (cos, sin) table of the demodulator's mixer
    unsigned char* d_txt = nullptr;
    unsigned short* d_crctab = nullptr; // [256] + syndromes [1936] (ACG_F_REPAIR)
    float2* d_bits = nullptr;
    int* d_nbits = nullptr;
    unsigned long long* d_stamp = nullptr;   // measurement build (ACG_MSK_STAMP): per-wave phase cycle sums of the last demodulator launch
    std::vector<int> chnum;                 // acg_set_channel_numbers: the number handed out for each slot; empty = the slot's own
    int* d_chnum = nullptr;                 // ... on the device, for the sinks' passes and the flight table; null = identity
    // acg_set_input_rate: the rational window grid (fir_grid.h).  rate_hz == 0: integer windows, none of this is used
    unsigned int rate_hz = 0, rate_P = 0, rate_Q = 0;
    unsigned long long rate_k = 0;          // windows since acg_reset / acg_set_input_rate
    std::vector<unsigned int> rate_grid;    // floor(r P / Q), r <= Q ...
    unsigned int* d_rate_grid = nullptr;    // ... and on the device
    float* d_rate_tapsum = nullptr;         // [nch][4]: the taps' sums over [0, decim - 1) and [0, decim), re and im
    // acg_set_channel_filter: taps over long_nseg windows (fir_grid.h).  long_nseg == 0: off, none of this is used or allocated
    int long_nseg = 0;
    float* d_long_taps = nullptr;           // [nch][long_nseg * decim + 8][2], the last 8 of a channel zeros
    unsigned char* d_long_hist[2] = {};     // [nstreams] rows of the long_nseg - 1 windows before the next call's first sample, raw;
    size_t long_hist_pitch = 0;             // ... a call reads long_hist_cur and writes the other one behind its last launch
    int long_hist_cur = 0;
    int long_have = 0;                      // windows of that history that exist (0 after acg_reset / a change of rate, filter or format)
    int long_fmt = -1;                      // the format the history is in
    hipEvent_t long_hist_ev = nullptr;      // the history is written: the next call's launches wait for it, whatever their stream
    bool long_hist_ev_valid = false;

    // ---- process.cpp: streams and events of the pipeline, call slots, dm buffers and guards, the staging ring, launch timing
    hipStream_t stream = nullptr;
    hipStream_t msk_stream = nullptr;   // demodulator launches (they carry the channel state) run here, in order
    hipStream_t post_stream = nullptr;  // ACG_F_REPAIR: the block thread's pass over a call's blocks, OFF the demodulator's serial chain
    hipEvent_t msk_end[8] = {};         // per call slot: the call's last demodulator launch has finished
    hipEvent_t last_guard = nullptr;    // the dm guard recorded behind the newest demodulator launch of the call being issued (or none)
    hipEvent_t in_ev = nullptr;
    hipStream_t fir_stream = nullptr;   // CU partition: down-converter on the CUs the demodulator does not own
    hipEvent_t fir_in = nullptr, fir_out = nullptr;
    int fir_ncu = 0;
    std::vector<hipEvent_t> fir_done;   // per chunk slot: FIR of the slot finished (recorded on the caller's stream)
    hipEvent_t msk_go = nullptr;        // the demodulator stream has reached the launch of the newest chunk
    bool msk_go_valid = false;
    std::vector<hipEvent_t> msk_done;   // per chunk slot: MSK has consumed the slot's dm (recorded on msk_stream)
    std::vector<int> msk_done_owner;    // per dm block: index of the event its last reader recorded, -1 = none
    // per process call: frame-queue length at its end (pinned host word) + completion event
    static constexpr int NCALL = 8;
    hipEvent_t call_done[NCALL] = {};
    unsigned int* h_call_count = nullptr;   // pinned [NCALL]
    unsigned long long call_seq = 0;        // process calls issued
    unsigned int* d_call_count = nullptr;   // device view of h_call_count
    int last_len = 0;               // samples per channel of the last demod call
    int timing_mode = 0;            // 0 none, 1 both stages, 2 down-converter only (acg_set_timing)
    bool last_had_demod = false;
    float* d_dm = nullptr;          // dm buffer of the newest call (one of the two halves of d_dm_all)
    float* d_dm_all = nullptr;      // two dm buffers: the down-converter of call i+1 fills one while the demodulator of call i reads the other
    int dm_par = 0;
    int gbase = 0;                  // offset of the current buffer's guards in msk_done / msk_done_owner
    unsigned int* d_msk_done = nullptr;     // workgroups-finished counter of the demodulator kernel
    unsigned int* d_work = nullptr;     // FIR run dispensers, ACG_DISP_WORDS words per chunk slot
    unsigned int* d_rep_upto = nullptr; // blocks already through the repair kernel
    StageRing stage;                // the *_host entry points' staging buffers
    std::vector<EvPair> fir_ev, msk_ev;
    std::vector<hipEvent_t> ev_pool;

    // ---- results.cpp: the block ring's consumer, staging of frames, messages and labels, filter, flight table, statistics
    hipStream_t copy_stream = nullptr;  // result copies that must not queue behind running kernels
    unsigned int consumed = 0;              // frames already handed to the host (monotonic, wraps with the counter)
    AcgFrameRec* d_frames = nullptr;
    unsigned int* d_frame_count = nullptr;
    AcgFrameRec* h_stage = nullptr;         // host staging for acg_collect_frames / acg_drain_frames
    size_t h_stage_cap = 0;
    AcgMsgRec* d_msgs = nullptr;            // device + host staging for acg_collect_msgs / acg_drain_msgs
    AcgMsgRec* h_msgs = nullptr;
    size_t msgs_cap = 0;
    bool msg_filter_on = false;             // acg_set_msg_filter: the sink's filters (label.hip) run on every message entry point
    AcgLabelFilter msg_filter{};
    AcgMsgRec* d_kmsgs = nullptr;           // label.hip's output: the kept records, their labels decoded, their count
    acg_oooi* d_oooi = nullptr;
    acg_oooi* h_oooi = nullptr;
    unsigned int* d_kwork = nullptr;        // [kmsgs_cap / 256 + 1] per-workgroup counts, then the total
    size_t kmsgs_cap = 0;
    AcgFlights* flights = nullptr;          // acg_flights_enable: the flight table (flights.cpp), updated by every message entry point
    AcgReasm* reasm = nullptr;              // acg_reasm_enable: the reassembly table (reasm.hip), fed by every message entry point
    AcgChanStats* d_stats = nullptr;        // acg_stats_enable: the per-channel statistics (stats.hip), [nch]; null = off
    unsigned long long lost_blocks = 0;     // ... and the blocks lost to a lapped ring since the table was zeroed

    // ---- sinks.cpp: the batch sinks
    // three independent instances of one type: configuration, order, work space and what the legs rendered (outs.hip's sequence)
    struct AcgOutputs* text = nullptr;      // acg_text_enable: the text sink, one leg (text.hip)
    struct AcgOutputs* json = nullptr;      // acg_json_enable: the JSON sink, one leg (json.hip)
    struct AcgOutputs* outs = nullptr;      // acg_outputs_enable: up to ACG_OUT_LEGS_MAX legs rendered from one take
};

#define HIPCHK(ctx, call)                                                                  \
    do {                                                                                   \
        hipError_t e__ = (call);                                                           \
        if (e__ != hipSuccess) {                                                           \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e__);               \
            return ACG_EHIP;                                                               \
        }                                                                                  \
    } while (0)

// ctx.cpp: the error text of a context, and the code handed back
int fail(acg_ctx* ctx, int code, const char* msg);
// ctx.cpp: HIPCHK's text and code out of line, for units with many calls to check (HIPCHK builds its string at every site)
int hip_fail(acg_ctx* ctx, hipError_t e, const char* call);
#define HIPCHK_OL(ctx, call)                                                               \
    do {                                                                                   \
        const hipError_t e__ = (call);                                                     \
        if (e__ != hipSuccess) return hip_fail((ctx), e__, #call);                         \
    } while (0)
// ctx.cpp: zero device memory and make sure it has happened before any later launch on any stream
int zero_sync(acg_ctx* c, void* p, size_t bytes);
// ctx.cpp: the statistics table as acg_stats_enable (results.cpp) and acg_reset leave it
int stats_zero(acg_ctx* ctx);
// ctx.cpp: the text every window-aligned entry point refuses with while a rate is set
extern const char* const RATE_SET_MSG;

// results.cpp: a drain's `lag`
static constexpr int DRAIN = -1;
// results.cpp: what ring_upto finds and ring_claim works on
struct RingSpan {
    unsigned int upto = 0;          // where this collect / drain ends
    unsigned int live = 0;          // the device's count with every issued call finished, where ring_upto has waited for that (a drain; a
                                    // collect that may have been lapped); otherwise upto: nothing newer can have reached the consumer
    bool any = false;               // false: a collect with nothing pending (it returns ACG_OK at once)
};
// results.cpp: where a collect / drain ends
int ring_upto(acg_ctx* ctx, int lag, RingSpan* span);
// results.cpp: accounts what the device overwrote, then claims the oldest min(pending, max) blocks
int ring_claim(acg_ctx* ctx, const RingSpan& span, int max, unsigned int* pending, unsigned int* take);
// results.cpp: what the call returns once the claimed records are out
int ring_result(acg_ctx* ctx, int rc, unsigned int pending, unsigned int take, const char* again);
// results.cpp: the split's records, device and host, grown on demand
int grow_msg_stage(acg_ctx* ctx, unsigned int take);
// results.cpp: label.hip's output, grown on demand
int grow_label_stage(acg_ctx* ctx, unsigned int take);
// results.cpp: the flight table's pass over the imported events alone
int commit_imports(acg_ctx* ctx);
// results.cpp: the split of the `take` oldest blocks, label.hip's pass, the flight table's and the reassembly table's behind it
int launch_split(acg_ctx* ctx, unsigned int take, bool labels, unsigned int** d_total);
// results.cpp: the device form of a message filter
int label_filter_dev(const acg_msg_filter* f, AcgLabelFilter* d);

// sinks.cpp: frees a sink or the outputs (null: nothing)
void outputs_destroy(struct AcgOutputs* o);


// ---- what the lab entries below share: public records turned back into the device's form, staged, and label.hip's pass over them
// with no ring (the split has nothing to split) on the null stream.  Holds at most `cap` records per pass.
struct LabStage {
    const size_t nwg;                       // d_work: nwg per-workgroup counts, then the total
    std::vector<AcgMsgRec> h;
    AcgMsgRec *d_in = nullptr, *d_out = nullptr;    // the records staged; the records kept
    acg_oooi* d_oooi = nullptr;
    unsigned int* d_work = nullptr;
    bool allocated;

    explicit LabStage(size_t cap) : nwg(cap / 256 + 1), h(std::max<size_t>(cap, 1))
    {
        allocated = hipMalloc(&d_in, h.size() * sizeof(AcgMsgRec)) == hipSuccess && hipMalloc(&d_out, h.size() * sizeof(AcgMsgRec)) == hipSuccess &&
                    hipMalloc(&d_oooi, h.size() * sizeof(acg_oooi)) == hipSuccess && hipMalloc(&d_work, (nwg + 1) * sizeof(unsigned int)) == hipSuccess;
    }
    LabStage(const LabStage&) = delete;
    ~LabStage()
    {
        hipDeviceSynchronize();
        hipFree(d_in); hipFree(d_out); hipFree(d_oooi); hipFree(d_work);
    }
    bool ok() const { return allocated; }
    unsigned int* d_total() const { return d_work + nwg; }
    // h[0, n): `valid` is 1, or with from_reserved2 what the sink handed out in acg_msg's reserved2; soh_back is as given, or with
    // fill_soh_back the distance the public record's two sample counts span
    void stage(const acg_msg* in, unsigned int n, bool from_reserved2, bool fill_soh_back)
    {
        for (unsigned int i = 0; i < n; ++i) {
            std::memcpy(&h[i], &in[i], sizeof(AcgMsgRec));
            h[i].valid = from_reserved2 && in[i].reserved2 ? 0 : 1;
            if (fill_soh_back) h[i].soh_back = (int)(in[i].end_sample - in[i].soh_sample);
        }
    }
    // h[0, n) to the device and the label pass over them; 0, or anything else for a HIP error
    int label(unsigned int n, const AcgLabelFilter* f, unsigned char* d_keep = nullptr, const AcgFlightPass* flights = nullptr)
    {
        return upload(n) || launch(n, f, d_keep, flights);
    }
    // ... in two steps, for a caller that times the passes without the records' way to the device
    int upload(unsigned int n) { return hipMemcpy(d_in, h.data(), (size_t)n * sizeof(AcgMsgRec), hipMemcpyHostToDevice) != hipSuccess; }
    int launch(unsigned int n, const AcgLabelFilter* f, unsigned char* d_keep = nullptr, const AcgFlightPass* flights = nullptr)
    {
        const AcgLabelPass pass{f, d_work, d_out, d_oooi, d_total(), d_keep, flights};
        return acg_launch_msg_split(nullptr, 0, 0, n, d_in, nullptr, &pass) != 0;
    }
};
