// acg_api.cpp -- the C ABI of include/acarsdec_amd.h on top of the HIP kernels.
// Host runtime only: buffers, launches, result queues.  There is deliberately no CPU compute
// path here: without a GPU acg_create() fails with ACG_ENODEV.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "acarsdec_amd.h"
#include "acarsdec_amd_lab.h"
#include "fir_mm_plan.h"
#include "acg_internal.h"
#include "flights.h"

extern "C" void acg_host_msk_h(float* h);
extern "C" void acg_host_sincos_table(double* tab);
extern "C" float acg_host_level_db(double lvlsum, int bitcount);
extern "C" void acg_host_crc_tables(unsigned short* crc, unsigned short* synd);
extern "C" void acg_host_crc_tables_n(unsigned short* crc, unsigned short* synd, int nk);

extern char** environ;

namespace {

struct EvPair { hipEvent_t a, b; };

// ---- tuning overrides --------------------------------------------------------------------------------------------
// Every measurement / layout switch of the library (ACG_FIR_VARIANT, ACG_MSK_LPC, ACG_PIPE_BLOCKS, ...) lives in ONE table.
// A production process has an EMPTY table: a look-up is then one relaxed atomic load and returns the default -- no mutex,
// no string, no allocation on any launch path.  The table gets entries in two ways only:
//   * acg_tune(name, value) (bench.py --ab, the tests' `tune` fixture, the probes);
//   * the environment, read ONCE at the first look-up of the process and reported on stderr -- in the product library only
//     when ACG_ALLOW_TUNING=1 is set as well (a stray ACG_* variable of a host process is then named on stderr and ignored);
//     the lab build (libacarsdec_amd_lab.so, -DACG_LAB: tests and probes) always takes it.
// The measurement-only kernels and debug shapes (FIR variants other than 5 / 3, ACG_FIR_DEBUG_*, the two-wave demodulator)
// are not compiled into the product library at all.
std::mutex g_tune_mx;
std::map<std::string, std::string> g_tune;
std::atomic<int> g_tune_state{0};            // 0 = environment not looked at yet, 1 = table empty, 2 = table has entries

void tune_init_locked()
{
    if (g_tune_state.load(std::memory_order_relaxed) != 0) return;
    std::string seen;
    bool allow = false;
#ifdef ACG_LAB
    allow = true;
#endif
    for (char** e = environ; e && *e; ++e)
        if (std::strcmp(*e, "ACG_ALLOW_TUNING=1") == 0) allow = true;
    for (char** e = environ; e && *e; ++e) {
        const char* kv = *e;
        if (std::strncmp(kv, "ACG_", 4) != 0 || std::strncmp(kv, "ACG_BENCH_", 10) == 0 || std::strncmp(kv, "ACG_ALLOW_TUNING", 16) == 0) continue;
        const char* eq = std::strchr(kv, '=');
        if (!eq) continue;
        if (allow) g_tune[std::string(kv, (size_t)(eq - kv))] = std::string(eq + 1);
        seen += std::string(" ") + kv;
    }
    if (!seen.empty())
        std::fprintf(stderr, allow ? "acarsdec_amd: tuning overrides taken from the environment (measurement switches, not product "
                                     "configuration):%s\n"
                                   : "acarsdec_amd: ACG_* variables in the environment IGNORED (they are measurement switches; set "
                                     "ACG_ALLOW_TUNING=1 to apply them):%s\n", seen.c_str());
    g_tune_state.store(g_tune.empty() ? 1 : 2, std::memory_order_release);
}

// ---- roctx ranges (rocprofv3 --marker-trace): bound at run time, so the library carries no profiler dependency ----
typedef int (*roctx_push_fn)(const char*);
typedef int (*roctx_pop_fn)(void);
roctx_push_fn g_roctx_push = nullptr;
roctx_pop_fn g_roctx_pop = nullptr;
std::once_flag g_roctx_once;

void roctx_bind()
{
    // rocprofv3 --marker-trace preloads librocprofiler-sdk-roctx: its symbols are then in the global scope.  Otherwise
    // there is nobody to read the ranges and they cost nothing.
    g_roctx_push = (roctx_push_fn)dlsym(RTLD_DEFAULT, "roctxRangePushA");
    g_roctx_pop = (roctx_pop_fn)dlsym(RTLD_DEFAULT, "roctxRangePop");
    if (!g_roctx_push || !g_roctx_pop) g_roctx_push = nullptr, g_roctx_pop = nullptr;
}
struct RoctxRange {
    bool on;
    explicit RoctxRange(const char* name)
    {
        std::call_once(g_roctx_once, roctx_bind);
        on = g_roctx_push != nullptr;
        if (on) g_roctx_push(name);
    }
    ~RoctxRange() { if (on) g_roctx_pop(); }
};

}  // namespace

// look-up used by the launchers (fir.hip, msk.hip) and this file: the override's integer value, or dflt
extern "C" int acg_tune_get(const char* name, int dflt)
{
    if (g_tune_state.load(std::memory_order_acquire) == 1) return dflt;          // the production case: nothing to look up
    std::lock_guard<std::mutex> lk(g_tune_mx);
    tune_init_locked();
    if (g_tune.empty()) return dflt;
    auto it = g_tune.find(name);
    return it == g_tune.end() ? dflt : std::atoi(it->second.c_str());
}
extern "C" int acg_tune_has(const char* name)
{
    if (g_tune_state.load(std::memory_order_acquire) == 1) return 0;
    std::lock_guard<std::mutex> lk(g_tune_mx);
    tune_init_locked();
    return g_tune.count(name) ? 1 : 0;
}
extern "C" int acg_tune(const char* name, const char* value)
{
    if (!name || std::strncmp(name, "ACG_", 4) != 0) return ACG_EINVAL;
    std::lock_guard<std::mutex> lk(g_tune_mx);
    tune_init_locked();
    if (value) g_tune[name] = value;
    else g_tune.erase(name);
    g_tune_state.store(g_tune.empty() ? 1 : 2, std::memory_order_release);
    return ACG_OK;
}
// 1 in the lab build (libacarsdec_amd_lab.so: every kernel variant and debug shape), 0 in the product library
extern "C" int acg_is_lab_build(void)
{
#ifdef ACG_LAB
    return 1;
#else
    return 0;
#endif
}

struct acg_ctx {
    acg_config cfg{};
    std::string err;
    hipStream_t stream = nullptr;
    hipStream_t msk_stream = nullptr;   // demodulator launches (they carry the channel state) run here, in order
    hipStream_t copy_stream = nullptr;  // result copies that must not queue behind running kernels
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
    int pipe_blocks = 1;            // 1024-output blocks per pipelined chunk (0 = no pipelining)
    // per process call: frame-queue length at its end (pinned host word) + completion event
    static constexpr int NCALL = 8;
    hipEvent_t call_done[NCALL] = {};
    unsigned int* h_call_count = nullptr;   // pinned [NCALL]
    unsigned long long call_seq = 0;        // process calls issued
    unsigned int consumed = 0;              // frames already handed to the host (monotonic, wraps with the counter)
    bool tile_path = true;          // decim % 8 == 0 -> LDS-tiled kernel
    bool exact_fir = false;         // ACG_F_EXACT_FIR: the exact-order down-converter (verification mode)
    int lag_max = 1;                // most calls acg_collect_* may stay behind (what frame_cap was sized for)
    int ntaps_pad = 0;
    int max_len = 0;                // max_blocks * 1024
    size_t dm_pitch = 0;
    int bit_cap = 0;
    unsigned int frame_cap = 0;
    int last_len = 0;               // samples per channel of the last demod call
    int msk_lpc = 8;                // lanes per channel in the MSK kernel
    int msk_high_prio = 1;
    int msk_split = 0;              // demodulator as wave pairs (msk2.hip)
    int timing_mode = 0;            // 0 none, 1 both stages, 2 down-converter only (acg_set_timing)
    int msk_cus_default = 0;        // CUs reserved for the demodulator (0 = no partition)
    bool last_had_demod = false;

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
    float* d_dm = nullptr;          // dm buffer of the newest call (one of the two halves of d_dm_all)
    float* d_dm_all = nullptr;      // two dm buffers: the down-converter of call i+1 fills one while the demodulator of call i reads the other
    int dm_par = 0;
    int gbase = 0;                  // offset of the current buffer's guards in msk_done / msk_done_owner
    AcgChan* d_st = nullptr;
    float* d_h = nullptr;
    double* d_sctab = nullptr;      // (cos, sin) table of the demodulator's mixer
    unsigned char* d_txt = nullptr;
    AcgFrameRec* d_frames = nullptr;
    unsigned int* d_frame_count = nullptr;
    unsigned int* d_call_count = nullptr;   // device view of h_call_count
    unsigned int* d_msk_done = nullptr;     // workgroups-finished counter of the demodulator kernel
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
    struct AcgSinkState* text = nullptr;    // acg_text_enable: the text sink (text.hip), as json
    struct AcgSinkState* json = nullptr;    // acg_json_enable: the JSON sink (json.hip): configuration, work space, rendered lines
    std::vector<int> chnum;                 // acg_set_channel_numbers: the number handed out for each slot; empty = the slot's own
    int* d_chnum = nullptr;                 // ... on the device, for the sinks' passes and the flight table; null = identity
    AcgChanStats* d_stats = nullptr;        // acg_stats_enable: the per-channel statistics (stats.hip), [nch]; null = off
    unsigned long long lost_blocks = 0;     // ... and the blocks lost to a lapped ring since the table was zeroed
    unsigned int* d_work = nullptr;     // FIR run dispensers, ACG_DISP_WORDS words per chunk slot
    bool stream_identity = true;        // channel c reads stream c
    unsigned short* d_crctab = nullptr; // [256] + syndromes [1936] (ACG_F_REPAIR)
    unsigned int* d_rep_upto = nullptr; // blocks already through the repair kernel
    float2* d_bits = nullptr;
    int* d_nbits = nullptr;
    unsigned long long* d_stamp = nullptr;   // measurement build (ACG_MSK_STAMP): per-wave phase cycle sums of the last demodulator launch
    // *_host entry points: TWO device staging buffers and a copy stream of their own, so that the host-to-device copy of
    // call i+1 runs while the kernels of call i read the other buffer (the caller's memory is free again when the call
    // returns: rtl.c:314-330 / soapy.c:220-254 hand over a buffer that is only valid during the callback)
    void* d_stage[2] = {nullptr, nullptr};
    size_t stage_bytes = 0;         // bytes of EACH buffer
    hipStream_t h2d_stream = nullptr;
    hipEvent_t h2d_done = nullptr;
    hipEvent_t stage_free[2] = {nullptr, nullptr};   // the down-converter launches that read the buffer have been enqueued before it
    bool stage_free_valid[2] = {false, false};
    unsigned int stage_seq = 0;     // acg_process_iq_u8_host: calls so far (slot = seq & 1)
    int feed_cur = 0;               // acg_feed_samples_host: the buffer whose head holds the carried samples
    int feed_fmt = 0;               // acg_feed_samples_host: format and samples of the incomplete window carried
    size_t feed_fill = 0;

    std::vector<EvPair> fir_ev, msk_ev;
    std::vector<hipEvent_t> ev_pool;
};

#define HIPCHK(ctx, call)                                                                  \
    do {                                                                                   \
        hipError_t e__ = (call);                                                           \
        if (e__ != hipSuccess) {                                                           \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e__);               \
            return ACG_EHIP;                                                               \
        }                                                                                  \
    } while (0)

static int fail(acg_ctx* ctx, int code, const char* msg)
{
    if (ctx) ctx->err = msg;
    return code;
}

// zero device memory and make sure it has happened before any later launch on any stream
static int zero_sync(acg_ctx* c, void* p, size_t bytes)
{
    HIPCHK(c, hipMemset(p, 0, bytes));
    HIPCHK(c, hipDeviceSynchronize());
    return ACG_OK;
}

extern "C" const char* acg_version(void) { return "acarsdec_amd 0.1 (gfx950)"; }

extern "C" const char* acg_strerror(int code)
{
    switch (code) {
    case ACG_OK: return "ok";
    case ACG_EINVAL: return "invalid argument";
    case ACG_ENOMEM: return "out of memory";
    case ACG_EHIP: return "HIP runtime error";
    case ACG_ENODEV: return "no GPU available (this library has no CPU fallback)";
    case ACG_EOVERFLOW: return "output queue overflow";
    case ACG_ESTATE: return "bad call sequence";
    case ACG_EAGAIN: return "more results queued than fit: call again (nothing lost)";
    default: return "unknown error";
    }
}

extern "C" const char* acg_last_error(const acg_ctx* ctx) { return ctx ? ctx->err.c_str() : ""; }

extern "C" int acg_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static void sink_destroy(struct AcgSinkState* st);
static void free_all(acg_ctx* c)
{
    if (!c) return;
    hipFree(c->d_taps); hipFree(c->d_stream_of); hipFree(c->d_groups); hipFree(c->d_group_ch); hipFree(c->d_gtaps); hipFree(c->d_mm_img); hipFree(c->d_mm1_img); hipFree(c->d_mm_chan); hipFree(c->d_dm_all); hipFree(c->d_st);
    hipFree(c->d_h); hipFree(c->d_sctab); hipFree(c->d_txt); hipFree(c->d_frames); hipFree(c->d_frame_count);
    hipFree(c->d_stamp);
    hipFree(c->d_stats);
    hipFree(c->d_chnum);
    hipFree(c->d_msgs); std::free(c->h_msgs);
    hipFree(c->d_kmsgs); hipFree(c->d_oooi); hipFree(c->d_kwork); std::free(c->h_oooi);
    if (c->flights) acg_fl_destroy(c->flights);
    c->flights = nullptr;
    sink_destroy(c->json);
    c->json = nullptr;
    sink_destroy(c->text);
    c->text = nullptr;
    hipFree(c->d_bits); hipFree(c->d_nbits); hipFree(c->d_stage[0]); hipFree(c->d_stage[1]); hipFree(c->d_work); hipFree(c->d_msk_done); std::free(c->h_stage); hipFree(c->d_crctab); hipFree(c->d_rep_upto);
    for (auto& p : c->fir_ev) { hipEventDestroy(p.a); hipEventDestroy(p.b); }
    for (auto& p : c->msk_ev) { hipEventDestroy(p.a); hipEventDestroy(p.b); }
    for (auto e : c->ev_pool) hipEventDestroy(e);
    for (auto e : c->fir_done) hipEventDestroy(e);
    if (c->msk_go) hipEventDestroy(c->msk_go);
    for (auto e : c->msk_done) hipEventDestroy(e);
    for (auto e : c->call_done) if (e) hipEventDestroy(e);
    if (c->h_call_count) hipHostFree(c->h_call_count);
    if (c->in_ev) hipEventDestroy(c->in_ev);
    if (c->fir_in) hipEventDestroy(c->fir_in);
    if (c->fir_out) hipEventDestroy(c->fir_out);
    if (c->fir_stream) hipStreamDestroy(c->fir_stream);
    if (c->msk_stream) hipStreamDestroy(c->msk_stream);
    if (c->copy_stream) hipStreamDestroy(c->copy_stream);
    if (c->post_stream) hipStreamDestroy(c->post_stream);
    for (auto e : c->msk_end) if (e) hipEventDestroy(e);
    if (c->h2d_stream) hipStreamDestroy(c->h2d_stream);
    if (c->h2d_done) hipEventDestroy(c->h2d_done);
    for (auto e : c->stage_free) if (e) hipEventDestroy(e);
    if (c->stream) hipStreamDestroy(c->stream);
}

extern "C" void acg_destroy(acg_ctx* ctx)
{
    if (!ctx) return;
    hipSetDevice(ctx->cfg.device);
    hipDeviceSynchronize();
    free_all(ctx);
    delete ctx;
}

// Channel -> stream map, plus its inverse for the shared-stream down-converter: channels ordered by
// stream and cut into groups of <= 8 channels of one stream (rtl.c's shape: one dongle, several channels).
#ifndef ACG_FIR_MM1_DEFAULT
#define ACG_FIR_MM1_DEFAULT 0
#endif

static int upload_stream_map(acg_ctx* c, const int* so)
{
    const int nch = c->cfg.nch, ns = c->cfg.nstreams;
    HIPCHK(c, hipMemcpy(c->d_stream_of, so, (size_t)nch * sizeof(int), hipMemcpyHostToDevice));
    c->stream_identity = true;
    for (int i = 0; i < nch; ++i) c->stream_identity &= so[i] == i;
    std::vector<int> cnt((size_t)ns + 1, 0), ord((size_t)nch);
    for (int i = 0; i < nch; ++i) cnt[(size_t)so[i] + 1]++;
    bool shared = false;
    for (int s = 0; s < ns; ++s) {
        shared |= cnt[(size_t)s + 1] > 1;
        cnt[(size_t)s + 1] += cnt[(size_t)s];
    }
    c->ngroups = 0;
    c->gtaps_dirty = true;
    c->mm_dirty = true;
    if (!shared || !c->tile_path) return ACG_OK;
    std::vector<int> fill(cnt.begin(), cnt.end() - 1);
    for (int i = 0; i < nch; ++i) ord[(size_t)fill[(size_t)so[i]]++] = i;          // stable: ascending channel id per stream
    std::vector<int4> groups;
    for (int s = 0; s < ns; ++s)
        for (int f = cnt[(size_t)s]; f < cnt[(size_t)s + 1]; f += 8)
            groups.push_back(make_int4(s, f, std::min(8, cnt[(size_t)s + 1] - f), 0));
    HIPCHK(c, hipMemcpy(c->d_group_ch, ord.data(), (size_t)nch * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_groups, groups.data(), groups.size() * sizeof(int4), hipMemcpyHostToDevice));
    c->ngroups = (int)groups.size();
    if (!acg_tune_get("ACG_FIR_SHARED", 1)) c->ngroups = 0;
    // the matrix-pipe kernel's tap digits: 2 KiB per group and 32-byte k-step (26 KiB per group at rtlMult 200)
    const size_t need = acg_fir_mm_image_bytes(c->cfg.decim, c->ngroups);
    if (need > c->mm_img_bytes) {
        hipFree(c->d_mm_img);
        c->d_mm_img = nullptr;
        c->mm_img_bytes = 0;
        HIPCHK(c, hipMalloc(&c->d_mm_img, need));
        c->mm_img_bytes = need;
    }
    if (need && !c->d_mm_chan) HIPCHK(c, hipMalloc(&c->d_mm_chan, (size_t)nch * sizeof(MmChan)));
    return ACG_OK;
}

extern "C" int acg_create(acg_ctx** out, const acg_config* cfg)
{
    if (!out || !cfg) return ACG_EINVAL;
    *out = nullptr;
    if (cfg->nch < 1 || cfg->nstreams < 1 || cfg->nstreams > cfg->nch || cfg->decim < 1 ||
        cfg->decim > ACG_MAXDECIM_SAMPLES || cfg->ntaps < 1 || cfg->ntaps > cfg->decim || cfg->max_blocks < 1 ||
        cfg->max_lag < 0 || cfg->max_lag > acg_ctx::NCALL - 2)
        return ACG_EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || cfg->device < 0 || cfg->device >= ndev)
        return ACG_ENODEV;

    acg_ctx* c = new (std::nothrow) acg_ctx;
    if (!c) return ACG_ENOMEM;
    c->cfg = *cfg;
    c->tile_path = (cfg->decim % 8) == 0;
    c->ntaps_pad = c->tile_path ? ((cfg->ntaps + 7) & ~7) : cfg->ntaps;
    c->max_len = cfg->max_blocks * ACG_BLOCK;
    c->dm_pitch = ((size_t)c->max_len + 63) & ~(size_t)63;
    c->bit_cap = c->max_len / 4 + 8;
    // shortest possible block: SYN SYN SOH ETX CRC CRC + END byte = 56 bits ~ 291 samples.  The ring holds the worst case of
    // lag_max + 1 calls (a collect that stays `lag` calls behind leaves lag + 1 calls' blocks in it), so a host that
    // collects after every call can never be lapped.  acg_config.max_lag = 0: lag up to NCALL - 2 = 6 where that costs
    // <= 512 MiB (1024 channels x 8 callbacks: 66 MB for all seven), fewer calls for very wide contexts (16 384 channels
    // x 8 callbacks: three calls); a host that names its lag gets exactly that (lag 1: two calls' worth).
    {
        const unsigned long long per_call = (unsigned long long)cfg->nch * (unsigned long long)(c->max_len / 291 + 2);
        unsigned long long calls = (512ull << 20) / (per_call * sizeof(AcgFrameRec));
        calls = std::max<unsigned long long>(2, std::min<unsigned long long>(acg_ctx::NCALL - 1, calls));
        if (cfg->max_lag > 0) calls = (unsigned long long)cfg->max_lag + 1;       // the host says how far behind it collects
        if (per_call * calls > 0x80000000ull) { delete c; return ACG_EINVAL; }
        // The ring's length is a POWER OF TWO (the worst case rounded up): its 32-bit monotonic counters (device: frame_count,
        // the published per-call marks, the repair pass's mark; host: consumed) then index it consistently across their wrap at
        // 2^32 blocks -- 2^32 mod 2^k = 0, so slot(count) = count & (cap - 1) has no jump there, differences of counters are
        // wrap-safe as unsigned / signed 32-bit differences, and fetch's two-piece copy stays contiguous.  (Round 4 indexed
        // count % cap with cap = per_call * calls: at the wrap the slot sequence jumped and live records aliased -- 3 h away at
        // bench rates, VERDICT r04 weak 6.  tests/test_gpu_round5.py presets the counters to 2^32 - k through the lab hook.)
        // The rounding is kept INSIDE the budget where the host left the lag to the library (rounding the 512 MiB
        // worst case up could allocate close to 1 GiB): the largest power of two within 512 MiB, as many calls as fit into it
        // (at least two).  A host that names max_lag gets the smallest power of two that holds max_lag + 1 calls -- up to twice
        // that worst case (include/acarsdec_amd.h, acg_config.max_lag) -- and lag_max says what the ring it got really holds.
        unsigned long long cap2 = 1;
        if (cfg->max_lag > 0) {
            while (cap2 < per_call * calls) cap2 <<= 1;
        } else {
            while (cap2 * 2 * sizeof(AcgFrameRec) <= (512ull << 20)) cap2 <<= 1;
            while (cap2 / 2 >= per_call * (acg_ctx::NCALL - 1)) cap2 >>= 1;          // (no larger than seven calls need)
            while (cap2 < per_call * 2) cap2 <<= 1;                                   // (very wide contexts: two calls, whatever they cost)
        }
        if (cap2 > 0x80000000ull) { delete c; return ACG_EINVAL; }
        c->frame_cap = (unsigned int)cap2;
        c->lag_max = (int)std::min<unsigned long long>(acg_ctx::NCALL - 2, cap2 / per_call - 1);
    }
    c->exact_fir = (cfg->flags & ACG_F_EXACT_FIR) != 0;
    // MSK kernel shape: the chip has 1024 SIMDs; give every channel as many lanes as keeps the
    // wave count around one per SIMD (latency mode), down to one lane per channel (throughput mode)
    c->msk_lpc = cfg->nch <= 8192 ? 8 : cfg->nch <= 16384 ? 4 : cfg->nch <= 32768 ? 2 : 1;
    // pipeline chunk: 4 callbacks per launch pair.  Few large launches beat many small ones at every size
    // measured (1024 ... 16384 channels: launch tails, event packets); with the two dm buffers the chunks of a
    // call only serve to let its demodulator start before its down-converter has finished.  Up to 2048
    // channels even that is not worth a second pair: there the demodulator is the longer stage, the down-converter of call
    // i+1 hides under the demodulator of call i entirely, and every extra demodulator launch costs its prologue / epilogue
    // and the gap between two launches on the serial chain (0 = whole calls; 2048 channels, round 5: whole calls +3.5 ... +13 %
    // over chunks of 4 on two boxes, chunks of 2 -3 %: profiles/r05_shard2048_sweep.txt).
    c->pipe_blocks = cfg->nch <= 2048 ? 0 : 4;
    c->pipe_blocks = std::max(0, acg_tune_get("ACG_PIPE_BLOCKS", c->pipe_blocks));
    c->msk_high_prio = cfg->nch <= 8192 ? 1 : 0;   // <= 8192: its chain is the longer stage (neutral at 4096, +7 % at 8192)
    c->timing_mode = (cfg->flags & ACG_F_TIMING) ? 1 : 0;
    // few channels: the demodulator's serial chain is the critical path -> give its waves CUs of their own
    // (one wave per SIMD), the down-converter keeps the rest (it is HBM-bound and needs ~176 CUs to reach 0.75 of the spec).
    // Measured (profiles/r02_experiments/bench_variants.txt): the job gets faster as the demodulator's share grows past
    // the one-wave-per-SIMD minimum n -- 1024 channels (n = 32): 32 CUs 1.13 M, 64: 1.16, 80: 1.17, 96: 1.18 channel*Msps
    // while the down-converter still reaches 0.75 of the HBM spec on the other 176.  Round 4 gave 2048 channels (n = 64)
    // 128 CUs; round 5's sweep (profiles/r05_shard2048_sweep.txt), taken after the block repair stopped occupying the
    // demodulator's SIMDs for most of every call, has the optimum where the down-converter keeps its 176 CUs: 80 for the
    // demodulator (whole job 0.53 -> 0.61 on the same box together with whole-call launches; 96: 0.60, 112: 0.59, 160: 0.52).
    // So: 2.5 n, at most 80.
    if (cfg->nch <= 2048) {
        const int need = std::max(1, (cfg->nch * c->msk_lpc / 64 + 3) / 4);
        c->msk_cus_default = std::min(80, (5 * need + 1) / 2);
    }
    c->msk_high_prio = acg_tune_get("ACG_MSK_PRIO", c->msk_high_prio) ? 1 : 0;
    {
        const int v = acg_tune_get("ACG_MSK_LPC", c->msk_lpc);
        if (v == 1 || v == 2 || v == 4 || v == 8) c->msk_lpc = v;
    }

    int rc = ACG_OK;
    auto body = [&]() -> int {
        HIPCHK(c, hipSetDevice(cfg->device));
        int total_cus = 256;
        (void)hipDeviceGetAttribute(&total_cus, hipDeviceAttributeMultiprocessorCount, cfg->device);
        // CU masks are sized from the device's CU count (MI355X: 256 = 8 words; a part with 304 CUs: 10), never truncated
        const int mask_words = (std::max(1, total_cus) + 31) / 32;
        std::vector<uint32_t> full_mask((size_t)mask_words, 0u);
        for (int cu = 0; cu < total_cus; ++cu) full_mask[(size_t)(cu >> 5)] |= 1u << (cu & 31);
        HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        {
            // CU partition (ACG_MSK_CUS=n): the demodulator's few long-lived waves get n CUs of their own
            // (mask bits [0, n)) and the down-converter runs on the other 256 - n through an internal
            // stream that is ordered against the caller's stream by events.  Whatever physical CUs the
            // driver maps the bits to, the two masks are disjoint.
            int ncu = acg_tune_get("ACG_MSK_CUS", c->msk_cus_default);
            const int total = total_cus;
            // (streams made by hipExtStreamCreateWithCUMask have the default flags: they synchronise implicitly with the NULL
            //  stream.  A host that issues work on the NULL stream -- none of this library's entry points does -- serialises
            //  against them; there is no flag-taking variant of the call.  INTEGRATION.md says so.)
            if (ncu > 0 && ncu < total) {
                std::vector<uint32_t> mm((size_t)mask_words, 0u), fm((size_t)mask_words, 0u);
                for (int cu = 0; cu < total; ++cu) (cu < ncu ? mm : fm)[(size_t)(cu >> 5)] |= 1u << (cu & 31);
                HIPCHK(c, hipExtStreamCreateWithCUMask(&c->msk_stream, (uint32_t)mask_words, mm.data()));
                HIPCHK(c, hipExtStreamCreateWithCUMask(&c->fir_stream, (uint32_t)mask_words, fm.data()));
                HIPCHK(c, hipEventCreateWithFlags(&c->fir_in, hipEventDisableTiming));
                HIPCHK(c, hipEventCreateWithFlags(&c->fir_out, hipEventDisableTiming));
                c->fir_ncu = total - ncu;
                // Measurement switch ACG_POST_MASK=1: the block repair's stream on the DOWN-CONVERTER's side of the partition.
                // Without a mask its workgroups go where the most resources are free -- the demodulator's CUs -- and the pass
                // takes 78 / 97 us (1024 / 2048 channels) instead of 47 / 68 us with the mask, 3.8 / 3.1 % of the GPU time instead
                // of 2.3 / 2.2 % (not issue arbitration: raising the pass's wave priority changes nothing, GPU call 19).  But the
                // WHOLE JOB is faster without the mask -- 1.422 M against 1.418 M at 1024 channels, 0.611 against 0.591 of HBM at
                // 2048, two alternating runs each on one box (profiles/r05_post_mask_ab.txt) -- and the whole job is what a
                // host gets: no mask.
                if ((cfg->flags & ACG_F_REPAIR) && acg_tune_get("ACG_POST_MASK", 0))
                    HIPCHK(c, hipExtStreamCreateWithCUMask(&c->post_stream, (uint32_t)mask_words, fm.data()));
            } else {
                // a stream of its own priority class gets a hardware queue of its own
                int lo = 0, hi = 0;
                HIPCHK(c, hipDeviceGetStreamPriorityRange(&lo, &hi));
                // >= 16 384 channels the down-converter is the longer stage and the demodulator fills its gaps: there a queue of
                // the demodulator's own at NORMAL priority (a stream with a CU mask -- all CUs -- gets an HSA queue of its own
                // instead of one out of the runtime's shared pool) measured 2.7 % faster per call than the high-priority stream
                // (profiles/r04_context_probe.txt: 9.38 -> 9.13 ms; at 4096 channels the high-priority stream wins by 11 %)
                if (cfg->nch >= 16384) HIPCHK(c, hipExtStreamCreateWithCUMask(&c->msk_stream, (uint32_t)mask_words, full_mask.data()));
                else HIPCHK(c, hipStreamCreateWithPriority(&c->msk_stream, hipStreamNonBlocking, hi));
            }
        }
        // (round 4 tried a CU mask on this stream and on the repair stream -- the down-converter's side of the partition, to keep
        //  both off the demodulator's CUs: the runtime then performs the result copies as blit kernels on those saturated CUs,
        //  the host gets its results later and the headline lost 6-10 %: profiles/LEDGER.md)
        HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        HIPCHK(c, hipEventCreateWithFlags(&c->in_ev, hipEventDisableTiming));
        c->fir_done.resize((size_t)cfg->max_blocks);
        c->msk_done.resize(2 * (size_t)cfg->max_blocks);
        c->msk_done_owner.assign(2 * (size_t)cfg->max_blocks, -1);
        for (auto& e : c->fir_done) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->msk_go, hipEventDisableTiming));
        for (auto& e : c->msk_done) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        for (auto& e : c->call_done) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIPCHK(c, hipHostMalloc((void**)&c->h_call_count, sizeof(unsigned int) * acg_ctx::NCALL, hipHostMallocDefault));
        std::memset(c->h_call_count, 0, sizeof(unsigned int) * acg_ctx::NCALL);
        HIPCHK(c, hipHostGetDevicePointer((void**)&c->d_call_count, c->h_call_count, 0));
        HIPCHK(c, hipMalloc(&c->d_msk_done, sizeof(unsigned int)));
        HIPCHK(c, hipMemset(c->d_msk_done, 0, sizeof(unsigned int)));
        const size_t nch = (size_t)cfg->nch;
        HIPCHK(c, hipMalloc(&c->d_taps, nch * c->ntaps_pad * 2 * sizeof(float)));
        HIPCHK(c, hipMemset(c->d_taps, 0, nch * c->ntaps_pad * 2 * sizeof(float)));
        HIPCHK(c, hipMalloc(&c->d_stream_of, nch * sizeof(int)));
        HIPCHK(c, hipMalloc(&c->d_dm_all, 2 * nch * c->dm_pitch * sizeof(float)));
        c->d_dm = c->d_dm_all;
        HIPCHK(c, hipMalloc(&c->d_st, nch * sizeof(AcgChan)));
        HIPCHK(c, hipMalloc(&c->d_h, 136 * sizeof(float)));
        HIPCHK(c, hipMalloc(&c->d_txt, nch * 256));
        HIPCHK(c, hipMemset(c->d_txt, 0, nch * 256));
        HIPCHK(c, hipMalloc(&c->d_frames, (size_t)c->frame_cap * sizeof(AcgFrameRec)));
        HIPCHK(c, hipMalloc(&c->d_frame_count, sizeof(unsigned int)));
        HIPCHK(c, hipMemset(c->d_frame_count, 0, sizeof(unsigned int)));
        if (cfg->flags & ACG_F_BITLOG)
            HIPCHK(c, hipMalloc(&c->d_bits, nch * (size_t)c->bit_cap * sizeof(float2)));
        HIPCHK(c, hipMalloc(&c->d_nbits, nch * sizeof(int)));
#ifdef ACG_MSK_STAMP
        HIPCHK(c, hipMalloc(&c->d_stamp, (nch + 64) * 10 * sizeof(unsigned long long)));      // <= one wave per channel
        HIPCHK(c, hipMemset(c->d_stamp, 0, (nch + 64) * 10 * sizeof(unsigned long long)));
#endif
        HIPCHK(c, hipMalloc(&c->d_work, sizeof(unsigned int) * ACG_DISP_WORDS * (size_t)(cfg->max_blocks + 1)));
        HIPCHK(c, hipMemset(c->d_work, 0, sizeof(unsigned int) * ACG_DISP_WORDS * (size_t)(cfg->max_blocks + 1)));   // dispensers re-arm themselves
        HIPCHK(c, hipMemset(c->d_nbits, 0, nch * sizeof(int)));

        if (cfg->flags & ACG_F_REPAIR) {
            std::vector<unsigned short> tabs(256 + 8 * 243);          // one row beyond the reference's table, see host_setup.c
            acg_host_crc_tables_n(tabs.data(), tabs.data() + 256, 243);
            HIPCHK(c, hipMalloc(&c->d_crctab, tabs.size() * sizeof(unsigned short)));
            HIPCHK(c, hipMemcpy(c->d_crctab, tabs.data(), tabs.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
            HIPCHK(c, hipMalloc(&c->d_rep_upto, 2 * sizeof(unsigned int)));       // {blocks through the pass, workgroups finished}
            HIPCHK(c, hipMemset(c->d_rep_upto, 0, 2 * sizeof(unsigned int)));
            if (!c->post_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->post_stream, hipStreamNonBlocking));
            for (auto& e : c->msk_end) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        float h[136] = {0};
        acg_host_msk_h(h);                               // msk.c:44-48
        HIPCHK(c, hipMemcpy(c->d_h, h, sizeof(h), hipMemcpyHostToDevice));
        double sct[2 * ACG_SINCOS_N];
        acg_host_sincos_table(sct);                      // the mixer's cexp(-p*I), msk.c:86-91
        HIPCHK(c, hipMalloc(&c->d_sctab, sizeof(sct)));
        HIPCHK(c, hipMemcpy(c->d_sctab, sct, sizeof(sct), hipMemcpyHostToDevice));
        HIPCHK(c, hipMalloc(&c->d_groups, nch * sizeof(int4)));
        HIPCHK(c, hipMalloc(&c->d_group_ch, nch * sizeof(int)));
        HIPCHK(c, hipMalloc(&c->d_gtaps, nch * (size_t)c->ntaps_pad * 2 * sizeof(float)));
#ifdef ACG_LAB
        if (acg_tune_has("ACG_DEBUG_ADDR"))                    // placement probes (profiles/probe/placement_probe.py)
            fprintf(stderr, "acg_create: taps %p (%zu B)  dm %p (%zu B)  st %p  work %p  stream_of %p  txt %p\n", (void*)c->d_taps,
                    nch * c->ntaps_pad * 2 * sizeof(float), (void*)c->d_dm_all, 2 * nch * c->dm_pitch * sizeof(float), (void*)c->d_st,
                    (void*)c->d_work, (void*)c->d_stream_of, (void*)c->d_txt);
#endif
        std::vector<int> so(nch);
        for (size_t i = 0; i < nch; ++i) so[i] = (int)(i % (size_t)cfg->nstreams);
        return upload_stream_map(c, so.data());
    };
    rc = body();
    if (rc == ACG_OK) rc = acg_reset(c);
    if (rc != ACG_OK) {
        // keep the message reachable through a static for the failing create
        static thread_local std::string last;
        last = c->err;
        free_all(c);
        delete c;
        return rc;
    }
    *out = c;
    return ACG_OK;
}

// the statistics table as acg_stats_enable and acg_reset leave it: all zero (AcgChanStats: its "none yet" values are zeros)
static int stats_zero(acg_ctx* ctx)
{
    ctx->lost_blocks = 0;
    return zero_sync(ctx, ctx->d_stats, (size_t)ctx->cfg.nch * sizeof(AcgChanStats));
}

extern "C" int acg_reset(acg_ctx* ctx)
{
    if (!ctx) return ACG_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    ctx->consumed = 0;
    ctx->call_seq = 0;
    ctx->last_guard = nullptr;
    ctx->feed_fill = 0;
    ctx->feed_cur = 0;
    ctx->stage_seq = 0;
    ctx->stage_free_valid[0] = ctx->stage_free_valid[1] = false;
    std::fill(ctx->msk_done_owner.begin(), ctx->msk_done_owner.end(), -1);
    // initMsk (msk.c:34-41): MskPhi = MskClk = MskS = MskDf = idx = 0, inb zeroed;
    // static storage: MskLvlSum = MskBitCount = 0; initAcars (acars.c:230-234): outbits 0, nbits 8, WSYN
    std::vector<AcgChan> st((size_t)ctx->cfg.nch);
    std::memset(st.data(), 0, st.size() * sizeof(AcgChan));
    for (auto& s : st) s.nbits = 8;
    HIPCHK(ctx, hipMemcpy(ctx->d_st, st.data(), st.size() * sizeof(AcgChan), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemset(ctx->d_frame_count, 0, sizeof(unsigned int)));
    if (ctx->d_rep_upto) HIPCHK(ctx, hipMemset(ctx->d_rep_upto, 0, 2 * sizeof(unsigned int)));
    std::memset(ctx->h_call_count, 0, sizeof(unsigned int) * acg_ctx::NCALL);
    int zr = zero_sync(ctx, ctx->d_nbits, (size_t)ctx->cfg.nch * sizeof(int));
    if (zr != ACG_OK) return zr;
    ctx->last_len = 0;
    ctx->last_had_demod = false;
    if (ctx->flights && acg_fl_reset(ctx->flights) != ACG_OK) return fail(ctx, ACG_EHIP, "flight table reset");
    if (ctx->d_stats) return stats_zero(ctx);
    return ACG_OK;
}

extern "C" int acg_set_taps(acg_ctx* ctx, int ch0, int n, const float* taps)
{
    if (!ctx || !taps || ch0 < 0 || n < 1 || ch0 + n > ctx->cfg.nch) return ACG_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    const size_t src_pitch = (size_t)ctx->cfg.ntaps * 2 * sizeof(float);
    const size_t dst_pitch = (size_t)ctx->ntaps_pad * 2 * sizeof(float);
    HIPCHK(ctx, hipDeviceSynchronize());                 // down-converter launches run on the callers' streams
    HIPCHK(ctx, hipMemcpy2D(ctx->d_taps + (size_t)ch0 * ctx->ntaps_pad * 2, dst_pitch, taps, src_pitch,
                            src_pitch, (size_t)n, hipMemcpyHostToDevice));
    ctx->gtaps_dirty = true;
    ctx->mm_dirty = true;
    ctx->mm1_dirty = true;
    return ACG_OK;
}

extern "C" int acg_set_channel_streams(acg_ctx* ctx, const int* stream_of_channel)
{
    if (!ctx || !stream_of_channel) return ACG_EINVAL;
    for (int i = 0; i < ctx->cfg.nch; ++i)
        if (stream_of_channel[i] < 0 || stream_of_channel[i] >= ctx->cfg.nstreams)
            return fail(ctx, ACG_EINVAL, "stream index out of range");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    return upload_stream_map(ctx, stream_of_channel);
}

// ------------------------------------------------------------------------------------------
static int get_event(acg_ctx* c, hipEvent_t* e)
{
    if (!c->ev_pool.empty()) {
        *e = c->ev_pool.back();
        c->ev_pool.pop_back();
        return ACG_OK;
    }
    HIPCHK(c, hipEventCreate(e));
    return ACG_OK;
}

// dm guards: the demodulator launch that read dm block j last recorded msk_done[owner(j)] (one event
// per chunk; every record is on the in-order demodulator stream, so a newer record of the same event
// only makes a wait more conservative).  guard_wait makes stream s wait for the readers of blocks [j0, j1).
static int guard_wait(acg_ctx* ctx, hipStream_t s, int j0, int j1)
{
    int last = -1;
    for (int j = ctx->gbase + j0; j < ctx->gbase + j1; ++j) {
        const int o = ctx->msk_done_owner[(size_t)j];
        if (o >= 0 && o != last) {
            HIPCHK(ctx, hipStreamWaitEvent(s, ctx->msk_done[(size_t)o], 0));
            last = o;
        }
    }
    return ACG_OK;
}
static int guard_record(acg_ctx* ctx, int j0, int j1)
{
    HIPCHK(ctx, hipEventRecord(ctx->msk_done[(size_t)(ctx->gbase + j0)], ctx->msk_stream));
    ctx->last_guard = ctx->msk_done[(size_t)(ctx->gbase + j0)];          // (recorded right behind the newest demodulator launch)
    for (int j = ctx->gbase + j0; j < ctx->gbase + j1; ++j) ctx->msk_done_owner[(size_t)j] = ctx->gbase + j0;
    return ACG_OK;
}

// Every call that produces dm takes the other buffer: its down-converter launches then only have to wait for
// the demodulator launches of the call before the previous one.
static void begin_dm(acg_ctx* ctx)
{
    ctx->dm_par ^= 1;
    ctx->d_dm = ctx->d_dm_all + (size_t)ctx->dm_par * (size_t)ctx->cfg.nch * ctx->dm_pitch;
    ctx->gbase = ctx->dm_par * ctx->cfg.max_blocks;
}

// The down-converter's arguments that do not depend on the input format.  The caller adds its format's geometry; the
// pipeline adds the chunk (iq, dm, nwin, work_counter) and, on the partition's stream, ncu.
static FirArgs fir_args(const acg_ctx* c)
{
    const acg_config& g = c->cfg;
    FirArgs a{};
    a.stream_of = c->d_stream_of;
    a.taps = c->d_taps;
    a.dm_pitch = c->dm_pitch;
    a.nch = g.nch;
    a.decim = g.decim;
    a.ntaps_pad = c->ntaps_pad;
    a.ntaps = g.ntaps;
    a.stream_identity = c->stream_identity ? 1 : 0;
    // >= 16 384 channels: both stages share every CU and the down-converter is by far the longer one (+3..5 % whole job
    // at 16 384 channels).  Below that the starved demodulator becomes the longer stage: 8192 channels lose 7 % with the
    // raise, 4096 channels 15 % (profiles/r02_experiments/bench_variants.txt, "v_" rows).
    a.high_prio = (!c->fir_stream && g.nch >= 16384) ? 1 : 0;
    a.high_prio = acg_tune_get("ACG_FIR_PRIO", a.high_prio) ? 1 : 0;
    a.shares_cus = c->fir_stream ? 0 : 1;       // no CU partition: demodulator workgroups run on the same CUs
    return a;
}

// u8 I/Q input at iq_dev, rows pitch bytes apart
static FirArgs u8_args(const acg_ctx* c, const uint8_t* iq_dev, size_t pitch)
{
    FirArgs a = fir_args(c);
    a.iq = iq_dev;
    a.pitch = pitch;
    a.row_bytes = 2 * c->cfg.decim;
    // few channels: the demodulator's serial chain is the critical path; three resident workgroups per CU
    // cost the down-converter ~5 % of its bandwidth and give the demodulator waves ~10 % (whole job +5 %)
    a.wg_per_cu = (c->cfg.nch <= 2048 && c->msk_high_prio && !c->fir_stream) ? 3 : 0;
    a.wg_per_cu = acg_tune_get("ACG_FIR_WG_HINT", a.wg_per_cu);
    return a;
}

// Which u8 I/Q down-converter kernel takes the launch a (nwin, ncu set by the caller) on this context; fills in the arguments that
// kernel needs.  Changes nothing in the context: launch_fir_u8 launches what this says, acg_lab_fir_launch_shape reports it.
enum FirU8Kernel { FIR_U8_GENERIC, FIR_U8_DIRECT, FIR_U8_SHARED, FIR_U8_MM, FIR_U8_MM1 };
static FirU8Kernel fir_u8_kernel(const acg_ctx* c, FirArgs& a)
{
    const acg_config& g = c->cfg;
    a.nseg = 1;
    // verification mode: rtl.c:335-353 in the reference's own order of operations (fir.hip, fir_u8_generic_kernel)
    if (c->exact_fir || !c->tile_path) return FIR_U8_GENERIC;
    a.cpr = a.row_bytes / 16;
    a.row_stride = (a.cpr & 1) ? a.row_bytes : a.row_bytes + 16;
    a.cpr_magic = ((1u << 20) + (unsigned int)a.cpr - 1) / (unsigned int)a.cpr;
    const int ntile = a.nwin / ACG_TILE_WIN;
    int nseg = (4096 + g.nch - 1) / g.nch;          // aim at >= ~4096 workgroups
    nseg = std::max(1, std::min(nseg, ntile));
    a.nseg = nseg;
    a.groups = c->d_groups;
    a.group_ch = c->d_group_ch;
    a.ngroups = c->ngroups;
    a.gtaps = c->d_gtaps;
    a.mm_img = c->d_mm_img;
    a.mm_chan = c->d_mm_chan;
    // one stream per channel: the exact contraction with K = 1 takes the arithmetic off the vector pipe (fir_u8_mm1_kernel)
    if (c->ngroups == 0 && acg_tune_get("ACG_FIR_MM1", ACG_FIR_MM1_DEFAULT) && acg_fir_mm1_image_bytes(g.decim, 1) != 0) {
        // (its images are made at the first launch that wants them, launch_fir_u8: whether the kernel takes the shape does not
        //  depend on where they lie)
        FirArgs t = a;
        t.mm_img = c->d_mm1_img ? c->d_mm1_img : (const void*)c->d_taps;
        t.mm_chan = c->d_mm_chan ? c->d_mm_chan : (const void*)c->d_taps;
        if (acg_fir_mm1_takes(&t)) return FIR_U8_MM1;
    }
    // several channels per stream: the contraction goes to the matrix pipe (fir_mm.hip) where it takes the shape
    // (rtlMult 160 / 192 / 200, whole tiles), else to the vector-pipe kernel
    if (c->ngroups > 0 && acg_tune_get("ACG_FIR_MM", 1) && acg_fir_mm_takes(&a)) return FIR_U8_MM;
    return c->ngroups > 0 ? FIR_U8_SHARED : FIR_U8_DIRECT;
}

// The u8 I/Q down-converter kernel for this context, and the tap images it needs.  Returns what the kernel's launcher
// returned (a HIP error, 0 = launched), or ACG_EHIP with the text in c->err when a tap image could not be made.
static int launch_fir_u8(acg_ctx* c, FirArgs& a, hipStream_t s)
{
    const acg_config& g = c->cfg;
    int e;
    switch (fir_u8_kernel(c, a)) {
    case FIR_U8_GENERIC:
        return acg_launch_fir_generic(&a, s);
    case FIR_U8_MM1:
        if (!c->d_mm1_img) {
            HIPCHK(c, hipMalloc(&c->d_mm1_img, acg_fir_mm1_image_bytes(g.decim, g.nch)));
            c->mm1_dirty = true;
        }
        if (!c->d_mm_chan) HIPCHK(c, hipMalloc(&c->d_mm_chan, (size_t)g.nch * sizeof(MmChan)));
        a.mm_img = c->d_mm1_img;
        a.mm_chan = c->d_mm_chan;
        if (c->mm1_dirty) {
            if ((e = acg_launch_fir_mm1_prep(&a, s)) != 0) {
                c->err = std::string("tap digit launch: ") + hipGetErrorString((hipError_t)e);
                return ACG_EHIP;
            }
            c->mm1_dirty = false;
        }
        return acg_launch_fir_mm1(&a, s);
    case FIR_U8_MM:
        if (c->mm_dirty) {
            if ((e = acg_launch_fir_mm_prep(&a, s)) != 0) {
                c->err = std::string("tap digit launch: ") + hipGetErrorString((hipError_t)e);
                return ACG_EHIP;
            }
            c->mm_dirty = false;
        }
        return acg_launch_fir_mm(&a, s);
    case FIR_U8_SHARED:
    case FIR_U8_DIRECT:
        break;
    }
    if (c->ngroups > 0 && c->gtaps_dirty) {          // taps or the stream map changed (both synchronise the device)
        if ((e = acg_launch_regroup_taps(&a, s)) != 0) {
            c->err = std::string("tap regroup launch: ") + hipGetErrorString((hipError_t)e);
            return ACG_EHIP;
        }
        c->gtaps_dirty = false;
    }
    return c->ngroups > 0 ? acg_launch_fir_shared(&a, s) : acg_launch_fir(&a, s);
}

// One down-converter launch on stream s: launch(c, a, s) is the format's kernel choice (launch_fir_u8 or acg_launch_fir_fmt),
// bracketed by the timing pair (acg_set_timing) and a named range (rocprofv3 --marker-trace).
template <class Launch>
static int fir_launch(acg_ctx* c, FirArgs& a, hipStream_t s, Launch&& launch)
{
    const bool timing = c->timing_mode != 0;
    EvPair ev{};
    if (timing) {
        int r;
        if ((r = get_event(c, &ev.a)) != ACG_OK || (r = get_event(c, &ev.b)) != ACG_OK) return r;
        HIPCHK(c, hipEventRecord(ev.a, s));
    }
    int e;
    {
        RoctxRange range("acg:down-converter");
        e = launch(c, a, s);
    }
    if (e < 0) return e;                             // an ACG_* code: the text is in c->err
    if (e != 0) {
        c->err = std::string("FIR launch: ") + hipGetErrorString((hipError_t)e);
        return ACG_EHIP;
    }
    if (timing) {
        HIPCHK(c, hipEventRecord(ev.b, s));
        c->fir_ev.push_back(ev);
    }
    return ACG_OK;
}

static int launch_msk(acg_ctx* c, const float* dm_dev, size_t pitch_floats, int len, hipStream_t s, bool append = false)
{
    const acg_config& g = c->cfg;
    MskArgs a{};
    a.st = c->d_st;
    a.dm = dm_dev;
    a.dm_pitch = pitch_floats;
    a.h = c->d_h;
    a.sctab = c->d_sctab;
    a.txt = c->d_txt;
    a.frames = c->d_frames;
    a.frame_count = c->d_frame_count;
    a.frame_cap = c->frame_cap;
    a.bits = c->d_bits;
    a.nbits_out = c->d_nbits;
    a.bit_cap = c->bit_cap;
    a.nch = g.nch;
    a.len = len;
    a.bit_append = append ? 1 : 0;
    a.high_prio = c->msk_high_prio;
    a.waves_per_group = c->fir_stream ? 4 : 1;
    a.snap = c->d_call_count + (c->call_seq % acg_ctx::NCALL);
    a.done_ctr = c->d_msk_done;
    a.dm_vec_ok = ((((uintptr_t)dm_dev) & 15) == 0 && (pitch_floats % 4) == 0) ? 1 : 0;
    a.stamp = c->d_stamp;
    a.precise_mixer = (g.flags & ACG_F_PRECISE_MIXER) ? 1 : 0;
    const bool timing = c->timing_mode == 1;
    EvPair ev{};
    if (timing) {
        int r;
        if ((r = get_event(c, &ev.a)) != ACG_OK || (r = get_event(c, &ev.b)) != ACG_OK) return r;
        HIPCHK(c, hipEventRecord(ev.a, s));
    }
    int lpc = c->msk_lpc;
    {                                                               // measurement aid: lanes per channel per launch (the channel state
        const int v = acg_tune_get("ACG_MSK_LPC_LIVE", lpc);          // does not depend on it), for same-context A/B (bench.py --ab)
        if (v == 1 || v == 2 || v == 4 || v == 8) lpc = v;
    }
    int e;
    {
        RoctxRange range("acg:demodulator");
        // lab build: the two-wave kernel (msk2.hip: the per-bit instruction stream split over a wave pair on two SIMDs);
        // bit-identical to the one-wave kernel, so the switch may change from launch to launch -- and slower
#ifdef ACG_LAB
        if (lpc == 8 && acg_tune_get("ACG_MSK_SPLIT", c->msk_split)) e = acg_launch_msk2(&a, c->fir_stream ? 2 : 1, s);
        else
#endif
            e = acg_launch_msk(&a, lpc, s);
    }
    if (e != 0) {
        c->err = std::string("MSK launch: ") + hipGetErrorString((hipError_t)e);
        return ACG_EHIP;
    }
    if (timing) {
        HIPCHK(c, hipEventRecord(ev.b, s));
        c->msk_ev.push_back(ev);
    }
    c->last_len = len;
    c->last_had_demod = true;
    return ACG_OK;
}

static int check_iq_args(acg_ctx* ctx, const void* p, size_t pitch, int nblocks)
{
    if (!ctx || !p) return ACG_EINVAL;
    if (nblocks < 1 || nblocks > ctx->cfg.max_blocks) return fail(ctx, ACG_EINVAL, "nblocks out of range");
    if (ctx->cfg.decim > ACG_MAXDECIM) return fail(ctx, ACG_EINVAL, "u8 I/Q path: decim above RTLMULTMAX (rtl.c:39)");
    const size_t row = (size_t)nblocks * ACG_BLOCK * ctx->cfg.decim * 2;
    if (ctx->cfg.nstreams > 1 && pitch < row) return fail(ctx, ACG_EINVAL, "pitch smaller than a row");
    return ACG_OK;
}

// ... of device input, which the tiled kernels read in 16-byte chunks
static int check_iq_dev_args(acg_ctx* ctx, const uint8_t* iq_dev, size_t pitch, int nblocks)
{
    const int r = check_iq_args(ctx, iq_dev, pitch, nblocks);
    if (r == ACG_OK && ctx->tile_path && (((uintptr_t)iq_dev | pitch) & 15))
        return fail(ctx, ACG_EINVAL, "I/Q base and pitch must be 16-byte aligned");
    return r;
}

extern "C" int acg_fir_only_dev(acg_ctx* ctx, const uint8_t* iq_dev, size_t pitch_bytes, int nblocks,
                                void* hip_stream)
{
    int r = check_iq_dev_args(ctx, iq_dev, pitch_bytes, nblocks);
    if (r != ACG_OK) return r;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
    begin_dm(ctx);
    if ((r = guard_wait(ctx, s, 0, nblocks)) != ACG_OK) return r;
    FirArgs a = u8_args(ctx, iq_dev, pitch_bytes);
    a.shares_cus = 0;                               // no demodulator launch runs beside it
    a.dm = ctx->d_dm;
    a.nwin = nblocks * ACG_BLOCK;
    a.work_counter = ctx->d_work;
    r = fir_launch(ctx, a, s, launch_fir_u8);
    if (r == ACG_OK) ctx->last_len = nblocks * ACG_BLOCK;
    return r;
}

// Start of a process call.  The call's slot of the NCALL-deep ring (its mark word in host-mapped memory, its events) was used
// by the call NCALL calls ago: that one must have finished COMPLETELY -- including its repair pass, which reads the mark word --
// before this call's demodulator publishes into the word (a host that streams without collecting could otherwise
// get a repair pass that reads a later call's mark).  The event has normally completed long ago: one query.
static int begin_call(acg_ctx* ctx)
{
    ctx->last_guard = nullptr;          // only ever a guard recorded in THIS call (a call that failed after guard_record leaves one behind: ADVICE r05)
    if (ctx->call_seq >= (unsigned long long)acg_ctx::NCALL)
        HIPCHK(ctx, hipEventSynchronize(ctx->call_done[ctx->call_seq % acg_ctx::NCALL]));
    return ACG_OK;
}

// Marks the end of one process call on the demodulator stream: the frame-queue length at that
// point goes to a pinned host word, followed by an event.
static int end_of_call(acg_ctx* ctx)
{
    const int slot = (int)(ctx->call_seq % acg_ctx::NCALL);
    // the queue length of this call was published by its last demodulator launch (MskArgs::snap)
    if (ctx->d_crctab) {
        // ACG_F_REPAIR: the block thread's work (acars.c:93-215) on what this call queued -- on a stream of its OWN, behind the
        // call's last demodulator launch: the demodulator of the next call does not wait for it (on its stream the pass sat on
        // the serial chain that sets the step at <= 2048 channels and cost 30 % of the headline: profiles/LEDGER.md round 4).
        // The pass ends at the call's published queue length, not at the live counter the next call is already moving.
        // (the dm guard recorded behind the call's last demodulator launch is that very point of the stream: no second record)
        if (ctx->last_guard) {
            HIPCHK(ctx, hipStreamWaitEvent(ctx->post_stream, ctx->last_guard, 0));
        } else {
            HIPCHK(ctx, hipEventRecord(ctx->msk_end[slot], ctx->msk_stream));
            HIPCHK(ctx, hipStreamWaitEvent(ctx->post_stream, ctx->msk_end[slot], 0));
        }
        const int e = acg_launch_blk_repair(ctx->d_frames, ctx->frame_cap, ctx->d_call_count + slot, ctx->d_rep_upto, ctx->d_rep_upto + 1,
                                            ctx->d_crctab + 256, ctx->d_crctab, ctx->cfg.nch, ctx->post_stream);
        if (e != 0) return fail(ctx, ACG_EHIP, "block repair launch failed");
        HIPCHK(ctx, hipEventRecord(ctx->call_done[slot], ctx->post_stream));
    } else {
        HIPCHK(ctx, hipEventRecord(ctx->call_done[slot], ctx->msk_stream));
    }
    ctx->last_guard = nullptr;
    ctx->call_seq++;
    return ACG_OK;
}

// Software pipeline of one process call over nwin windows of input at a.iq (win_bytes per window and plane), in chunks of
// chunk_win windows; launch is the input format's down-converter (see fir_launch).  The (bandwidth-bound, wide)
// down-converter chunks run on the CALLER's stream: they are the only consumers of the input, so whatever the caller
// enqueues next on that stream (refilling the buffer, the next call) is ordered correctly.  The (latency-bound,
// narrow) demodulator chunks run in order on the context's own stream -- they carry the
// channel state -- each waiting for its chunk of dm.  A dm chunk slot is rewritten by the
// next call only after the demodulator launch that read it has finished.  So FIR(k+1) overlaps
// MSK(k) inside a call, and FIR of call i+1 overlaps the MSK tail of call i.
template <class Launch>
static int run_pipeline(acg_ctx* ctx, hipStream_t caller, FirArgs& a, size_t win_bytes, int nwin, int chunk_win, Launch&& launch)
{
    int r;
    if ((r = begin_call(ctx)) != ACG_OK) return r;
    begin_dm(ctx);
    hipStream_t s = caller;
    if (ctx->fir_stream) {
        // CU partition: the down-converter runs on its own masked stream, ordered after what the caller
        // has enqueued so far (the input is ready) ...
        s = ctx->fir_stream;
        HIPCHK(ctx, hipEventRecord(ctx->fir_in, caller));
        HIPCHK(ctx, hipStreamWaitEvent(s, ctx->fir_in, 0));
        a.ncu = ctx->fir_ncu;
    }
    // dispatch order: the demodulator launch of the previous chunk goes to the chip BEFORE this
    // down-converter launch floods it (otherwise its few long-lived waves are placed into whatever the
    // persistent workgroups left over and run ~20 % slower): wait until the demodulator stream has
    // reached that launch.  Costs one cross-queue signal per chunk; the down-converter is then at
    // most two chunks ahead, which is all the run-ahead the pipeline needs.
    // (with a CU partition the two stages cannot take each other's CUs: no ordering of the dispatches is needed, and the
    //  demodulator's serial chain is spared one barrier packet per launch -- every packet between two of its kernels is
    //  ~7 us during which the stage that sets the step stands still)
    const bool order_dispatch = ctx->fir_stream == nullptr;
    const uint8_t* iq0 = a.iq;
    int k = 0;
    for (int w0 = 0; w0 < nwin; w0 += chunk_win, ++k) {
        const int nw = std::min(chunk_win, nwin - w0);
        const int j0 = w0 / ACG_BLOCK;
        const int j1 = std::min(ctx->cfg.max_blocks, (w0 + nw + ACG_BLOCK - 1) / ACG_BLOCK);
        // dm blocks [j0, j1) may still be read by demodulator launches of the previous call
        if ((r = guard_wait(ctx, s, j0, j1)) != ACG_OK) return r;
        if (order_dispatch && ctx->msk_go_valid) HIPCHK(ctx, hipStreamWaitEvent(s, ctx->msk_go, 0));
        a.iq = iq0 + (size_t)w0 * win_bytes;
        a.dm = ctx->d_dm + w0;
        a.nwin = nw;
        a.work_counter = ctx->d_work + (size_t)ACG_DISP_WORDS * j0;     // one dispenser per chunk slot
        if ((r = fir_launch(ctx, a, s, launch)) != ACG_OK) return r;
        HIPCHK(ctx, hipEventRecord(ctx->fir_done[(size_t)k], s));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->msk_stream, ctx->fir_done[(size_t)k], 0));
        if (order_dispatch) {
            HIPCHK(ctx, hipEventRecord(ctx->msk_go, ctx->msk_stream));
            ctx->msk_go_valid = true;
        }
        if ((r = launch_msk(ctx, ctx->d_dm + w0, ctx->dm_pitch, nw, ctx->msk_stream, w0 > 0)) != ACG_OK) return r;
        if ((r = guard_record(ctx, j0, j1)) != ACG_OK) return r;
    }
    if (ctx->fir_stream) {
        // ... and whatever the caller enqueues next on its stream (refilling the input) waits for the
        // last down-converter launch of this call
        HIPCHK(ctx, hipEventRecord(ctx->fir_out, s));
        HIPCHK(ctx, hipStreamWaitEvent(caller, ctx->fir_out, 0));
    }
    ctx->last_len = nwin;
    return end_of_call(ctx);
}

extern "C" int acg_process_iq_u8_dev(acg_ctx* ctx, const uint8_t* iq_dev, size_t pitch_bytes, int nblocks,
                                     void* hip_stream)
{
    int r = check_iq_dev_args(ctx, iq_dev, pitch_bytes, nblocks);
    if (r != ACG_OK) return r;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    int cb = acg_tune_get("ACG_PIPE_BLOCKS_LIVE", ctx->pipe_blocks);      // (per call: same-context A/B of the chunk size)
    if (cb <= 0 || cb > nblocks) cb = nblocks;
    FirArgs a = u8_args(ctx, iq_dev, pitch_bytes);
    return run_pipeline(ctx, hip_stream ? (hipStream_t)hip_stream : ctx->stream, a, (size_t)a.row_bytes, nblocks * ACG_BLOCK,
                        cb * ACG_BLOCK, launch_fir_u8);
}

static int ensure_stage(acg_ctx* c, size_t bytes)
{
    if (!c->h2d_stream) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->h2d_stream, hipStreamNonBlocking));
        HIPCHK(c, hipEventCreateWithFlags(&c->h2d_done, hipEventDisableTiming));
        for (auto& e : c->stage_free) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    if (c->stage_bytes >= bytes) return ACG_OK;
    if (c->feed_fill) return fail(c, ACG_ESTATE, "staging buffers cannot grow while a partial window is carried");
    HIPCHK(c, hipDeviceSynchronize());                    // nothing may still read the buffers that go away
    for (auto& p : c->d_stage) {
        if (p) hipFree(p);
        p = nullptr;
    }
    c->stage_bytes = 0;
    c->stage_free_valid[0] = c->stage_free_valid[1] = false;
    c->feed_cur = 0;
    for (auto& p : c->d_stage) HIPCHK(c, hipMalloc(&p, bytes));
    c->stage_bytes = bytes;
    return ACG_OK;
}

// Host input: the copy of THIS call goes to the staging buffer the call before the previous one used, on the copy stream,
// as soon as the down-converter launches that read that buffer are done -- i.e. it runs beside the kernels of the previous
// call.  The call returns when the copy has left the caller's memory (rtl.c:314-330: the buffer belongs to the driver
// again after the callback); its kernels run after the return, beside the host's next call.  From pinned memory
// (acg_host_alloc / acg_host_register) the copy is one DMA at the link's rate; from pageable memory the runtime stages it.
extern "C" int acg_process_iq_u8_host(acg_ctx* ctx, const uint8_t* iq_host, size_t pitch_bytes, int nblocks)
{
    int r = check_iq_args(ctx, iq_host, pitch_bytes, nblocks);
    if (r != ACG_OK) return r;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    const size_t row = (size_t)nblocks * ACG_BLOCK * ctx->cfg.decim * 2;
    const size_t dpitch = (row + 15) & ~(size_t)15;
    const size_t max_row = (((size_t)ctx->cfg.max_blocks * ACG_BLOCK * ctx->cfg.decim * 2) + 15) & ~(size_t)15;
    // (acg_feed_samples_host keeps the samples of an incomplete window at the head of the same staging buffers)
    if (ctx->feed_fill) return fail(ctx, ACG_ESTATE, "acg_feed_samples_host is carrying a partial window in the staging buffers (acg_reset drops it)");
    if ((r = ensure_stage(ctx, max_row * ctx->cfg.nstreams)) != ACG_OK) return r;
    const int slot = (int)(ctx->stage_seq++ & 1u);
    if (ctx->stage_free_valid[slot]) HIPCHK(ctx, hipStreamWaitEvent(ctx->h2d_stream, ctx->stage_free[slot], 0));
    HIPCHK(ctx, hipMemcpy2DAsync(ctx->d_stage[slot], dpitch, iq_host, ctx->cfg.nstreams > 1 ? pitch_bytes : row,
                                 row, (size_t)ctx->cfg.nstreams, hipMemcpyHostToDevice, ctx->h2d_stream));
    HIPCHK(ctx, hipEventRecord(ctx->h2d_done, ctx->h2d_stream));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->h2d_done, 0));
    r = acg_process_iq_u8_dev(ctx, (const uint8_t*)ctx->d_stage[slot], dpitch, nblocks, nullptr);
    if (r != ACG_OK) {
        (void)hipEventSynchronize(ctx->h2d_done);           // the copy may still be reading the caller's buffer: not after we return
        return r;
    }
    // (the context's stream is ordered behind the call's last down-converter launch, whichever stream that ran on)
    HIPCHK(ctx, hipEventRecord(ctx->stage_free[slot], ctx->stream));
    ctx->stage_free_valid[slot] = true;
    HIPCHK(ctx, hipEventSynchronize(ctx->h2d_done));       // the caller's buffer is free again
    return ACG_OK;
}

extern "C" int acg_process_dm_dev(acg_ctx* ctx, const float* dm_dev, size_t pitch_floats, int len,
                                  void* hip_stream)
{
    if (!ctx || !dm_dev) return ACG_EINVAL;
    if (len < 0 || len > ctx->max_len) return fail(ctx, ACG_EINVAL, "len out of range");
    if (ctx->cfg.nch > 1 && pitch_floats < (size_t)len) return fail(ctx, ACG_EINVAL, "pitch smaller than len");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
    { const int br = begin_call(ctx); if (br != ACG_OK) return br; }
    HIPCHK(ctx, hipEventRecord(ctx->in_ev, s));                       // dm produced on the caller's stream
    HIPCHK(ctx, hipStreamWaitEvent(ctx->msk_stream, ctx->in_ev, 0));
    int r = launch_msk(ctx, dm_dev, pitch_floats, len, ctx->msk_stream);
    if (r != ACG_OK) return r;
    // the demodulator is the only reader of dm_dev: whatever the caller enqueues next on its stream
    // (refilling the buffer in place) is ordered behind it, the same contract as the iq entry points
    HIPCHK(ctx, hipEventRecord(ctx->in_ev, ctx->msk_stream));
    HIPCHK(ctx, hipStreamWaitEvent(s, ctx->in_ev, 0));
    return end_of_call(ctx);
}

extern "C" int acg_process_dm_host(acg_ctx* ctx, const float* dm_host, size_t pitch_floats, int len)
{
    if (!ctx || !dm_host) return ACG_EINVAL;
    if (len < 0 || len > ctx->max_len) return fail(ctx, ACG_EINVAL, "len out of range");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    { const int br = begin_call(ctx); if (br != ACG_OK) return br; }
    if (len > 0) {
        const size_t rowb = (size_t)len * sizeof(float);
        HIPCHK(ctx, hipMemcpy2DAsync(ctx->d_dm, ctx->dm_pitch * sizeof(float), dm_host,
                                     (ctx->cfg.nch > 1 ? pitch_floats : (size_t)len) * sizeof(float), rowb,
                                     (size_t)ctx->cfg.nch, hipMemcpyHostToDevice, ctx->msk_stream));
    }
    int r = launch_msk(ctx, ctx->d_dm, ctx->dm_pitch, len, ctx->msk_stream);
    if (r != ACG_OK) return r;
    if (len > 0 && (r = guard_record(ctx, 0, std::min(ctx->cfg.max_blocks, (len + ACG_BLOCK - 1) / ACG_BLOCK))) != ACG_OK) return r;
    return end_of_call(ctx);
}

// ---- the 12.5 kHz front ends (soundfile.c, alsa.c): interleaved PCM frames, all channels in one call ----
static size_t pcm_elem(int fmt) { return fmt == ACG_PCM_S16 ? 2 : 4; }

static int check_pcm_args(acg_ctx* ctx, int fmt, const void* frames)
{
    if (!ctx || !frames) return ACG_EINVAL;
    if (fmt != ACG_PCM_S16 && fmt != ACG_PCM_F32) return fail(ctx, ACG_EINVAL, "unknown PCM format");
    if (((uintptr_t)frames) & 3) return fail(ctx, ACG_EINVAL, "PCM frames must be 4-byte aligned");
    if (!acg_launch_pcm_deint) return fail(ctx, ACG_ESTATE, "this build has no PCM unit");
    return ACG_OK;
}

static int launch_pcm(acg_ctx* ctx, int fmt, const void* frames_dev, int nframes, float* dm, size_t pitch, hipStream_t s)
{
    PcmArgs p{frames_dev, dm, pitch, ctx->cfg.nch, nframes, fmt};
    RoctxRange range("acg:pcm-deinterleave");
    const int e = acg_launch_pcm_deint(&p, s);
    if (e != 0) {
        ctx->err = std::string("PCM de-interleave launch: ") + hipGetErrorString((hipError_t)e);
        return ACG_EHIP;
    }
    return ACG_OK;
}

// acg_process_dm_host with the copy replaced by the de-interleave kernel: it fills the context's dm image, the demodulator
// follows on its own stream, and the guard record is the same.  The kernel is the only reader of frames_dev and runs on the
// CALLER's stream, behind the guards of the image: what the caller enqueues next is ordered behind it and does not wait for the
// demodulator.  (Launched on the demodulator's stream instead -- in order there, no guard needed -- the kernel cost the same,
// but the demodulator launch behind it took 1.81 ms instead of 1.20 ms at 16 384 channels x 8192 frames, with or without a
// host synchronise between the two; at 4096 channels nothing: profiles/LEDGER.md, "12.5 kHz PCM front end".)
extern "C" int acg_process_pcm_dev(acg_ctx* ctx, int fmt, const void* frames_dev, int nframes, void* hip_stream)
{
    int r = check_pcm_args(ctx, fmt, frames_dev);
    if (r != ACG_OK) return r;
    if (nframes < 0 || nframes > ctx->max_len) return fail(ctx, ACG_EINVAL, "nframes out of range");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
    if ((r = begin_call(ctx)) != ACG_OK) return r;
    if (nframes > 0) {
        // the dm image may still be read by the demodulator launch of the call before (the guard acg_process_dm_host and the
        // pipeline record); then the kernel, on the CALLER's stream like the down-converter's chunks
        const int nb = std::min(ctx->cfg.max_blocks, (nframes + ACG_BLOCK - 1) / ACG_BLOCK);
        if ((r = guard_wait(ctx, s, 0, nb)) != ACG_OK) return r;
        if ((r = launch_pcm(ctx, fmt, frames_dev, nframes, ctx->d_dm, ctx->dm_pitch, s)) != ACG_OK) return r;
        HIPCHK(ctx, hipEventRecord(ctx->in_ev, s));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->msk_stream, ctx->in_ev, 0));
    }
    if ((r = launch_msk(ctx, ctx->d_dm, ctx->dm_pitch, nframes, ctx->msk_stream)) != ACG_OK) return r;
    if (nframes > 0 && (r = guard_record(ctx, 0, std::min(ctx->cfg.max_blocks, (nframes + ACG_BLOCK - 1) / ACG_BLOCK))) != ACG_OK) return r;
    return end_of_call(ctx);
}

// Host frames of any count: chunks of at most max_len frames, each ONE contiguous copy into the staging buffer the chunk before
// the previous one used (acg_process_iq_u8_host's scheme: the copy of chunk k + 1 runs beside the kernels of chunk k), then the
// device path.  Returns when the last copy has left the caller's buffer.
extern "C" int acg_feed_pcm_host(acg_ctx* ctx, int fmt, const void* frames, size_t nframes)
{
    int r = check_pcm_args(ctx, fmt, frames);
    if (r != ACG_OK) return r;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    if (ctx->feed_fill) return fail(ctx, ACG_ESTATE, "acg_feed_samples_host is carrying a partial window in the staging buffers (acg_reset drops it)");
    if (nframes == 0) return acg_process_pcm_dev(ctx, fmt, frames, 0, nullptr);
    const size_t fb = (size_t)ctx->cfg.nch * pcm_elem(fmt);          // bytes per frame
    if ((r = ensure_stage(ctx, ((size_t)ctx->max_len * fb + 3) & ~(size_t)3)) != ACG_OK) return r;
    for (size_t done = 0; done < nframes;) {
        const size_t take = std::min(nframes - done, (size_t)ctx->max_len);
        const int slot = (int)(ctx->stage_seq++ & 1u);
        if (ctx->stage_free_valid[slot]) HIPCHK(ctx, hipStreamWaitEvent(ctx->h2d_stream, ctx->stage_free[slot], 0));
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_stage[slot], (const unsigned char*)frames + done * fb, take * fb, hipMemcpyHostToDevice, ctx->h2d_stream));
        HIPCHK(ctx, hipEventRecord(ctx->h2d_done, ctx->h2d_stream));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->h2d_done, 0));
        r = acg_process_pcm_dev(ctx, fmt, ctx->d_stage[slot], (int)take, nullptr);
        if (r != ACG_OK) {
            (void)hipEventSynchronize(ctx->h2d_done);           // the copy may still be reading the caller's buffer: not after we return
            return r;
        }
        // (the context's stream is ordered behind the de-interleave kernel, the buffer's only reader)
        HIPCHK(ctx, hipEventRecord(ctx->stage_free[slot], ctx->stream));
        ctx->stage_free_valid[slot] = true;
        done += take;
    }
    HIPCHK(ctx, hipEventSynchronize(ctx->h2d_done));           // the caller's buffer is free again (the copy stream runs in order)
    return ACG_OK;
}

// Only the kernel, into a scratch image of nch x pitch_floats words pre-filled with `fill`; the input lies in a device buffer
// of exactly its own size (rounded up to a word), so that a read or a write outside the ranges pcm.hip promises shows.
extern "C" int acg_lab_pcm_deinterleave(acg_ctx* ctx, int fmt, const void* frames_host, int nframes, float* dm_host, size_t pitch_floats,
                                        float fill)
{
    int r = check_pcm_args(ctx, fmt, frames_host);
    if (r != ACG_OK) return r;
    if (!dm_host || nframes < 0 || pitch_floats < (size_t)nframes || pitch_floats == 0) return fail(ctx, ACG_EINVAL, "image smaller than the frames");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    const size_t img = (size_t)ctx->cfg.nch * pitch_floats, in_bytes = ((size_t)nframes * ctx->cfg.nch * pcm_elem(fmt) + 3) & ~(size_t)3;
    for (size_t i = 0; i < img; ++i) dm_host[i] = fill;
    float* d_img = nullptr;
    void* d_in = nullptr;
    hipError_t e = hipMalloc(&d_img, img * sizeof(float));
    if (e == hipSuccess && in_bytes) e = hipMalloc(&d_in, in_bytes);
    if (e == hipSuccess) e = hipMemcpy(d_img, dm_host, img * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess && in_bytes) e = hipMemcpy(d_in, frames_host, (size_t)nframes * ctx->cfg.nch * pcm_elem(fmt), hipMemcpyHostToDevice);
    r = ACG_OK;
    if (e == hipSuccess && nframes > 0) r = launch_pcm(ctx, fmt, d_in, nframes, d_img, pitch_floats, ctx->stream);
    if (e == hipSuccess && r == ACG_OK) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess && r == ACG_OK) e = hipMemcpy(dm_host, d_img, img * sizeof(float), hipMemcpyDeviceToHost);
    if (d_img) (void)hipFree(d_img);
    if (d_in) (void)hipFree(d_in);
    if (e != hipSuccess) {
        ctx->err = std::string("acg_lab_pcm_deinterleave: ") + hipGetErrorString(e);
        return ACG_EHIP;
    }
    return r;
}

extern "C" int acg_sync(acg_ctx* ctx)
{
    if (!ctx) return ACG_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->msk_stream));
    if (ctx->post_stream) HIPCHK(ctx, hipStreamSynchronize(ctx->post_stream));
    return ACG_OK;
}

// A placement trial: one untimed process call (it also checks the arguments), `repeats` timed ones, then a reset
template <class Call>
static int placement_trial(acg_ctx* ctx, int repeats, double* ms_per_call, Call&& call)
{
    if (!ctx || !ms_per_call || repeats < 1) return ACG_EINVAL;
    int rc = call();
    if (rc != ACG_OK) return rc;
    HIPCHK(ctx, hipDeviceSynchronize());
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < repeats && rc == ACG_OK; ++i) rc = call();
    HIPCHK(ctx, hipDeviceSynchronize());
    const auto t1 = std::chrono::steady_clock::now();
    *ms_per_call = std::chrono::duration<double, std::milli>(t1 - t0).count() / repeats;
    int rr = acg_reset(ctx);
    if (rr == ACG_OK) rr = acg_get_timing(ctx, nullptr, nullptr, nullptr, nullptr);      // the trial's launches are nobody's timing
    return rc != ACG_OK ? rc : rr;
}

extern "C" int acg_placement_trial(acg_ctx* ctx, const uint8_t* iq_dev, size_t pitch_bytes, int nblocks, int repeats,
                                   void* hip_stream, double* ms_per_call)
{
    return placement_trial(ctx, repeats, ms_per_call,
                           [&] { return acg_process_iq_u8_dev(ctx, iq_dev, pitch_bytes, nblocks, hip_stream); });
}

extern "C" int acg_placement_trial_samples(acg_ctx* ctx, int fmt, const void* dev, size_t pitch_bytes, size_t plane_bytes, int nblocks,
                                           int repeats, void* hip_stream, double* ms_per_call)
{
    return placement_trial(ctx, repeats, ms_per_call,
                           [&] { return acg_process_samples_dev(ctx, fmt, dev, pitch_bytes, plane_bytes, nblocks, hip_stream); });
}

// ------------------------------------------------------------------------------------------
// The host's side of the block ring.  A collect hands out blocks up to the mark of the call `lag` calls behind the newest
// (the queue length when that call ended), a drain (lag = DRAIN) up to the device's count once everything has finished:
// the oldest min(pending, max) records of [consumed, upto), ordered by (chn, end_bit) within the call.  What does not fit
// STAYS queued (ACG_EAGAIN: call again, nothing lost); only a ring that the device has lapped loses blocks (ACG_EOVERFLOW,
// the count is in acg_last_error).
static constexpr int DRAIN = -1;

// *upto: where this collect / drain ends; *any = false: a collect with nothing pending (it returns ACG_OK at once)
static int ring_upto(acg_ctx* ctx, int lag, unsigned int* upto, bool* any)
{
    *any = false;
    if (lag != DRAIN && lag > ctx->lag_max) return fail(ctx, ACG_EINVAL, "lag above acg_max_lag(): the block queue of this context holds fewer calls");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    if (lag == DRAIN) {
        HIPCHK(ctx, hipDeviceSynchronize());
        HIPCHK(ctx, hipMemcpy(upto, ctx->d_frame_count, sizeof(*upto), hipMemcpyDeviceToHost));
        *any = true;
        return ACG_OK;
    }
    if (ctx->call_seq <= (unsigned long long)lag) return ACG_OK;              // nothing old enough yet
    const unsigned long long call = ctx->call_seq - 1 - (unsigned long long)lag;
    const int slot = (int)(call % acg_ctx::NCALL);
    HIPCHK(ctx, hipEventSynchronize(ctx->call_done[slot]));                   // only that call, not newer ones
    *upto = ctx->h_call_count[slot];
    // (a drain may already have handed out more than that call had queued: its mark then lies BEHIND the consumer -- nothing
    //  is pending; the counters are monotonic and wrap, so the comparison is a signed difference)
    *any = (int)(*upto - ctx->consumed) > 0;
    return ACG_OK;
}

// Claims the oldest min(pending, max) blocks of [consumed, upto); ACG_EOVERFLOW when the device lapped the host
static int ring_claim(acg_ctx* ctx, unsigned int upto, int max, unsigned int* pending, unsigned int* take)
{
    int rc = ACG_OK;
    *pending = upto - ctx->consumed;                              // monotonic counters, wrap-safe
    if (*pending > ctx->frame_cap) {                              // the device lapped the host: oldest lost
        char msg[96];
        std::snprintf(msg, sizeof(msg), "block queue lapped: the %u oldest blocks are lost", *pending - ctx->frame_cap);
        ctx->err = msg;
        if (ctx->d_stats) ctx->lost_blocks += *pending - ctx->frame_cap;   // (they belong to no channel: their records are gone)
        ctx->consumed = upto - ctx->frame_cap;
        *pending = ctx->frame_cap;
        rc = ACG_EOVERFLOW;
    }
    *take = std::min(*pending, (unsigned int)std::max(0, max));
    return rc;
}

// ... and what the call returns once the claimed records are out: the lap (its text is already in ctx->err), or `again`
// when some stayed queued
static int ring_result(acg_ctx* ctx, int rc, unsigned int pending, unsigned int take, const char* again)
{
    if (rc != ACG_OK) return rc;
    if (take < pending) return fail(ctx, ACG_EAGAIN, again);
    return ACG_OK;
}

// Statistics on: stats.hip's pass over the blocks [consumed, consumed + take) this call consumes, on the copy stream behind
// whatever the entry point has put there (msg_entry: the split's records lie in d_msgs).  Off: nothing is launched.
static int launch_stats(acg_ctx* ctx, unsigned int take, bool msg_entry)
{
    if (!ctx->d_stats || !take) return ACG_OK;
    const AcgStatsPass sp{ctx->d_frames, ctx->frame_cap, ctx->consumed, take, msg_entry ? ctx->d_msgs : nullptr, &ctx->msg_filter,
                          msg_entry && ctx->msg_filter_on ? 1 : 0, ctx->d_stats, ctx->cfg.nch};
    if (acg_launch_chan_stats(&sp, ctx->copy_stream) != 0) return fail(ctx, ACG_EHIP, "statistics pass failed");
    return ACG_OK;
}

// acg_set_channel_numbers: the staged records' slots become the numbers handed out, before anything is ordered or copied out
template <class Rec>
static void number_channels(const acg_ctx* ctx, Rec* rec, unsigned int n)
{
    const size_t nmap = ctx->chnum.size();
    for (unsigned int i = 0; nmap && i < n; ++i)
        if ((size_t)(unsigned int)rec[i].chn < nmap) rec[i].chn = ctx->chnum[(size_t)rec[i].chn];
}

// per channel in order (the contract): sorts an index into the records, not the records
template <class Rec>
static void order_by_channel(std::vector<unsigned int>& order, const Rec* rec)
{
    std::sort(order.begin(), order.end(), [rec](unsigned int x, unsigned int y) {
        return rec[x].chn != rec[y].chn ? rec[x].chn < rec[y].chn : rec[x].end_bit < rec[y].end_bit;
    });
}

static int fetch_frames(acg_ctx* ctx, int lag, acg_frame* out, int max_frames, int* nframes)
{
    unsigned int upto = 0, pending = 0, take = 0;
    bool any = false;
    int rc = ring_upto(ctx, lag, &upto, &any);
    if (rc != ACG_OK || !any) return rc;
    rc = ring_claim(ctx, upto, max_frames, &pending, &take);
    if (take > ctx->h_stage_cap) {                                // host staging, grown on demand
        // Pageable on purpose: with a pinned destination (one SDMA transfer) the same copy, issued while the
        // down-converter saturates HBM, made every step 0.9 ms slower at 16 384 channels (10.3 -> 11.2 ms);
        // through the runtime's own staging path it is invisible to the kernels.
        std::free(ctx->h_stage);
        ctx->h_stage = nullptr;
        ctx->h_stage_cap = 0;
        const size_t want = std::max<size_t>(take, 4096);
        ctx->h_stage = (AcgFrameRec*)std::malloc(want * sizeof(AcgFrameRec));
        if (!ctx->h_stage) return fail(ctx, ACG_ENOMEM, "frame staging");
        ctx->h_stage_cap = want;
    }
    AcgFrameRec* rec = ctx->h_stage;
    if (take) {
        const unsigned int cap = ctx->frame_cap;
        const unsigned int first = ctx->consumed & (cap - 1);      // (cap is a power of two)
        const unsigned int n1 = std::min(take, cap - first);
        if (const int sr = launch_stats(ctx, take, false)) return sr;
        HIPCHK(ctx, hipMemcpyAsync(rec, ctx->d_frames + first, (size_t)n1 * sizeof(AcgFrameRec),
                                   hipMemcpyDeviceToHost, ctx->copy_stream));
        if (take > n1)
            HIPCHK(ctx, hipMemcpyAsync(rec + n1, ctx->d_frames, (size_t)(take - n1) * sizeof(AcgFrameRec),
                                       hipMemcpyDeviceToHost, ctx->copy_stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
    }
    ctx->consumed += take;
    number_channels(ctx, rec, take);
    std::vector<unsigned int> order(take);
    for (unsigned int i = 0; i < take; ++i) order[i] = i;
    order_by_channel(order, rec);
    unsigned int kept = 0;
    for (unsigned int i = 0; i < take; ++i) {
        const AcgFrameRec& r = rec[order[i]];
        if (r.status == 2) continue;                              // dropped by the block repair (acars.c:124-207)
        acg_frame& f = out[kept++];
        std::memset(&f, 0, sizeof(f));
        f.chn = r.chn;
        f.len = r.len;
        f.err = r.err;
        f.lvl = acg_host_level_db(r.lvlsum, r.bitcount);         // acars.c:351
        f.crc[0] = r.crc[0];
        f.crc[1] = r.crc[1];
        if (r.len > 0) std::memcpy(f.txt, r.txt, (size_t)std::min(r.len, ACG_TXTMAX));
        f.end_bit = r.end_bit;
        f.end_sample = r.end_sample;
        f.soh_sample = r.end_sample - (long long)r.soh_back;      // acars.c:290: where the reference stamps blk->tv
    }
    *nframes = (int)kept;
    return ring_result(ctx, rc, pending, take, "more blocks queued than fit: call again");
}

extern "C" int acg_collect_frames(acg_ctx* ctx, int lag, acg_frame* out, int max_frames, int* nframes)
{
    if (!ctx || !nframes || (max_frames > 0 && !out) || lag < 0 || lag >= acg_ctx::NCALL - 1) return ACG_EINVAL;
    *nframes = 0;
    return fetch_frames(ctx, lag, out, max_frames, nframes);
}

extern "C" int acg_drain_frames(acg_ctx* ctx, acg_frame* out, int max_frames, int* nframes)
{
    if (!ctx || !nframes || (max_frames > 0 && !out)) return ACG_EINVAL;
    *nframes = 0;
    return fetch_frames(ctx, DRAIN, out, max_frames, nframes);
}

// ------------------------------------------------------------------------------------------
// the claimed blocks through the device-side field split (blk.hip msg_split_kernel)
static_assert(sizeof(AcgMsgRec) == sizeof(acg_msg), "device record and public record must have one layout");
// the message entry points' staging (fetch_msgs, sink_fetch), grown on demand: the split's records, device and host ...
static int grow_msg_stage(acg_ctx* ctx, unsigned int take)
{
    if (take <= ctx->msgs_cap) return ACG_OK;
    hipFree(ctx->d_msgs);
    std::free(ctx->h_msgs);
    ctx->d_msgs = nullptr;
    ctx->h_msgs = nullptr;
    ctx->msgs_cap = 0;
    const size_t want = std::max<size_t>(take, 4096);
    HIPCHK(ctx, hipMalloc(&ctx->d_msgs, want * sizeof(AcgMsgRec)));
    ctx->h_msgs = (AcgMsgRec*)std::malloc(want * sizeof(AcgMsgRec));
    if (!ctx->h_msgs) return fail(ctx, ACG_ENOMEM, "message staging");
    ctx->msgs_cap = want;
    return ACG_OK;
}

// ... and label.hip's output: the kept records, their labels, the per-workgroup counts and the total
static int grow_label_stage(acg_ctx* ctx, unsigned int take)
{
    if (take <= ctx->kmsgs_cap) return ACG_OK;
    hipFree(ctx->d_kmsgs); hipFree(ctx->d_oooi); hipFree(ctx->d_kwork);
    std::free(ctx->h_oooi);
    ctx->d_kmsgs = nullptr; ctx->d_oooi = nullptr; ctx->d_kwork = nullptr; ctx->h_oooi = nullptr;
    ctx->kmsgs_cap = 0;
    const size_t want = std::max<size_t>(take, 4096);
    HIPCHK(ctx, hipMalloc(&ctx->d_kmsgs, want * sizeof(AcgMsgRec)));
    HIPCHK(ctx, hipMalloc(&ctx->d_oooi, want * sizeof(acg_oooi)));
    HIPCHK(ctx, hipMalloc(&ctx->d_kwork, (want / 256 + 2) * sizeof(unsigned int)));
    ctx->h_oooi = (acg_oooi*)std::malloc(want * sizeof(acg_oooi));
    if (!ctx->h_oooi) return fail(ctx, ACG_ENOMEM, "label staging");
    ctx->kmsgs_cap = want;
    return ACG_OK;
}

// The owner of a flight table shared by several contexts, in a message entry point that consumes no blocks: the pass still runs,
// over the imported events alone.  Looks at the import queue only when the table is on; nothing queued: nothing launched.
static int commit_imports(acg_ctx* ctx)
{
    if (!ctx->flights || !acg_fl_imports_queued(ctx->flights)) return ACG_OK;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    const int rc = acg_fl_commit(ctx->flights, ctx->copy_stream);
    return rc == ACG_OK ? rc : fail(ctx, rc, "flight table: the pass over the imported events failed");
}

// The split of the `take` oldest blocks into d_msgs on the copy stream (it writes every byte of a record, text tail zeroed, so
// nothing stale crosses the ABI); with `labels`, label.hip's pass behind it into d_kmsgs / d_oooi (the caller has grown the label
// stage) and, the flight table on, its pass.  *d_total: the label pass's count of kept records, a device word.
static int launch_split(acg_ctx* ctx, unsigned int take, bool labels, unsigned int** d_total)
{
    *d_total = ctx->d_kwork + ctx->kmsgs_cap / 256 + 1;
    AcgLabelPass pass{&ctx->msg_filter, ctx->d_kwork, ctx->d_kmsgs, ctx->d_oooi, *d_total, nullptr, nullptr};
    if (ctx->flights) {                                           // over exactly the blocks this call consumes, before -e drops any
        const int fr = acg_fl_prepare(ctx->flights, take, ctx->copy_stream, &pass.flights);
        if (fr != ACG_OK) return fail(ctx, fr, "flight table: work space");
    }
    if (acg_launch_msg_split(ctx->d_frames, ctx->frame_cap, ctx->consumed, take, ctx->d_msgs, ctx->copy_stream, labels ? &pass : nullptr) != 0)
        return fail(ctx, ACG_EHIP, "message split launch failed");
    return launch_stats(ctx, take, true);
}

static int fetch_msgs(acg_ctx* ctx, int lag, acg_msg* out, acg_oooi* oooi, int max_msgs, int* nmsgs)
{
    unsigned int upto = 0, pending = 0, take = 0;
    bool any = false;
    int rc = ring_upto(ctx, lag, &upto, &any);
    if (rc != ACG_OK) return rc;
    if (!any) return commit_imports(ctx);
    if (!ctx->d_crctab) return fail(ctx, ACG_ESTATE, "context created without ACG_F_REPAIR");
    // A call splits and copies the oldest min(pending, max_msgs) blocks only (a block yields at most one message, so they
    // all fit) and consumes exactly those: draining a long queue through a small buffer costs what it hands out, not the
    // square of it, and the staging follows the caller's buffer, not the ring.
    rc = ring_claim(ctx, upto, max_msgs, &pending, &take);
    if (const int gr = grow_msg_stage(ctx, take)) return gr;
    // label.hip's pass (filters, label decoding, compaction) runs when a filter is set, the labels are asked for or the flight
    // table is on (its pass hangs on this one and shares its round trip); without all three the call launches and copies exactly
    // what it did before the pass existed
    const bool labels = oooi != nullptr || ctx->msg_filter_on || ctx->flights != nullptr;
    if (labels)
        if (const int gr = grow_label_stage(ctx, take)) return gr;
    unsigned int nrec = take;                                     // records that cross to the host
    if (take) {
        unsigned int* d_total = nullptr;
        if (const int lr = launch_split(ctx, take, labels, &d_total)) return lr;
        if (labels) {
            HIPCHK(ctx, hipMemcpyAsync(&nrec, d_total, sizeof(nrec), hipMemcpyDeviceToHost, ctx->copy_stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
            if (nrec > take) return fail(ctx, ACG_EHIP, "message label pass: count out of range");
            if (nrec) {
                HIPCHK(ctx, hipMemcpyAsync(ctx->h_msgs, ctx->d_kmsgs, (size_t)nrec * sizeof(AcgMsgRec), hipMemcpyDeviceToHost, ctx->copy_stream));
                HIPCHK(ctx, hipMemcpyAsync(ctx->h_oooi, ctx->d_oooi, (size_t)nrec * sizeof(acg_oooi), hipMemcpyDeviceToHost, ctx->copy_stream));
            }
        } else {
            HIPCHK(ctx, hipMemcpyAsync(ctx->h_msgs, ctx->d_msgs, (size_t)take * sizeof(AcgMsgRec), hipMemcpyDeviceToHost, ctx->copy_stream));
        }
        HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
    } else if (const int cr = commit_imports(ctx)) {
        return cr;
    }
    number_channels(ctx, ctx->h_msgs, nrec);
    const AcgMsgRec* rec = ctx->h_msgs;
    ctx->consumed += take;
    std::vector<unsigned int> order;
    order.reserve(nrec);
    for (unsigned int i = 0; i < nrec; ++i)
        if (rec[i].valid) order.push_back(i);                     // (blocks the repair dropped yield nothing)
    order_by_channel(order, rec);
    unsigned int kept = 0;
    for (unsigned int i : order) {
        acg_msg& m = out[kept++];
        std::memcpy(&m, &rec[i], sizeof(m));
        m.lvl = acg_host_level_db(rec[i].lvlsum, rec[i].bitcount);   // acars.c:351
        m.soh_sample = rec[i].end_sample - (long long)rec[i].soh_back;   // acars.c:290 (the device record holds the distance)
        m.reserved1 = 0;
        m.reserved2 = 0;
        m.reserved3 = 0;
        if (oooi) oooi[kept - 1] = ctx->h_oooi[i];
    }
    *nmsgs = (int)kept;
    return ring_result(ctx, rc, pending, take, "more messages queued than fit: call again");
}

extern "C" int acg_collect_msgs(acg_ctx* ctx, int lag, acg_msg* out, int max_msgs, int* nmsgs)
{
    if (!ctx || !nmsgs || (max_msgs > 0 && !out) || lag < 0 || lag >= acg_ctx::NCALL - 1) return ACG_EINVAL;
    *nmsgs = 0;
    return fetch_msgs(ctx, lag, out, nullptr, max_msgs, nmsgs);
}

extern "C" int acg_drain_msgs(acg_ctx* ctx, acg_msg* out, int max_msgs, int* nmsgs)
{
    if (!ctx || !nmsgs || (max_msgs > 0 && !out)) return ACG_EINVAL;
    *nmsgs = 0;
    return fetch_msgs(ctx, DRAIN, out, nullptr, max_msgs, nmsgs);
}

extern "C" int acg_collect_msgs_oooi(acg_ctx* ctx, int lag, acg_msg* out, acg_oooi* oooi, int max_msgs, int* nmsgs)
{
    if (!ctx || !nmsgs || (max_msgs > 0 && (!out || !oooi)) || lag < 0 || lag >= acg_ctx::NCALL - 1) return ACG_EINVAL;
    *nmsgs = 0;
    acg_oooi none;
    return fetch_msgs(ctx, lag, out, oooi ? oooi : &none, max_msgs, nmsgs);
}

extern "C" int acg_drain_msgs_oooi(acg_ctx* ctx, acg_msg* out, acg_oooi* oooi, int max_msgs, int* nmsgs)
{
    if (!ctx || !nmsgs || (max_msgs > 0 && (!out || !oooi))) return ACG_EINVAL;
    *nmsgs = 0;
    acg_oooi none;
    return fetch_msgs(ctx, DRAIN, out, oooi ? oooi : &none, max_msgs, nmsgs);
}

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

// ---- the sink's filters (label.c:9-23 build_label_filter, acarsdec.c -A / -b / -e) --------------------------------------
static_assert(ACG_LBL_MAXTOK == ACG_MSGF_MAXLABELS, "token capacity");
static_assert(sizeof(acg_oooi) == 40 && offsetof(acg_oooi, decoded) == 35 && offsetof(acg_oooi, won) == 30,
              "acg_oooi: oooi_t (acarsdec.h:94-102), decoded, padding");

extern "C" int acg_parse_label_filter(const char* arg, acg_msg_filter* f)
{
    if (!f) return ACG_EINVAL;
    int n = 0;
    char tok[ACG_MSGF_MAXLABELS][4] = {};
    for (const char* p = arg; p && *p;) {
        if (*p == ':') { ++p; continue; }                         // strtok: runs of separators delimit nothing
        const char* e = p;
        while (*e && *e != ':') ++e;
        if (n == ACG_MSGF_MAXLABELS) return ACG_EINVAL;
        const size_t len = std::min<size_t>((size_t)(e - p), 3);   // a longer token never matches a label (at most 2 chars) either
        std::memcpy(tok[n++], p, len);
        p = e;
    }
    f->nlabels = n;
    std::memcpy(f->labels, tok, sizeof(tok));
    return ACG_OK;
}

// the device form of a filter (label.hip); ACG_EINVAL when it is not one acg_parse_label_filter could have made
static int label_filter_dev(const acg_msg_filter* f, AcgLabelFilter* d)
{
    std::memset(d, 0, sizeof(*d));
    if (!f) return ACG_OK;
    if ((f->flags & ~(ACG_MSGF_DOWNLINK_ONLY | ACG_MSGF_SKIP_EMPTY)) || f->nlabels < 0 || f->nlabels > ACG_MSGF_MAXLABELS) return ACG_EINVAL;
    d->flags = f->flags;
    d->nlabels = f->nlabels;
    for (int i = 0; i < f->nlabels; ++i) {
        const char* t = f->labels[i];
        if (!t[0] || std::memchr(t, 0, 4) == nullptr) return ACG_EINVAL;
        unsigned int w = 0;
        for (int k = 0; k < 3 && t[k]; ++k) w |= (unsigned int)(unsigned char)t[k] << (8 * k);
        d->tok[i] = w;
    }
    return ACG_OK;
}

extern "C" int acg_set_msg_filter(acg_ctx* ctx, const acg_msg_filter* f)
{
    if (!ctx) return ACG_EINVAL;
    AcgLabelFilter d;
    if (label_filter_dev(f, &d) != ACG_OK) return fail(ctx, ACG_EINVAL, "message filter: unknown flag, label count or empty token");
    ctx->msg_filter = d;
    ctx->msg_filter_on = f != nullptr;
    return ACG_OK;
}

extern "C" int acg_selftest_msg_labels(const acg_msg* in, int n, const acg_msg_filter* f, unsigned char* keep, acg_oooi* oooi)
{
    if (n < 0 || (n > 0 && (!in || !keep || !oooi))) return ACG_EINVAL;
    AcgLabelFilter d;
    if (label_filter_dev(f, &d) != ACG_OK) return ACG_EINVAL;
    if (n == 0) return ACG_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return ACG_ENODEV;
    LabStage lab((size_t)n);
    lab.stage(in, (unsigned int)n, false, false);                  // soh_back as given: the kept records are compared with these
    unsigned char* d_keep = nullptr;
    std::vector<AcgMsgRec> kept((size_t)n);
    std::vector<acg_oooi> ko((size_t)n);
    unsigned int total = 0;
    int rc = ACG_EHIP;
    if (lab.ok() && hipMalloc(&d_keep, (size_t)n) == hipSuccess && lab.label((unsigned int)n, &d, d_keep) == 0 &&
        hipMemcpy(&total, lab.d_total(), sizeof(total), hipMemcpyDeviceToHost) == hipSuccess && total <= (unsigned int)n &&
        hipMemcpy(keep, d_keep, (size_t)n, hipMemcpyDeviceToHost) == hipSuccess &&
        hipMemcpy(kept.data(), lab.d_out, (size_t)total * sizeof(AcgMsgRec), hipMemcpyDeviceToHost) == hipSuccess &&
        hipMemcpy(ko.data(), lab.d_oooi, (size_t)total * sizeof(acg_oooi), hipMemcpyDeviceToHost) == hipSuccess) {
        // the compaction's own check: the kept records, in input order, and nothing else
        rc = ACG_OK;
        unsigned int j = 0;
        for (int i = 0; i < n; ++i) {
            std::memset(&oooi[i], 0, sizeof(acg_oooi));
            if (!keep[i]) continue;
            if (j >= total || std::memcmp(&kept[j], &lab.h[i], sizeof(AcgMsgRec)) != 0) rc = ACG_ESTATE;
            else oooi[i] = ko[j];
            ++j;
        }
        if (j != total) rc = ACG_ESTATE;
    }
    hipFree(d_keep);
    return rc;
}

// ---- the channel numbers a sharded host hands out (acg_set_channel_numbers; the sinks' order keys: acg_sink_keys below) ---
extern "C" int acg_channel_numbers_check(const int* chn, int n)
{
    if (n < 0 || (n > 0 && !chn)) return ACG_EINVAL;
    if (n > (1 << 20)) return ACG_EINVAL;                         // (more values than numbers: two are equal)
    unsigned char* seen = (unsigned char*)std::calloc(1u << 17, 1);      // a bit per number
    if (!seen) return ACG_ENOMEM;
    int rc = ACG_OK;
    for (int i = 0; i < n && rc == ACG_OK; ++i) {
        const unsigned int v = (unsigned int)chn[i];              // (a negative value is a large one)
        if (v >= (1u << 20) || (seen[v >> 3] >> (v & 7u) & 1u)) rc = ACG_EINVAL;
        else seen[v >> 3] |= (unsigned char)(1u << (v & 7u));
    }
    std::free(seen);
    return rc;
}

extern "C" int acg_set_channel_numbers(acg_ctx* ctx, const int* chn)
{
    if (!ctx) return ACG_EINVAL;
    const int nch = ctx->cfg.nch;
    if (chn && acg_channel_numbers_check(chn, nch) != ACG_OK) return fail(ctx, ACG_EINVAL, "channel numbers: outside 0 .. 2^20 - 1, or not distinct");
    int* d_new = nullptr;
    // (every entry point that reads the map ends with a synchronise of its stream: nothing in flight holds the old array)
    if (hipSetDevice(ctx->cfg.device) != hipSuccess || hipStreamSynchronize(ctx->copy_stream) != hipSuccess ||
        (chn && (hipMalloc(&d_new, (size_t)nch * sizeof(int)) != hipSuccess ||
                 hipMemcpy(d_new, chn, (size_t)nch * sizeof(int), hipMemcpyHostToDevice) != hipSuccess))) {
        hipFree(d_new);
        return fail(ctx, ACG_EHIP, "channel numbers: upload failed");
    }
    hipFree(ctx->d_chnum);
    ctx->d_chnum = d_new;
    ctx->chnum.assign(chn, chn ? chn + nch : chn);
    if (ctx->flights) acg_fl_context_channels(ctx->flights, ctx->d_chnum, (unsigned int)nch);
    return ACG_OK;
}

// ---- the flight table (flight.hip, flights.cpp) -------------------------------------------------------------------------
extern "C" int acg_flights_enable(acg_ctx* ctx, const acg_flight_config* cfg)
{
    if (!ctx || (cfg && !acg_fl_config_ok(cfg))) return ACG_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    if (ctx->flights) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
        acg_fl_destroy(ctx->flights);
        ctx->flights = nullptr;
    }
    if (!cfg) return ACG_OK;
    if (!acg_fl_create) return fail(ctx, ACG_ESTATE, "flight table: not in this build");
    if (!ctx->d_crctab) return fail(ctx, ACG_ESTATE, "flight table: context created without ACG_F_REPAIR");
    if (ctx->cfg.nch > (1 << 20)) return fail(ctx, ACG_EINVAL, "flight table: more than 2^20 channels");
    const int rc = acg_fl_create(&ctx->flights, cfg);
    if (rc != ACG_OK) return fail(ctx, rc, "flight table: allocation failed");
    acg_fl_context_channels(ctx->flights, ctx->d_chnum, (unsigned int)ctx->cfg.nch);     // (acg_set_channel_numbers, until the table gets a map of its own)
    return ACG_OK;
}

extern "C" int acg_flight_snapshot(acg_ctx* ctx, acg_flight* out, int max, int* n, int* dropped)
{
    if (!ctx || !n || max < 0 || (max > 0 && !out)) return ACG_EINVAL;
    *n = 0;
    if (!ctx->flights) return fail(ctx, ACG_ESTATE, "flight table is off");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    const int rc = acg_fl_snapshot(ctx->flights, ctx->copy_stream, out, max, n, dropped);
    return rc == ACG_OK ? rc : fail(ctx, rc, rc == ACG_EAGAIN ? "more flights than fit: *n says how many" : "flight snapshot failed");
}

extern "C" int acg_drain_routes(acg_ctx* ctx, acg_route* out, int max, int* n)
{
    if (!ctx || !n || max < 0 || (max > 0 && !out)) return ACG_EINVAL;
    *n = 0;
    if (!ctx->flights) return fail(ctx, ACG_ESTATE, "flight table is off");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    const int rc = acg_fl_drain_routes(ctx->flights, ctx->copy_stream, out, max, n);
    return rc == ACG_OK ? rc : fail(ctx, rc, rc == ACG_EAGAIN ? "more routes queued than fit: call again" : "route hand-over failed");
}

// ---- one flight table for the channels of several contexts: events leave the peers and enter the owner ---------------------
extern "C" int acg_flight_events_check(const acg_flight_event* ev, int n)
{
    if (n < 0 || (n > 0 && !ev)) return ACG_EINVAL;
    for (int i = 0; i < n; ++i) {
        const acg_flight_event& e = ev[i];
        if (e.usec < 0 || e.usec > 999999 || e.addr[0] == 0 || e.chn < 0 || e.chn >= (1 << 20) || e.end_sample < 0 || e.end_sample >= (1ll << 43) ||
            (e.e_ok != 0 && e.e_ok != 1))
            return ACG_EINVAL;
    }
    return ACG_OK;
}

extern "C" int acg_flights_set_channels(acg_ctx* ctx, const int* chn)
{
    if (!ctx) return ACG_EINVAL;
    if (!ctx->flights) return fail(ctx, ACG_ESTATE, "flight table is off");
    for (int c = 0; chn && c < ctx->cfg.nch; ++c)
        if (chn[c] < 0 || chn[c] >= (1 << 20)) return fail(ctx, ACG_EINVAL, "flight table: a channel number outside 0 .. 2^20 - 1");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    const int rc = acg_fl_set_channels(ctx->flights, chn, ctx->cfg.nch);
    return rc == ACG_OK ? rc : fail(ctx, rc, "flight table: channel map");
}

extern "C" int acg_flights_export(acg_ctx* ctx, int on)
{
    if (!ctx) return ACG_EINVAL;
    if (!ctx->flights) return fail(ctx, ACG_ESTATE, "flight table is off");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    const int rc = acg_fl_export(ctx->flights, on);
    return rc == ACG_OK ? rc : fail(ctx, rc, "flight table: export queue");
}

extern "C" int acg_drain_flight_events(acg_ctx* ctx, acg_flight_event* out, int max, int* n)
{
    if (!ctx || !n || max < 0 || (max > 0 && !out)) return ACG_EINVAL;
    *n = 0;
    if (!ctx->flights) return fail(ctx, ACG_ESTATE, "flight table is off");
    if (!acg_fl_exporting(ctx->flights)) return fail(ctx, ACG_ESTATE, "flight table: export is off (acg_flights_export first)");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    const int rc = acg_fl_drain_events(ctx->flights, ctx->copy_stream, out, max, n);
    return rc == ACG_OK ? rc : fail(ctx, rc, rc == ACG_EAGAIN ? "more flight events queued than fit: call again" : "flight event hand-over failed");
}

extern "C" int acg_flights_import(acg_ctx* ctx, const acg_flight_event* ev, int n)
{
    if (!ctx || n < 0 || (n > 0 && !ev)) return ACG_EINVAL;
    if (acg_flight_events_check(ev, n) != ACG_OK) return fail(ctx, ACG_EINVAL, "flight event import: a field out of range (acg_flight_events_check)");
    if (!ctx->flights) return fail(ctx, ACG_ESTATE, "flight table is off");
    if (acg_fl_exporting(ctx->flights)) return fail(ctx, ACG_ESTATE, "flight table: this context exports its events, it cannot import");
    const int rc = n ? acg_fl_import(ctx->flights, ev, n) : ACG_OK;
    return rc == ACG_OK ? rc : fail(ctx, rc, "flight event import");
}

extern "C" int acg_flights_commit(acg_ctx* ctx)
{
    if (!ctx) return ACG_EINVAL;
    if (!ctx->flights) return fail(ctx, ACG_ESTATE, "flight table is off");
    if (acg_fl_exporting(ctx->flights)) return fail(ctx, ACG_ESTATE, "flight table: this context exports its events");
    return commit_imports(ctx);
}

extern "C" int acg_selftest_flights(const acg_msg* in, const int* batch, int nbatch, const acg_flight_config* cfg, const acg_msg_filter* f,
                                    acg_flight* snaps, int snap_cap, int* snap_n, acg_route* routes, int route_cap, int* nroutes, int* dropped)
{
    if (nbatch < 0 || !acg_fl_config_ok(cfg) || snap_cap < 0 || route_cap < 0 || !nroutes || (nbatch > 0 && (!batch || !snap_n)) ||
        (snap_cap > 0 && !snaps) || (route_cap > 0 && !routes))
        return ACG_EINVAL;
    AcgLabelFilter d;
    if (label_filter_dev(f, &d) != ACG_OK) return ACG_EINVAL;
    size_t total = 0, biggest = 0;
    for (int b = 0; b < nbatch; ++b) {
        if (batch[b] < 0) return ACG_EINVAL;
        total += (size_t)batch[b];
        biggest = std::max(biggest, (size_t)batch[b]);
    }
    if (total > 0 && !in) return ACG_EINVAL;
    *nroutes = 0;
    int ndev = 0;
    if (!acg_fl_create || hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return ACG_ENODEV;
    AcgFlights* t = nullptr;
    int rc = acg_fl_create(&t, cfg);
    if (rc != ACG_OK) return rc;
    {
        LabStage lab(biggest);
        if (!lab.ok()) rc = ACG_ENOMEM;
        size_t at = 0;
        int snap_at = 0;
        for (int b = 0; b < nbatch && rc == ACG_OK; ++b) {
            const unsigned int n = (unsigned int)batch[b];
            lab.stage(in + at, n, false, true);
            at += n;
            if (n) {
                const AcgFlightPass* fp = nullptr;
                rc = acg_fl_prepare(t, n, nullptr, &fp);
                if (rc == ACG_OK && lab.label(n, &d, nullptr, fp) != 0) rc = ACG_EHIP;
            }
            if (rc == ACG_OK) {
                rc = acg_fl_snapshot(t, nullptr, snaps + snap_at, snap_cap - snap_at, &snap_n[b], dropped);
                if (rc == ACG_OK) snap_at += snap_n[b];
            }
        }
        if (rc == ACG_OK) rc = acg_fl_drain_routes(t, nullptr, routes, route_cap, nroutes);
    }
    acg_fl_destroy(t);
    return rc;
}

// acg_selftest_flights over SEVERAL tables, as a host that shards its channels `c mod nshards` drives them: in[i].chn is the global
// channel; shard r = chn % nshards holds it as local channel chn / nshards under the map l -> l * nshards + r; shards 1 .. export,
// shard 0 owns the table.  A batch is a round: every peer's pass and the drain of its events, their import at the owner, the
// owner's pass (no records of its own in the round: acg_fl_commit, as a message entry point that consumes no blocks).
extern "C" int acg_selftest_flights_sharded(const acg_msg* in, const int* batch, int nbatch, int nshards, const acg_flight_config* cfg,
                                            const acg_msg_filter* f, acg_flight* snaps, int snap_cap, int* snap_n, acg_route* routes, int route_cap,
                                            int* nroutes, int* dropped, float* pass_ms)
{
    if (nbatch < 0 || nshards < 1 || nshards > 64 || !acg_fl_config_ok(cfg) || snap_cap < 0 || route_cap < 0 || !nroutes ||
        (nbatch > 0 && (!batch || !snap_n || !dropped)) || (snap_cap > 0 && !snaps) || (route_cap > 0 && !routes))
        return ACG_EINVAL;
    AcgLabelFilter d;
    if (label_filter_dev(f, &d) != ACG_OK) return ACG_EINVAL;
    size_t total = 0, biggest = 0;
    for (int b = 0; b < nbatch; ++b) {
        if (batch[b] < 0) return ACG_EINVAL;
        total += (size_t)batch[b];
        biggest = std::max(biggest, (size_t)batch[b]);
    }
    if (total > 0 && !in) return ACG_EINVAL;
    int nloc = 1;                                                  // local channels per shard
    for (size_t i = 0; i < total; ++i) {
        if (in[i].chn < 0 || in[i].chn >= (1 << 20)) return ACG_EINVAL;
        nloc = std::max(nloc, in[i].chn / nshards + 1);
    }
    *nroutes = 0;
    int ndev = 0;
    if (!acg_fl_create || hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return ACG_ENODEV;
    std::vector<AcgFlights*> T((size_t)nshards, nullptr);
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int rc = ACG_OK;
    if (pass_ms && (hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess)) rc = ACG_EHIP;
    for (int r = 0; r < nshards && rc == ACG_OK; ++r) {
        std::vector<int> map((size_t)nloc);
        for (int l = 0; l < nloc; ++l) map[(size_t)l] = l * nshards + r;
        rc = acg_fl_create(&T[(size_t)r], cfg);
        if (rc == ACG_OK && nshards > 1) rc = acg_fl_set_channels(T[(size_t)r], map.data(), nloc);       // (one shard: the identity, left unset)
        if (rc == ACG_OK && r > 0) rc = acg_fl_export(T[(size_t)r], 1);
    }
    if (rc == ACG_OK) {
        LabStage lab(biggest);
        if (!lab.ok()) rc = ACG_ENOMEM;
        std::vector<acg_msg> part(std::max<size_t>(biggest, 1));
        std::vector<acg_flight_event> evs(std::max<size_t>(biggest, 1));
        size_t at = 0;
        int snap_at = 0;
        for (int b = 0; b < nbatch && rc == ACG_OK; ++b) {
            for (int r = nshards > 1 ? 1 : 0; rc == ACG_OK; r = (r + 1) % nshards) {      // the peers, then the owner
                unsigned int n = 0;
                for (size_t i = at; i < at + (size_t)batch[b]; ++i)
                    if (in[i].chn % nshards == r) {
                        part[n] = in[i];
                        part[n++].chn = in[i].chn / nshards;
                    }
                AcgFlights* t = T[(size_t)r];
                const AcgFlightPass* fp = nullptr;
                lab.stage(part.data(), n, false, true);
                if (n && lab.upload(n) != 0) rc = ACG_EHIP;
                if (rc == ACG_OK && r == 0 && pass_ms && hipEventRecord(ev0, nullptr) != hipSuccess) rc = ACG_EHIP;
                if (rc == ACG_OK && n) {
                    rc = acg_fl_prepare(t, n, nullptr, &fp);
                    if (rc == ACG_OK && lab.launch(n, &d, nullptr, fp) != 0) rc = ACG_EHIP;
                } else if (rc == ACG_OK && r == 0) {
                    rc = acg_fl_commit(t, nullptr);
                }
                if (rc == ACG_OK && r > 0) {
                    int k = 0;
                    rc = acg_fl_drain_events(t, nullptr, evs.data(), (int)evs.size(), &k);
                    if (rc == ACG_OK && acg_flight_events_check(evs.data(), k) != ACG_OK) rc = ACG_ESTATE;
                    if (rc == ACG_OK && k) rc = acg_fl_import(T[0], evs.data(), k);
                }
                if (r == 0) break;
            }
            if (rc == ACG_OK && pass_ms) {
                if (hipEventRecord(ev1, nullptr) != hipSuccess || hipEventSynchronize(ev1) != hipSuccess ||
                    hipEventElapsedTime(&pass_ms[b], ev0, ev1) != hipSuccess)
                    rc = ACG_EHIP;
            }
            at += (size_t)batch[b];
            if (rc == ACG_OK) {
                rc = acg_fl_snapshot(T[0], nullptr, snaps + snap_at, snap_cap - snap_at, &snap_n[b], &dropped[b]);
                if (rc == ACG_OK) snap_at += snap_n[b];
            }
        }
        if (rc == ACG_OK) rc = acg_fl_drain_routes(T[0], nullptr, routes, route_cap, nroutes);
        for (int r = 1; r < nshards && rc == ACG_OK; ++r) {        // a peer's table stays empty and emits nothing
            acg_flight one;
            acg_route rt;
            int k = 0, kr = 0, dr = 0;
            const int rs = acg_fl_snapshot(T[(size_t)r], nullptr, &one, 1, &k, &dr), rr = acg_fl_drain_routes(T[(size_t)r], nullptr, &rt, 1, &kr);
            if (rs != ACG_OK || rr != ACG_OK || k || kr || dr) rc = ACG_ESTATE;
        }
    }
    for (AcgFlights* t : T)
        if (t) acg_fl_destroy(t);
    if (ev0) hipEventDestroy(ev0);
    if (ev1) hipEventDestroy(ev1);
    return rc;
}

// ---- the device renderers of the batch sink (json.hip: buildjson()'s lines; text.hip: printoneline(), printmsg(), Netoutpp(),
// Netoutsv()): one host runtime.  A format supplies its descriptor, the check of its configuration, what it renders once on the
// host (its AcgJsonDev / AcgTextDev and the channels' frequency tokens) and the argument checks of its entry points.
static_assert(ACG_JS_LINE_MAX == ACG_JSON_LINE_MAX, "line bound");
static_assert(ACG_TX_REC_MAX == ACG_TEXT_REC_MAX, "record bound");

struct AcgSinkFormat {
    const char* name;                       // the first word of the shared messages
    const char* is_off;                     // what a fetch says while the sink is off
    size_t rec_max;                         // the longest record
    unsigned int max_take;                  // the most records one pass takes: their offsets are 32-bit
    int (*launch)(const AcgSinkPass*, void*);   // null: the unit is not in this build
    bool offsets;                           // the entry points hand out the table of the records' offsets
};
static const AcgSinkFormat SINK_JSON = {"JSON", "JSON sink is off: acg_json_enable first", ACG_JSON_LINE_MAX, (1u << 31) / ACG_JSON_LINE_MAX,
                                        acg_launch_json, false};
static const AcgSinkFormat SINK_TEXT = {"text", "text sink is off: acg_text_enable first", ACG_TEXT_REC_MAX, (1u << 31) / ACG_TEXT_REC_MAX,
                                        acg_launch_text, true};

static int sink_fail(acg_ctx* ctx, int code, const AcgSinkFormat* fmt, const char* rest)
{
    return fail(ctx, code, (std::string(fmt->name) + rest).c_str());
}

// a sink: its format, its configuration on the device and its work space (sort keys, lengths, offsets and the rendered bytes)
struct AcgSinkState {
    const AcgSinkFormat* fmt = nullptr;
    void* d_cfg = nullptr;                  // AcgJsonDev / AcgTextDev
    unsigned char* d_freq = nullptr;        // [nch] frequency tokens: [8] "%3.3f" / [ACG_TX_FREQ_SLOT] "F:%3.3f "
    unsigned int* d_cnt = nullptr;          // [4]: bytes, records of the last pass; the level guard
    size_t cap = 0;                         // records the work space below holds
    unsigned long long *d_key = nullptr, *d_key_s = nullptr;
    unsigned int *d_idx = nullptr, *d_idx_s = nullptr, *d_len = nullptr, *d_off = nullptr, *d_wg = nullptr;
    unsigned char* d_out = nullptr;         // cap * fmt->rec_max bytes
    unsigned int last_nrecs = 0;            // records the most recent fetch handed out: the first keys of d_key_s (acg_sink_keys)
};

static void sink_free_work(AcgSinkState* st)
{
    hipFree(st->d_key); hipFree(st->d_key_s); hipFree(st->d_idx); hipFree(st->d_idx_s); hipFree(st->d_len); hipFree(st->d_off);
    hipFree(st->d_wg); hipFree(st->d_out);
    st->d_key = st->d_key_s = nullptr;
    st->d_idx = st->d_idx_s = st->d_len = st->d_off = st->d_wg = nullptr;
    st->d_out = nullptr;
    st->cap = 0;
}

static void sink_destroy(AcgSinkState* st)
{
    if (!st) return;
    sink_free_work(st);
    hipFree(st->d_cfg); hipFree(st->d_freq); hipFree(st->d_cnt);
    delete st;
}

// what a format renders once on the host
struct SinkBlob {
    int rc = ACG_OK;                        // ACG_EINVAL: a stretch does not fit (cannot happen); sink_create hands it on
    std::vector<unsigned char> cfg, freq;
};

// ACG_OK, ACG_ENOMEM or ACG_EHIP (or the blob's own verdict)
static int sink_create(AcgSinkState** out, const AcgSinkFormat* fmt, const SinkBlob& blob)
{
    if (blob.rc != ACG_OK) return blob.rc;
    AcgSinkState* st = new (std::nothrow) AcgSinkState();
    if (!st) return ACG_ENOMEM;
    st->fmt = fmt;
    if (hipMalloc(&st->d_cfg, blob.cfg.size()) != hipSuccess || hipMalloc(&st->d_freq, blob.freq.size()) != hipSuccess ||
        hipMalloc(&st->d_cnt, 4 * sizeof(unsigned int)) != hipSuccess) {
        sink_destroy(st);
        return ACG_ENOMEM;
    }
    if (hipMemcpy(st->d_cfg, blob.cfg.data(), blob.cfg.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(st->d_freq, blob.freq.data(), blob.freq.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(st->d_cnt, 0, 4 * sizeof(unsigned int)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        sink_destroy(st);
        return ACG_EHIP;
    }
    *out = st;
    return ACG_OK;
}

// work space and output buffer for n records, grown on demand as d_kmsgs is
static int sink_reserve(AcgSinkState* st, size_t n)
{
    if (n <= st->cap) return ACG_OK;
    sink_free_work(st);
    const size_t want = std::max<size_t>(n, 4096);
    if (hipMalloc(&st->d_key, want * 8) != hipSuccess || hipMalloc(&st->d_key_s, want * 8) != hipSuccess ||
        hipMalloc(&st->d_idx, want * 4) != hipSuccess || hipMalloc(&st->d_idx_s, want * 4) != hipSuccess ||
        hipMalloc(&st->d_len, want * 4) != hipSuccess || hipMalloc(&st->d_off, want * 4) != hipSuccess ||
        hipMalloc(&st->d_wg, 2 * (want / 256 + 1) * 4) != hipSuccess || hipMalloc(&st->d_out, want * st->fmt->rec_max) != hipSuccess) {
        sink_free_work(st);
        return ACG_ENOMEM;
    }
    st->cap = want;
    return ACG_OK;
}

static AcgSinkPass sink_pass(const AcgSinkState* st, const AcgMsgRec* recs, const void* oooi, const unsigned int* total, unsigned int nmax, bool lvl_from_rec)
{
    AcgSinkPass p;
    std::memset(&p, 0, sizeof(p));
    p.recs = recs;
    p.oooi = (const unsigned char*)oooi;
    p.total = total;
    p.nmax = nmax;
    p.cfg = st->d_cfg;
    p.freq = st->d_freq;
    p.lvl_from_rec = lvl_from_rec ? 1 : 0;
    p.key = st->d_key; p.key_s = st->d_key_s;
    p.idx = st->d_idx; p.idx_s = st->d_idx_s;
    p.len = st->d_len; p.off = st->d_off;
    p.wg_sum = st->d_wg; p.wg_cnt = st->d_wg + (st->cap / 256 + 1);
    p.counters = st->d_cnt;
    p.out = st->d_out;
    p.out_cap = (unsigned int)std::min<size_t>(st->cap * st->fmt->rec_max, 0xffffffffu);
    return p;
}

// What acg_json_enable and acg_text_enable share, behind the check of their configuration: the old sink leaves behind a stream
// sync; blob == null leaves the sink off
static int sink_enable(acg_ctx* ctx, AcgSinkState** slot, const AcgSinkFormat* fmt, const SinkBlob* blob)
{
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    if (*slot) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
        sink_destroy(*slot);
        *slot = nullptr;
    }
    if (!blob) return ACG_OK;
    if (!fmt->launch) return sink_fail(ctx, ACG_ESTATE, fmt, " sink: not in this build");
    if (!ctx->d_crctab) return sink_fail(ctx, ACG_ESTATE, fmt, " sink: context created without ACG_F_REPAIR");
    if (ctx->cfg.nch > (1 << 20)) return sink_fail(ctx, ACG_EINVAL, fmt, " sink: more than 2^20 channels");
    const int rc = sink_create(slot, fmt, *blob);
    return rc == ACG_OK ? rc : sink_fail(ctx, rc, fmt, " sink: allocation failed");
}

// fetch_msgs' sibling: the same claim, split, label pass and flight pass; then the renderer's passes on the same stream, and only
// the packed records, two counters and (offs != null) the table of the records' offsets cross to the host.  A block yields at
// most one record of at most rec_max bytes: the oldest min(max_recs, cap / rec_max) always fit.
static int sink_fetch(acg_ctx* ctx, const AcgSinkFormat* fmt, AcgSinkState* st, int lag, char* out, size_t cap, size_t* nbytes, unsigned int* offs,
                      int max_recs, int* nrecs)
{
    if (!ctx->d_crctab) return fail(ctx, ACG_ESTATE, "context created without ACG_F_REPAIR");
    if (!st) return fail(ctx, ACG_ESTATE, fmt->is_off);
    st->last_nrecs = 0;
    const size_t fit = std::min<size_t>(std::min<size_t>(cap / fmt->rec_max, (size_t)max_recs), fmt->max_take);
    unsigned int upto = 0, pending = 0, take = 0;
    bool any = false;
    int rc = ring_upto(ctx, lag, &upto, &any);
    if (rc != ACG_OK) return rc;
    if (!any) return commit_imports(ctx);
    rc = ring_claim(ctx, upto, (int)fit, &pending, &take);
    if (!take) {
        if (const int cr = commit_imports(ctx)) return cr;
        return ring_result(ctx, rc, pending, take, "more messages queued than fit: call again");
    }
    if (const int gr = grow_msg_stage(ctx, take)) return gr;
    if (const int gr = grow_label_stage(ctx, take)) return gr;
    if (sink_reserve(st, take) != ACG_OK) return fail(ctx, ACG_ENOMEM, "sink: work space");
    unsigned int* d_total = nullptr;
    if (const int lr = launch_split(ctx, take, true, &d_total)) return lr;
    AcgSinkPass sp = sink_pass(st, ctx->d_kmsgs, ctx->d_oooi, d_total, take, false);
    sp.chmap = ctx->d_chnum;                                      // the map in force at hand-out (acg_set_channel_numbers)
    sp.nmap = ctx->d_chnum ? (unsigned int)ctx->cfg.nch : 0u;
    if (fmt->launch(&sp, ctx->copy_stream) != 0) return sink_fail(ctx, ACG_EHIP, fmt, " pass launch failed");
    unsigned int cnt[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(cnt, st->d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, ctx->copy_stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
    if (cnt[0] > cap || cnt[1] > take || (size_t)cnt[0] > (size_t)take * fmt->rec_max) return sink_fail(ctx, ACG_EHIP, fmt, " pass: counts out of range");
    if (cnt[0]) {                                                 // (kept records sort in front of dropped ones: the first cnt[1] offsets)
        HIPCHK(ctx, hipMemcpyAsync(out, st->d_out, cnt[0], hipMemcpyDeviceToHost, ctx->copy_stream));
        if (offs) HIPCHK(ctx, hipMemcpyAsync(offs, st->d_off, (size_t)cnt[1] * sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->copy_stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
    }
    if (offs) offs[cnt[1]] = cnt[0];
    ctx->consumed += take;
    st->last_nrecs = cnt[1];
    *nbytes = cnt[0];
    *nrecs = (int)cnt[1];
    return ring_result(ctx, rc, pending, take, "more messages queued than fit: call again");
}

static int sink_level_guard(acg_ctx* ctx, const AcgSinkFormat* fmt, const AcgSinkState* st, unsigned int* near_midpoint)
{
    *near_midpoint = 0;
    if (!st) return sink_fail(ctx, ACG_ESTATE, fmt, " sink is off");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
    HIPCHK(ctx, hipMemcpy(near_midpoint, st->d_cnt + 2, sizeof(unsigned int), hipMemcpyDeviceToHost));
    return ACG_OK;
}

// the order keys of the records the most recent fetch of a sink handed out: one small copy, no kernel
extern "C" int acg_sink_keys(acg_ctx* ctx, int sink, unsigned long long* keys, int max, int* n)
{
    if (!ctx || !n || max < 0 || (max > 0 && !keys) || (sink != ACG_SINK_JSON && sink != ACG_SINK_TEXT)) return ACG_EINVAL;
    *n = 0;
    const AcgSinkState* st = sink == ACG_SINK_JSON ? ctx->json : ctx->text;
    if (!st) return fail(ctx, ACG_ESTATE, (sink == ACG_SINK_JSON ? SINK_JSON : SINK_TEXT).is_off);
    *n = (int)st->last_nrecs;
    if (st->last_nrecs > (unsigned int)max) return fail(ctx, ACG_EAGAIN, "sink keys: *n keys do not fit");
    // (kept records sort in front of dropped ones: the first keys; the pass that wrote them has been waited for)
    if (st->last_nrecs && (hipSetDevice(ctx->cfg.device) != hipSuccess ||
                           hipMemcpy(keys, st->d_key_s, (size_t)st->last_nrecs * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess))
        return fail(ctx, ACG_EHIP, "sink keys: copy failed");
    return ACG_OK;
}

// records a lab entry may hand to a renderer
static bool sink_records_ok(const acg_msg* in, int n, int nch)
{
    for (int i = 0; i < n; ++i)
        if (in[i].chn < 0 || in[i].chn >= nch || in[i].end_bit < 0 || in[i].end_bit >= (1ll << 44)) return false;
    return true;
}

// the two sink selftests behind their argument checks: label pass and renderer over n records, no context
static int sink_selftest(const AcgSinkFormat* fmt, const SinkBlob& blob, const acg_msg* in, int n, const acg_msg_filter* f, int nch, char* out, size_t cap,
                         size_t* nbytes, unsigned int* offs, int* nrecs)
{
    AcgLabelFilter d;
    if (label_filter_dev(f, &d) != ACG_OK || !sink_records_ok(in, n, nch)) return ACG_EINVAL;
    *nbytes = 0;
    *nrecs = 0;
    if (n == 0) {
        if (offs) offs[0] = 0;
        return ACG_OK;
    }
    int ndev = 0;
    if (!fmt->launch || hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return ACG_ENODEV;
    AcgSinkState* st = nullptr;
    int rc = sink_create(&st, fmt, blob);
    if (rc != ACG_OK) return rc;
    rc = sink_reserve(st, (size_t)n);
    if (rc == ACG_OK) {
        LabStage lab((size_t)n);
        lab.stage(in, (unsigned int)n, true, true);
        const AcgSinkPass sp = sink_pass(st, lab.d_out, lab.d_oooi, lab.d_total(), (unsigned int)n, true);
        unsigned int cnt[2] = {0, 0};
        if (!lab.ok()) rc = ACG_ENOMEM;
        else if (lab.label((unsigned int)n, &d) != 0 || fmt->launch(&sp, nullptr) != 0 ||
                 hipMemcpy(cnt, st->d_cnt, sizeof(cnt), hipMemcpyDeviceToHost) != hipSuccess || cnt[1] > (unsigned int)n ||
                 (size_t)cnt[0] > (size_t)n * fmt->rec_max)
            rc = ACG_EHIP;
        if (rc == ACG_OK) {
            *nbytes = cnt[0];
            *nrecs = (int)cnt[1];
            if (cnt[0] > cap) rc = ACG_EAGAIN;
            else if ((cnt[0] && hipMemcpy(out, st->d_out, cnt[0], hipMemcpyDeviceToHost) != hipSuccess) ||
                     (offs && cnt[1] && hipMemcpy(offs, st->d_off, (size_t)cnt[1] * sizeof(unsigned int), hipMemcpyDeviceToHost) != hipSuccess))
                rc = ACG_EHIP;
            else if (offs) offs[cnt[1]] = cnt[0];
        }
    }
    sink_destroy(st);
    return rc;
}

// ---- the JSON sink: its configuration and entry points ------------------------------------------------------------------------
// print_string_ptr's escaping (cJSON.c:828-950) of a C string, appended to dst; returns the new length
static unsigned int json_escape(unsigned char* dst, unsigned int at, const char* s)
{
    for (; *s; ++s) {
        const unsigned char b = (unsigned char)*s;
        const char* two = b == '"' ? "\\\"" : b == '\\' ? "\\\\" : b == '\b' ? "\\b" : b == '\f' ? "\\f" : b == '\n' ? "\\n" : b == '\r' ? "\\r" :
                          b == '\t' ? "\\t" : nullptr;
        if (two) { dst[at++] = (unsigned char)two[0]; dst[at++] = (unsigned char)two[1]; }
        else if (b < 32) at += (unsigned int)std::snprintf((char*)dst + at, 7, "\\u%04x", b);
        else dst[at++] = b;
    }
    return at;
}

static unsigned int json_append(unsigned char* dst, unsigned int at, const char* lit)
{
    const size_t n = std::strlen(lit);
    std::memcpy(dst + at, lit, n);
    return at + (unsigned int)n;
}

static bool json_config_ok(const acg_json_config* c)
{
    return c && c->t0_sec >= 1000000000ll && c->t0_sec < 4000000000ll && c->t0_usec >= 0 && c->t0_usec <= 999999 &&
           std::memchr(c->station_id, 0, sizeof(c->station_id)) && std::memchr(c->app_name, 0, sizeof(c->app_name)) &&
           std::memchr(c->app_ver, 0, sizeof(c->app_ver));
}

// the constant stretches of a line, escaped, and the channels' "%3.3f" tokens; cfg has passed json_config_ok
static SinkBlob json_blob(const acg_json_config* cfg, const int* Fr_hz, int nch)
{
    SinkBlob b;
    AcgJsonDev h;
    std::memset(&h, 0, sizeof(h));
    h.t0_sec = cfg->t0_sec;
    h.t0_usec = cfg->t0_usec;
    h.nch = nch;
    if (cfg->station_id[0]) {                                     // output.c:246
        h.pre_len = json_append(h.pre, 0, ",\"station_id\":\"");
        h.pre_len = json_escape(h.pre, h.pre_len, cfg->station_id);
        h.pre_len = json_append(h.pre, h.pre_len, "\"");
    }
    h.post_len = json_append(h.post, 0, ",\"app\":{\"name\":\"");
    h.post_len = json_escape(h.post, h.post_len, cfg->app_name);
    h.post_len = json_append(h.post, h.post_len, "\",\"ver\":\"");
    h.post_len = json_escape(h.post, h.post_len, cfg->app_ver);
    h.post_len = json_append(h.post, h.post_len, "\"}}\n");
    if (h.pre_len > ACG_JS_PRE_MAX || h.post_len > ACG_JS_POST_MAX) b.rc = ACG_EINVAL;      // (cannot happen: 208 and 221)
    b.cfg.assign((const unsigned char*)&h, (const unsigned char*)&h + sizeof(h));
    b.freq.assign((size_t)nch * 8, 0);
    for (int c = 0; c < nch; ++c) {
        const float f = (float)((Fr_hz ? Fr_hz[c] : 0) / 1000000.0);                        // output.c:232
        char tmp[8];
        std::snprintf(tmp, sizeof(tmp), "%3.3f", f);                                        // output.c:248: cut to 7 characters
        const size_t n = std::strlen(tmp);
        std::memcpy(&b.freq[(size_t)c * 8], tmp, n);
        b.freq[(size_t)c * 8 + 7] = (unsigned char)n;
    }
    return b;
}

extern "C" int acg_json_enable(acg_ctx* ctx, const acg_json_config* cfg, const int* Fr_hz)
{
    if (!ctx) return ACG_EINVAL;
    if (!cfg) return sink_enable(ctx, &ctx->json, &SINK_JSON, nullptr);
    if (!json_config_ok(cfg)) return fail(ctx, ACG_EINVAL, "JSON sink: t0 outside [10^9, 4 * 10^9) s / 0..999999 us, or an unterminated string");
    const SinkBlob b = json_blob(cfg, Fr_hz, ctx->cfg.nch);
    return sink_enable(ctx, &ctx->json, &SINK_JSON, &b);
}

static int json_args(acg_ctx* ctx, char* out, size_t cap, size_t* nbytes, int* nlines)
{
    if (!ctx || !out || !nbytes || !nlines) return ACG_EINVAL;
    *nbytes = 0;
    *nlines = 0;
    if (cap < ACG_JSON_LINE_MAX) return fail(ctx, ACG_EINVAL, "JSON sink: the buffer holds less than one line (ACG_JSON_LINE_MAX)");
    return ACG_OK;
}

extern "C" int acg_collect_json(acg_ctx* ctx, int lag, char* out, size_t cap, size_t* nbytes, int* nlines)
{
    if (lag < 0 || lag >= acg_ctx::NCALL - 1) return ACG_EINVAL;
    if (const int rc = json_args(ctx, out, cap, nbytes, nlines)) return rc;
    return sink_fetch(ctx, &SINK_JSON, ctx->json, lag, out, cap, nbytes, nullptr, INT_MAX, nlines);
}

extern "C" int acg_drain_json(acg_ctx* ctx, char* out, size_t cap, size_t* nbytes, int* nlines)
{
    if (const int rc = json_args(ctx, out, cap, nbytes, nlines)) return rc;
    return sink_fetch(ctx, &SINK_JSON, ctx->json, DRAIN, out, cap, nbytes, nullptr, INT_MAX, nlines);
}

extern "C" int acg_lab_json_level_guard(acg_ctx* ctx, unsigned int* near_midpoint)
{
    if (!ctx || !near_midpoint) return ACG_EINVAL;
    return sink_level_guard(ctx, &SINK_JSON, ctx->json, near_midpoint);
}

extern "C" int acg_selftest_msg_json(const acg_msg* in, int n, const acg_msg_filter* f, const acg_json_config* cfg, const int* Fr_hz, int nch,
                                     char* out, size_t cap, size_t* nbytes, int* nlines)
{
    if (n < 0 || (n > 0 && !in) || !json_config_ok(cfg) || nch < 1 || nch > (1 << 20) || !nbytes || !nlines || (cap > 0 && !out) ||
        (unsigned int)n > SINK_JSON.max_take)
        return ACG_EINVAL;
    return sink_selftest(&SINK_JSON, json_blob(cfg, Fr_hz, nch), in, n, f, nch, out, cap, nbytes, nullptr, nlines);
}

// ---- the flight table's text (flight_text.hip; host side: flights.cpp): the monitor screen and the route lines ------------------
static_assert(ACG_FT_ROW_MAX == ACG_MONITOR_ROW_MAX && ACG_FT_LINE_MAX == ACG_ROUTE_LINE_MAX && ACG_FT_HDR_LEN == ACG_MONITOR_HDR_LEN, "record bounds");

static bool flight_text_config_ok(const acg_flight_text_config* c)
{
    return c && c->nbch >= 0 && c->nbch <= 16 && std::memchr(c->station_id, 0, sizeof(c->station_id));
}

// nbch and the station stretch of a route line, escaped as the JSON sink's; cfg has passed flight_text_config_ok
static AcgFlightTextDev flight_text_dev(const acg_flight_text_config* cfg)
{
    AcgFlightTextDev h;
    std::memset(&h, 0, sizeof(h));
    h.nbch = cfg->nbch;
    if (cfg->station_id[0]) {                                     // output.c:444
        h.pre_len = json_append(h.pre, 0, ",\"station_id\":\"");
        h.pre_len = json_escape(h.pre, h.pre_len, cfg->station_id);
        h.pre_len = json_append(h.pre, h.pre_len, "\"");          // (at most 208 of ACG_JS_PRE_MAX bytes)
    }
    return h;
}

extern "C" int acg_flight_text_enable(acg_ctx* ctx, const acg_flight_text_config* cfg)
{
    if (!ctx) return ACG_EINVAL;
    if (cfg && !flight_text_config_ok(cfg)) return fail(ctx, ACG_EINVAL, "flight text: nbch outside 0..16, or an unterminated station_id");
    if (!ctx->flights || !acg_fl_text_enable) return fail(ctx, ACG_ESTATE, "flight text: the flight table is off (acg_flights_enable first)");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
    if (!cfg) return acg_fl_text_enable(ctx->flights, nullptr);
    const AcgFlightTextDev h = flight_text_dev(cfg);
    const int rc = acg_fl_text_enable(ctx->flights, &h);
    return rc == ACG_OK ? rc : fail(ctx, rc, "flight text: allocation failed");
}

extern "C" int acg_flight_monitor_text(acg_ctx* ctx, long long hdr_soh_sample, char* out, size_t cap, size_t* nbytes, int* nrows, int* dropped)
{
    if (!ctx || !nbytes || !nrows || (cap > 0 && !out)) return ACG_EINVAL;
    *nbytes = 0;
    *nrows = 0;
    if (!ctx->flights) return fail(ctx, ACG_ESTATE, "flight table is off");
    if (!acg_fl_text_on(ctx->flights)) return fail(ctx, ACG_ESTATE, "flight text is off: acg_flight_text_enable first");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    const int rc = acg_fl_monitor_text(ctx->flights, ctx->copy_stream, hdr_soh_sample, out, cap, nbytes, nrows, dropped);
    return rc == ACG_OK ? rc : fail(ctx, rc, rc == ACG_EAGAIN ? "the frame does not fit: *nbytes says how many bytes it needs" : "monitor frame failed");
}

extern "C" int acg_drain_routes_json(acg_ctx* ctx, char* out, size_t cap, size_t* nbytes, int* nlines)
{
    if (!ctx || !nbytes || !nlines || (cap > 0 && !out)) return ACG_EINVAL;
    *nbytes = 0;
    *nlines = 0;
    if (!ctx->flights) return fail(ctx, ACG_ESTATE, "flight table is off");
    if (!acg_fl_text_on(ctx->flights)) return fail(ctx, ACG_ESTATE, "flight text is off: acg_flight_text_enable first");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    const int rc = acg_fl_routes_json(ctx->flights, ctx->copy_stream, out, cap, nbytes, nlines);
    return rc == ACG_OK ? rc : fail(ctx, rc, rc == ACG_EAGAIN ? "the route lines do not fit: *nbytes says how many bytes they need" :
                                             rc == ACG_ESTATE ? "routes are pending from an acg_drain_routes that returned ACG_EAGAIN: drain them there first" :
                                                                "route lines failed");
}

extern "C" int acg_selftest_flight_text(const acg_flight* in, int n, const acg_route* rt, int nr, const acg_flight_config* cfg,
                                        const acg_flight_text_config* tcfg, long long hdr_soh_sample, char* mon, size_t mon_cap, size_t* mon_nbytes,
                                        int* nrows, char* rts, size_t rts_cap, size_t* rts_nbytes, int* nlines)
{
    if (n < 0 || nr < 0 || n > (1 << 24) || (n > 0 && !in) || (nr > 0 && !rt) || !acg_fl_config_ok(cfg) || !flight_text_config_ok(tcfg) || !mon_nbytes ||
        !nrows || !rts_nbytes || !nlines || (mon_cap > 0 && !mon) || (rts_cap > 0 && !rts))
        return ACG_EINVAL;
    *mon_nbytes = *rts_nbytes = 0;
    *nrows = *nlines = 0;
    int ndev = 0;
    if (!acg_fl_create || hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return ACG_ENODEV;
    acg_flight_config c = *cfg;
    c.max_flights = std::max(c.max_flights, std::max(n, 1));
    AcgFlights* t = nullptr;
    int rc = acg_fl_create(&t, &c);
    if (rc != ACG_OK) return rc;
    const AcgFlightTextDev h = flight_text_dev(tcfg);
    rc = acg_fl_text_enable(t, &h);
    if (rc == ACG_OK) rc = acg_fl_load_designed(t, in, n, rt, nr);
    if (rc == ACG_OK) {
        const int rm = acg_fl_monitor_text(t, nullptr, hdr_soh_sample, mon, mon_cap, mon_nbytes, nrows, nullptr);
        const int rr = (rm == ACG_OK || rm == ACG_EAGAIN) ? acg_fl_routes_json(t, nullptr, rts, rts_cap, rts_nbytes, nlines) : rm;
        rc = (rr == ACG_OK || rr == ACG_EAGAIN) ? (rm != ACG_OK ? rm : rr) : rr;
    }
    acg_fl_destroy(t);
    return rc;
}

// ---- the text sink: its configuration and entry points ------------------------------------------------------------------------
static bool text_config_ok(const acg_text_config* c)
{
    if (!c || c->format < ACG_TEXT_ONELINE || c->format > ACG_TEXT_SV) return false;
    const unsigned int takes = c->format == ACG_TEXT_ONELINE ? ACG_TEXT_F_DATE : c->format == ACG_TEXT_STD ? (ACG_TEXT_F_DATE | ACG_TEXT_F_FREQ) : 0u;
    return !(c->flags & ~takes) && c->t0_sec >= 1000000000ll && c->t0_sec < 4000000000ll && c->t0_usec >= 0 && c->t0_usec <= 999999 &&
           std::memchr(c->station_id, 0, sizeof(c->station_id));
}

// format, flags, SV's station and the channels' "F:%3.3f " tokens; cfg has passed text_config_ok
static SinkBlob text_blob(const acg_text_config* cfg, const int* Fr_hz, int nch)
{
    SinkBlob b;
    AcgTextDev h;
    std::memset(&h, 0, sizeof(h));
    h.t0_sec = cfg->t0_sec;
    h.t0_usec = cfg->t0_usec;
    h.nch = nch;
    h.format = cfg->format;
    h.flags = cfg->flags;
    char st8[40];
    h.station_len = (unsigned int)std::snprintf(st8, sizeof(st8), "%8s", cfg->station_id);      // netout.c:131
    if (h.station_len > sizeof(h.station)) { b.rc = ACG_EINVAL; return b; }                      // (cannot happen: 32 characters)
    std::memcpy(h.station, st8, h.station_len);
    b.cfg.assign((const unsigned char*)&h, (const unsigned char*)&h + sizeof(h));
    b.freq.assign((size_t)nch * ACG_TX_FREQ_SLOT, 0);
    for (int c = 0; c < nch; ++c) {
        char tmp[32];
        const int n = std::snprintf(tmp, sizeof(tmp), "F:%3.3f ", (Fr_hz ? Fr_hz[c] : 0) / 1000000.0);   // output.c:168-169: a double
        if (n < 0 || n >= ACG_TX_FREQ_SLOT) { b.rc = ACG_EINVAL; return b; }                     // (cannot happen: an int's 12 characters)
        std::memcpy(&b.freq[(size_t)c * ACG_TX_FREQ_SLOT], tmp, (size_t)n);
        b.freq[(size_t)c * ACG_TX_FREQ_SLOT + ACG_TX_FREQ_SLOT - 1] = (unsigned char)n;
    }
    return b;
}

extern "C" int acg_text_enable(acg_ctx* ctx, const acg_text_config* cfg, const int* Fr_hz)
{
    if (!ctx) return ACG_EINVAL;
    if (!cfg) return sink_enable(ctx, &ctx->text, &SINK_TEXT, nullptr);
    if (!text_config_ok(cfg))
        return fail(ctx, ACG_EINVAL, "text sink: unknown format, a flag the format does not take, t0 outside [10^9, 4 * 10^9) s / 0..999999 us, or an unterminated station_id");
    const SinkBlob b = text_blob(cfg, Fr_hz, ctx->cfg.nch);
    return sink_enable(ctx, &ctx->text, &SINK_TEXT, &b);
}

static int text_args(acg_ctx* ctx, char* out, size_t cap, size_t* nbytes, unsigned int* offs, int max_recs, int* nrecs)
{
    if (!ctx || !out || !nbytes || !offs || !nrecs) return ACG_EINVAL;
    *nbytes = 0;
    *nrecs = 0;
    offs[0] = 0;
    if (cap < ACG_TEXT_REC_MAX || max_recs < 1) return fail(ctx, ACG_EINVAL, "text sink: the buffer holds less than one record (ACG_TEXT_REC_MAX), or max_recs < 1");
    return ACG_OK;
}

extern "C" int acg_collect_text(acg_ctx* ctx, int lag, char* out, size_t cap, size_t* nbytes, unsigned int* offs, int max_recs, int* nrecs)
{
    if (lag < 0 || lag >= acg_ctx::NCALL - 1) return ACG_EINVAL;
    if (const int rc = text_args(ctx, out, cap, nbytes, offs, max_recs, nrecs)) return rc;
    return sink_fetch(ctx, &SINK_TEXT, ctx->text, lag, out, cap, nbytes, offs, max_recs, nrecs);
}

extern "C" int acg_drain_text(acg_ctx* ctx, char* out, size_t cap, size_t* nbytes, unsigned int* offs, int max_recs, int* nrecs)
{
    if (const int rc = text_args(ctx, out, cap, nbytes, offs, max_recs, nrecs)) return rc;
    return sink_fetch(ctx, &SINK_TEXT, ctx->text, DRAIN, out, cap, nbytes, offs, max_recs, nrecs);
}

extern "C" int acg_lab_text_level_guard(acg_ctx* ctx, unsigned int* near_midpoint)
{
    if (!ctx || !near_midpoint) return ACG_EINVAL;
    return sink_level_guard(ctx, &SINK_TEXT, ctx->text, near_midpoint);
}

extern "C" int acg_selftest_msg_text(const acg_msg* in, int n, const acg_msg_filter* f, const acg_text_config* cfg, const int* Fr_hz, int nch,
                                     char* out, size_t cap, size_t* nbytes, unsigned int* offs, int* nrecs)
{
    if (n < 0 || (n > 0 && !in) || !text_config_ok(cfg) || nch < 1 || nch > (1 << 20) || !nbytes || !nrecs || !offs || (cap > 0 && !out) ||
        (unsigned int)n > SINK_TEXT.max_take)
        return ACG_EINVAL;
    return sink_selftest(&SINK_TEXT, text_blob(cfg, Fr_hz, nch), in, n, f, nch, out, cap, nbytes, offs, nrecs);
}

extern "C" int acg_lab_time_sink_passes(const acg_msg* in, int n, const acg_json_config* jcfg, const acg_text_config* tcfg, int nch, int warmup,
                                        int reps, float* ms)
{
    if (n < 1 || !in || !json_config_ok(jcfg) || !text_config_ok(tcfg) || nch < 1 || nch > (1 << 20) || warmup < 0 || reps < 1 || !ms ||
        (unsigned int)n > std::min(SINK_JSON.max_take, SINK_TEXT.max_take) || !sink_records_ok(in, n, nch))
        return ACG_EINVAL;
    int ndev = 0;
    if (!acg_launch_json || !acg_launch_text || hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return ACG_ENODEV;
    AcgSinkState* st[2] = {nullptr, nullptr};                      // the arms: JSON, text
    AcgLabelFilter none;
    std::memset(&none, 0, sizeof(none));
    hipEvent_t ev[2] = {nullptr, nullptr};
    int* d_map = nullptr;
    int rc = sink_create(&st[0], &SINK_JSON, json_blob(jcfg, nullptr, nch));
    if (rc == ACG_OK) rc = sink_create(&st[1], &SINK_TEXT, text_blob(tcfg, nullptr, nch));
    if (rc == ACG_OK) rc = sink_reserve(st[0], (size_t)n);
    if (rc == ACG_OK) rc = sink_reserve(st[1], (size_t)n);
    if (rc == ACG_OK) {
        LabStage lab((size_t)n);
        lab.stage(in, (unsigned int)n, true, true);
        if (!lab.ok()) rc = ACG_ENOMEM;
        if (rc == ACG_OK && acg_tune_get("ACG_SINK_MAP", 0)) {    // the passes under a channel map (slot l -> nch - 1 - l): what the look-up costs
            std::vector<int> m((size_t)nch);
            for (int l = 0; l < nch; ++l) m[(size_t)l] = nch - 1 - l;
            if (hipMalloc(&d_map, m.size() * sizeof(int)) != hipSuccess || hipMemcpy(d_map, m.data(), m.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
                rc = ACG_EHIP;
        }
        if (rc == ACG_OK && (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess)) rc = ACG_EHIP;
        if (rc == ACG_OK && (lab.label((unsigned int)n, &none) != 0 || hipDeviceSynchronize() != hipSuccess)) rc = ACG_EHIP;
        for (int r = -warmup; r < reps && rc == ACG_OK; ++r)
            for (int arm = 0; arm < 2 && rc == ACG_OK; ++arm) {
                AcgSinkPass sp = sink_pass(st[arm], lab.d_out, lab.d_oooi, lab.d_total(), (unsigned int)n, true);
                sp.chmap = d_map;
                sp.nmap = d_map ? (unsigned int)nch : 0u;
                float t = 0.0f;
                if (hipEventRecord(ev[0], nullptr) != hipSuccess || st[arm]->fmt->launch(&sp, nullptr) != 0 ||
                    hipEventRecord(ev[1], nullptr) != hipSuccess || hipEventSynchronize(ev[1]) != hipSuccess ||
                    hipEventElapsedTime(&t, ev[0], ev[1]) != hipSuccess)
                    rc = ACG_EHIP;
                else if (r >= 0) ms[arm * reps + r] = t;
            }
    }
    if (ev[0]) hipEventDestroy(ev[0]);
    if (ev[1]) hipEventDestroy(ev[1]);
    hipFree(d_map);
    sink_destroy(st[0]);
    sink_destroy(st[1]);
    return rc;
}

extern "C" int acg_bit_capacity(const acg_ctx* ctx) { return ctx ? ctx->bit_cap : 0; }
extern "C" int acg_max_lag(const acg_ctx* ctx) { return ctx ? ctx->lag_max : 0; }

// ------------------------------------------------------------------------------------------
// Per-channel reception statistics (stats.hip)
extern "C" int acg_stats_enable(acg_ctx* ctx, int on)
{
    if (!ctx) return ACG_EINVAL;
    if (!acg_launch_chan_stats) return fail(ctx, ACG_ESTATE, "no statistics unit");
    if (!ctx->d_crctab) return fail(ctx, ACG_ESTATE, "context created without ACG_F_REPAIR");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    if (!on) {
        hipFree(ctx->d_stats);
        ctx->d_stats = nullptr;
        ctx->lost_blocks = 0;
        return ACG_OK;
    }
    if (!ctx->d_stats) HIPCHK(ctx, hipMalloc(&ctx->d_stats, (size_t)ctx->cfg.nch * sizeof(AcgChanStats)));
    return stats_zero(ctx);
}

extern "C" int acg_stats_read(acg_ctx* ctx, int ch0, int n, acg_chan_stats* out, unsigned long long* lost_blocks)
{
    if (!ctx) return ACG_EINVAL;
    if (!ctx->d_stats) return fail(ctx, ACG_ESTATE, "statistics are off");
    if (ch0 < 0 || n < 0 || ch0 > ctx->cfg.nch || n > ctx->cfg.nch - ch0 || (n > 0 && !out)) return fail(ctx, ACG_EINVAL, "statistics: bad channel range");
    static_assert(sizeof(AcgChanStats) == sizeof(acg_chan_stats), "device and public statistics record must have one layout");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    if (n) HIPCHK(ctx, hipMemcpy(out, ctx->d_stats + ch0, (size_t)n * sizeof(AcgChanStats), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {                                 // the device's encodings, chosen so that zero means "none yet"
        unsigned long long inv;
        std::memcpy(&inv, &out[i].lvl_min, sizeof(inv));
        inv = inv ? ~inv : 0ull;                                  // (lvl_max_bits is the ratio's own bit pattern)
        std::memcpy(&out[i].lvl_min, &inv, sizeof(inv));
        out[i].last_end_sample -= 1;
    }
    if (lost_blocks) *lost_blocks = ctx->lost_blocks;
    return ACG_OK;
}

extern "C" int acg_read_bits(acg_ctx* ctx, int ch, float* vo, float* lvl, int max_bits, int* nbits)
{
    if (!ctx || !nbits || ch < 0 || ch >= ctx->cfg.nch) return ACG_EINVAL;
    if (!ctx->d_bits) return fail(ctx, ACG_ESTATE, "context created without ACG_F_BITLOG");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    int n = 0;
    HIPCHK(ctx, hipMemcpy(&n, ctx->d_nbits + ch, sizeof(int), hipMemcpyDeviceToHost));
    *nbits = n;
    const int m = std::min(std::min(n, ctx->bit_cap), max_bits);
    if (m > 0) {
        std::vector<float2> tmp((size_t)m);
        HIPCHK(ctx, hipMemcpy(tmp.data(), ctx->d_bits + (size_t)ch * ctx->bit_cap, (size_t)m * sizeof(float2),
                              hipMemcpyDeviceToHost));
        for (int i = 0; i < m; ++i) {
            if (vo) vo[i] = tmp[(size_t)i].x;
            if (lvl) lvl[i] = tmp[(size_t)i].y;
        }
    }
    return n > ctx->bit_cap ? ACG_EOVERFLOW : ACG_OK;
}

extern "C" int acg_read_bits_all(acg_ctx* ctx, int* counts, float* vo, float* lvl)
{
    if (!ctx || !counts) return ACG_EINVAL;
    if (!ctx->d_bits) return fail(ctx, ACG_ESTATE, "context created without ACG_F_BITLOG");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    const size_t nch = (size_t)ctx->cfg.nch, cap = (size_t)ctx->bit_cap;
    HIPCHK(ctx, hipMemcpy(counts, ctx->d_nbits, nch * sizeof(int), hipMemcpyDeviceToHost));
    if (vo || lvl) {
        std::vector<float2> tmp(nch * cap);
        HIPCHK(ctx, hipMemcpy(tmp.data(), ctx->d_bits, tmp.size() * sizeof(float2), hipMemcpyDeviceToHost));
        for (size_t c = 0; c < nch; ++c) {
            const size_t m = (size_t)std::min<int>(counts[c], (int)cap);
            for (size_t i = 0; i < m; ++i) {
                if (vo) vo[c * cap + i] = tmp[c * cap + i].x;
                if (lvl) lvl[c * cap + i] = tmp[c * cap + i].y;
            }
        }
    }
    return ACG_OK;
}

extern "C" int acg_replay_bits(acg_ctx* ctx, acg_bit_sink sink, void* user)
{
    if (!ctx || !sink) return ACG_EINVAL;
    if (!ctx->d_bits) return fail(ctx, ACG_ESTATE, "context created without ACG_F_BITLOG");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    const size_t nch = (size_t)ctx->cfg.nch, cap = (size_t)ctx->bit_cap;
    std::vector<int> counts(nch);
    HIPCHK(ctx, hipMemcpy(counts.data(), ctx->d_nbits, nch * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<float2> tmp(nch * cap);
    HIPCHK(ctx, hipMemcpy(tmp.data(), ctx->d_bits, tmp.size() * sizeof(float2), hipMemcpyDeviceToHost));
    int rc = ACG_OK;
    for (size_t c = 0; c < nch; ++c) {
        if (counts[c] > (int)cap) rc = ACG_EOVERFLOW;
        const size_t m = (size_t)std::min<int>(counts[c], (int)cap);
        for (size_t i = 0; i < m; ++i) sink(user, (int)c, tmp[c * cap + i].x, tmp[c * cap + i].y);
    }
    return rc;
}

extern "C" int acg_read_dm_n(acg_ctx* ctx, int ch0, int n, float* dm, size_t pitch_floats, int nfloats)
{
    if (!ctx || !dm || ch0 < 0 || n < 1 || ch0 + n > ctx->cfg.nch || nfloats < 0 || nfloats > ctx->max_len ||
        (n > 1 && pitch_floats < (size_t)nfloats))
        return ACG_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    if (nfloats)
        HIPCHK(ctx, hipMemcpy2D(dm, pitch_floats * sizeof(float), ctx->d_dm + (size_t)ch0 * ctx->dm_pitch, ctx->dm_pitch * sizeof(float),
                                (size_t)nfloats * sizeof(float), (size_t)n, hipMemcpyDeviceToHost));
    return ACG_OK;
}

extern "C" int acg_read_dm(acg_ctx* ctx, int ch, float* dm, int n)
{
    return acg_read_dm_n(ctx, ch, 1, dm, (size_t)(n > 0 ? n : 0), n);
}

static void state_from_dev(const AcgChan& d, acg_chan_state* st)
{
    st->MskPhi = d.phi; st->MskDf = d.df; st->MskLvlSum = d.lvlsum; st->MskClk = d.clk;
    st->MskBitCount = d.bitcount; st->MskS = d.S; st->idx = d.idx;
    std::memcpy(st->inb, d.inb, sizeof(d.inb));
    st->outbits = (int)d.outbits; st->nbits = d.nbits; st->Acarsstate = d.astate;
    st->blk_len = d.blen; st->blk_err = d.berr;
    // the SOH stamp as a distance (the sample counter is the slot's own, the distance travels): ADVICE r05
    const unsigned int back = (unsigned int)d.nsamp_total - d.soh32;
    st->soh_back = (d.astate >= 3 && d.astate <= 5 && back < 65536u) ? (int)back : 0;
}

// channels ch0 .. ch0+n-1 in one transfer (the legacy view moves all channels of a dongle per callback)
extern "C" int acg_get_state_n(acg_ctx* ctx, int ch0, int n, acg_chan_state* st)
{
    if (!ctx || !st || ch0 < 0 || n < 1 || ch0 + n > ctx->cfg.nch) return ACG_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    std::vector<AcgChan> d((size_t)n);
    HIPCHK(ctx, hipMemcpy(d.data(), ctx->d_st + ch0, (size_t)n * sizeof(AcgChan), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) state_from_dev(d[(size_t)i], st + i);
    return ACG_OK;
}

extern "C" int acg_get_state(acg_ctx* ctx, int ch, acg_chan_state* st) { return acg_get_state_n(ctx, ch, 1, st); }

extern "C" int acg_set_state_n(acg_ctx* ctx, int ch0, int n, const acg_chan_state* st)
{
    if (!ctx || !st || ch0 < 0 || n < 1 || ch0 + n > ctx->cfg.nch) return ACG_EINVAL;
    for (int i = 0; i < n; ++i) {
        if (st[i].idx >= ACG_FLEN) return fail(ctx, ACG_EINVAL, "idx out of range");
        // blk_len indexes the channel's 256-byte text row on the device (acars.c:304 `blk->txt[blk->len] = r`; the reference resets a
        // block beyond 240 bytes, acars.c:336): a length no decodeAcars() leaves behind is refused instead of written through
        if (st[i].blk_len < 0 || st[i].blk_len > 241) return fail(ctx, ACG_EINVAL, "blk_len out of range");
    }
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    // read-modify-write: the bookkeeping that is not part of channel_t (bit / sample counters, the held CRC byte) stays as the
    // device has it; the SOH stamp is re-based on this slot's sample counter from the distance the caller brings
    std::vector<AcgChan> dv((size_t)n);
    HIPCHK(ctx, hipMemcpy(dv.data(), ctx->d_st + ch0, (size_t)n * sizeof(AcgChan), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
        AcgChan& d = dv[(size_t)i];
        const acg_chan_state& t = st[i];
        d.phi = t.MskPhi; d.df = t.MskDf; d.lvlsum = t.MskLvlSum; d.clk = t.MskClk;
        d.bitcount = t.MskBitCount; d.S = t.MskS; d.idx = t.idx;
        std::memcpy(d.inb, t.inb, sizeof(d.inb));
        d.outbits = (unsigned int)t.outbits & 0xffu; d.nbits = t.nbits; d.astate = t.Acarsstate;
        d.blen = t.blk_len; d.berr = t.blk_err;
        d.soh32 = (unsigned int)d.nsamp_total - (unsigned int)(t.soh_back > 0 && t.soh_back < 65536 ? t.soh_back : 0);
    }
    HIPCHK(ctx, hipMemcpy(ctx->d_st + ch0, dv.data(), (size_t)n * sizeof(AcgChan), hipMemcpyHostToDevice));
    return ACG_OK;
}

extern "C" int acg_set_state(acg_ctx* ctx, int ch, const acg_chan_state* st) { return acg_set_state_n(ctx, ch, 1, st); }

// blk->txt being assembled (the device keeps 256 bytes per channel, ACG_TXTMAX of them are the reference's msgblk_t::txt)
extern "C" int acg_get_block_text(acg_ctx* ctx, int ch, unsigned char* txt)
{
    if (!ctx || !txt || ch < 0 || ch >= ctx->cfg.nch) return ACG_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    HIPCHK(ctx, hipMemcpy(txt, ctx->d_txt + (size_t)ch * 256, ACG_TXTMAX, hipMemcpyDeviceToHost));
    return ACG_OK;
}

extern "C" int acg_set_block_text(acg_ctx* ctx, int ch, const unsigned char* txt)
{
    if (!ctx || !txt || ch < 0 || ch >= ctx->cfg.nch) return ACG_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    HIPCHK(ctx, hipMemcpy(ctx->d_txt + (size_t)ch * 256, txt, ACG_TXTMAX, hipMemcpyHostToDevice));
    return ACG_OK;
}

// ---- lab: the block counters next to their wrap (acarsdec_amd_lab.h) ----------------------------------------------------
extern "C" int acg_lab_set_block_counter(acg_ctx* ctx, unsigned int value)
{
    if (!ctx) return ACG_EINVAL;
    if (ctx->call_seq != 0) return fail(ctx, ACG_ESTATE, "acg_lab_set_block_counter: only right after acg_reset");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    HIPCHK(ctx, hipMemcpy(ctx->d_frame_count, &value, sizeof(value), hipMemcpyHostToDevice));
    if (ctx->d_rep_upto) HIPCHK(ctx, hipMemcpy(ctx->d_rep_upto, &value, sizeof(value), hipMemcpyHostToDevice));
    for (int i = 0; i < acg_ctx::NCALL; ++i) ctx->h_call_count[i] = value;
    ctx->consumed = value;
    HIPCHK(ctx, hipDeviceSynchronize());
    return ACG_OK;
}
extern "C" unsigned int acg_lab_block_ring_size(const acg_ctx* ctx) { return ctx ? ctx->frame_cap : 0u; }

// ---- lab: the stream counters after days of uptime (acarsdec_amd_lab.h) -------------------------------------------------
extern "C" int acg_lab_set_stream_counters(acg_ctx* ctx, int ch0, int n, long long nsamp_total, long long nbit_total)
{
    if (!ctx || ch0 < 0 || n < 1 || ch0 + n > ctx->cfg.nch || nsamp_total < 0 || nbit_total < 0) return ACG_EINVAL;
    if (ctx->call_seq != 0) return fail(ctx, ACG_ESTATE, "acg_lab_set_stream_counters: only right after acg_reset");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    // read-modify-write, as acg_set_state_n: everything but the three counters stays as the device has it
    std::vector<AcgChan> dv((size_t)n);
    HIPCHK(ctx, hipMemcpy(dv.data(), ctx->d_st + ch0, (size_t)n * sizeof(AcgChan), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
        AcgChan& d = dv[(size_t)i];
        d.nsamp_total = nsamp_total;
        d.nbit_total = nbit_total;
        d.soh32 = (unsigned int)nsamp_total;
    }
    HIPCHK(ctx, hipMemcpy(ctx->d_st + ch0, dv.data(), (size_t)n * sizeof(AcgChan), hipMemcpyHostToDevice));
    return ACG_OK;
}

// ---- lab: the down-converter launch of `nblocks` callbacks, as the launcher decides it ---------------------------------------
extern "C" int acg_lab_fir_launch_shape(acg_ctx* ctx, int nblocks, acg_lab_launch_shape* out)
{
    if (!ctx || !out) return ACG_EINVAL;
    if (nblocks < 1 || nblocks > ctx->cfg.max_blocks) return fail(ctx, ACG_EINVAL, "nblocks out of range");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    std::memset(out, 0, sizeof *out);
    (void)hipDeviceGetAttribute(&out->device_cus, hipDeviceAttributeMultiprocessorCount, ctx->cfg.device);
    // the arguments of run_pipeline's launch: the format's, the chunk's window count, the partition's CU count
    FirArgs a = u8_args(ctx, nullptr, 0);
    a.nwin = nblocks * ACG_BLOCK;
    if (ctx->fir_stream) a.ncu = ctx->fir_ncu;
    out->ncu = a.ncu > 0 ? a.ncu : out->device_cus;
    out->chunk_blocks = ctx->pipe_blocks;
    const FirU8Kernel k = fir_u8_kernel(ctx, a);
    if (k != FIR_U8_MM && k != FIR_U8_MM1) return ACG_OK;
    const MmPlan p = k == FIR_U8_MM ? acg_fir_mm_plan(&a, out->device_cus) : acg_fir_mm1_plan(&a, out->device_cus);
    out->kernel = p.kernel;
    out->stages = p.stages;
    out->cpr = p.cpr;
    out->ncu = p.ncu;
    out->units = p.units;
    out->runs_per_unit = p.runs_per_unit;
    out->tiles_per_run = p.tiles_per_run;
    out->runs = p.runs;
    out->wave_slots = p.wave_slots;
    out->workgroups = p.workgroups;
    out->waves = p.waves;
    return ACG_OK;
}

extern "C" int acg_set_timing(acg_ctx* ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 2) return ACG_EINVAL;
    ctx->timing_mode = mode;
    return ACG_OK;
}

extern "C" int acg_get_timing(acg_ctx* ctx, double* fir_ms, int* fir_launches, double* msk_ms, int* msk_launches)
{
    if (!ctx) return ACG_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    auto sum = [&](std::vector<EvPair>& v, double* ms, int* n) -> int {
        double t = 0;
        for (auto& p : v) {
            float f = 0;
            HIPCHK(ctx, hipEventElapsedTime(&f, p.a, p.b));
            t += f;
            ctx->ev_pool.push_back(p.a);
            ctx->ev_pool.push_back(p.b);
        }
        if (ms) *ms = t;
        if (n) *n = (int)v.size();
        v.clear();
        return ACG_OK;
    };
    int r = sum(ctx->fir_ev, fir_ms, fir_launches);
    if (r != ACG_OK) return r;
    return sum(ctx->msk_ev, msk_ms, msk_launches);
}

// ------------------------------------------------------------------------------------------
// The other front ends' sample formats: soapy.c (CS16), sdrplay.c (split int16),
// air.c (real f32).  Same tile kernel, 4 bytes per input sample.
static int fmt_args(acg_ctx* ctx, int fmt, FirArgs* a)
{
    const acg_config& g = ctx->cfg;
    if (fmt < ACG_FMT_CS16 || fmt > ACG_FMT_F32_REAL) return fail(ctx, ACG_EINVAL, "unknown sample format");
    if (g.decim % (fmt == ACG_FMT_S16_SPLIT ? 8 : 4) || (fmt == ACG_FMT_S16_SPLIT && g.decim > 208))
        return fail(ctx, ACG_EINVAL, "this sample format needs decim % 4 == 0 (split planes: % 8 and <= 208)");
    if (ctx->ntaps_pad % (fmt == ACG_FMT_S16_SPLIT ? 8 : 4))
        return fail(ctx, ACG_EINVAL, "this sample format needs ntaps % 4 == 0 when decim % 8 != 0");
    *a = fir_args(ctx);
    a->row_bytes = 4 * g.decim;
    a->cpr_total = a->row_bytes / 16;
    a->kseg = (a->cpr_total + 51) / 52;                 // LDS slice <= 52 chunks per window (Airspy: 480 -> 3 x 40, 800 -> 4 x 50)
    a->cpr = (a->cpr_total + a->kseg - 1) / a->kseg;
    a->row_stride = 16 * ((a->cpr & 1) ? a->cpr : a->cpr + 1);
    a->cpr_magic = ((1u << 20) + (unsigned int)a->cpr - 1) / (unsigned int)a->cpr;
    a->nseg = 1;
    a->out_scale = fmt == ACG_FMT_CS16 ? 1.0f / 32768.0f : fmt == ACG_FMT_S16_SPLIT ? 0.25f : 1.0f;
    return ACG_OK;
}

// pipeline chunk of the formats: 4-byte samples, half the callbacks per ~2 GB
static int fmt_chunk_win(const acg_ctx* ctx)
{
    return (ctx->pipe_blocks > 0 ? (ctx->pipe_blocks + 1) / 2 : ctx->cfg.max_blocks) * ACG_BLOCK;
}

extern "C" int acg_process_samples_dev(acg_ctx* ctx, int fmt, const void* dev, size_t pitch_bytes, size_t plane_bytes,
                                       int nblocks, void* hip_stream)
{
    if (!ctx || !dev) return ACG_EINVAL;
    if (nblocks < 1 || nblocks > ctx->cfg.max_blocks) return fail(ctx, ACG_EINVAL, "nblocks out of range");
    if ((((uintptr_t)dev | pitch_bytes | plane_bytes) & 15)) return fail(ctx, ACG_EINVAL, "base, pitch and plane must be 16-byte aligned");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    FirArgs a;
    int r = fmt_args(ctx, fmt, &a);
    if (r != ACG_OK) return r;
    a.iq = (const uint8_t*)dev;
    a.pitch = pitch_bytes;
    a.plane = plane_bytes;
    const size_t win_bytes = (size_t)ctx->cfg.decim * (fmt == ACG_FMT_S16_SPLIT ? 2 : 4);      // of one plane
    return run_pipeline(ctx, hip_stream ? (hipStream_t)hip_stream : ctx->stream, a, win_bytes, nblocks * ACG_BLOCK, fmt_chunk_win(ctx),
                        [fmt](acg_ctx*, FirArgs& f, hipStream_t s) { return acg_launch_fir_fmt(&f, fmt, s); });
}

// Host feed with carry: windows may straddle feeds of any size (soapy.c:232-254, sdrplay.c:215-236,
// air.c:299-338 carry D / the index across buffers; here the incomplete window's SAMPLES wait at the
// head of a device staging row -- the sums are then the same sequential windows).
extern "C" int acg_feed_samples_host(acg_ctx* ctx, int fmt, const void* p0, const void* p1, size_t pitch_samples,
                                     size_t nsamples)
{
    if (!ctx || !p0 || (fmt == ACG_FMT_S16_SPLIT && !p1)) return ACG_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    FirArgs a;
    int r = fmt_args(ctx, fmt, &a);
    if (r != ACG_OK) return r;
    if (ctx->feed_fmt != fmt) { ctx->feed_fmt = fmt; ctx->feed_fill = 0; }
    const acg_config& g = ctx->cfg;
    const size_t M = (size_t)g.decim;
    const size_t bps = fmt == ACG_FMT_S16_SPLIT ? 2 : 4;                     // bytes per sample per plane
    const size_t cap = (size_t)ctx->max_len * M;                              // samples a staging row holds (<= max_len windows per launch)
    const size_t plane = ((cap * bps) + 15) & ~(size_t)15;
    const size_t rowb = fmt == ACG_FMT_S16_SPLIT ? 2 * plane : plane;
    if ((r = ensure_stage(ctx, rowb * (size_t)g.nstreams)) != ACG_OK) return r;
    hipStream_t s = ctx->stream, hs = ctx->h2d_stream;
    size_t done = 0;
    while (done < nsamples) {
        const size_t take = std::min(nsamples - done, cap - ctx->feed_fill);
        const int cur = ctx->feed_cur;
        unsigned char* base = (unsigned char*)ctx->d_stage[cur];
        // new samples behind the carried ones, on the copy stream (which already waits for the last reader of this buffer
        // and carries the copy of the carried samples: both were enqueued when the buffer became the current one)
        HIPCHK(ctx, hipMemcpy2DAsync(base + ctx->feed_fill * bps, rowb, (const unsigned char*)p0 + done * bps,
                                     (g.nstreams > 1 ? pitch_samples : nsamples) * bps, take * bps, (size_t)g.nstreams,
                                     hipMemcpyHostToDevice, hs));
        if (fmt == ACG_FMT_S16_SPLIT)
            HIPCHK(ctx, hipMemcpy2DAsync(base + plane + ctx->feed_fill * bps, rowb, (const unsigned char*)p1 + done * bps,
                                         (g.nstreams > 1 ? pitch_samples : nsamples) * bps, take * bps, (size_t)g.nstreams,
                                         hipMemcpyHostToDevice, hs));
        HIPCHK(ctx, hipEventRecord(ctx->h2d_done, hs));
        done += take;
        const size_t have = ctx->feed_fill + take;
        const size_t nwin = have / M;
        if (nwin > 0) {
            HIPCHK(ctx, hipStreamWaitEvent(s, ctx->h2d_done, 0));
            a.iq = base;
            a.pitch = rowb;
            a.plane = plane;
            if ((r = run_pipeline(ctx, s, a, M * bps, (int)nwin, fmt_chunk_win(ctx),
                                  [fmt](acg_ctx*, FirArgs& f, hipStream_t st) { return acg_launch_fir_fmt(&f, fmt, st); })) != ACG_OK) {
                (void)hipEventSynchronize(ctx->h2d_done);   // the copy may still be reading the caller's buffers: not after we return
                return r;
            }
            HIPCHK(ctx, hipEventRecord(ctx->stage_free[cur], s));      // behind the last down-converter launch that reads `cur`
            ctx->stage_free_valid[cur] = true;
            // the other buffer becomes the current one: once its last reader (the launches of the feed before this one) is
            // done, the < M samples of the incomplete window move to its head -- on the copy stream, beside the kernels
            const int nxt = cur ^ 1;
            const size_t left = have - nwin * M;
            if (ctx->stage_free_valid[nxt]) HIPCHK(ctx, hipStreamWaitEvent(hs, ctx->stage_free[nxt], 0));
            if (left) {
                unsigned char* nb = (unsigned char*)ctx->d_stage[nxt];
                HIPCHK(ctx, hipMemcpy2DAsync(nb, rowb, base + nwin * M * bps, rowb, left * bps, (size_t)g.nstreams,
                                             hipMemcpyDeviceToDevice, hs));
                if (fmt == ACG_FMT_S16_SPLIT)
                    HIPCHK(ctx, hipMemcpy2DAsync(nb + plane, rowb, base + plane + nwin * M * bps, rowb, left * bps,
                                                 (size_t)g.nstreams, hipMemcpyDeviceToDevice, hs));
            }
            ctx->feed_fill = left;
            ctx->feed_cur = nxt;
        } else {
            ctx->feed_fill = have;
        }
        HIPCHK(ctx, hipEventSynchronize(ctx->h2d_done));   // the caller's buffers may be reused after return
    }
    return ACG_OK;
}

// pinned host memory for the *_host entry points, so that a C host needs no HIP headers: hipHostMalloc / hipHostRegister
extern "C" void* acg_host_alloc(size_t bytes)
{
    void* p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
extern "C" void acg_host_free(void* p)
{
    if (p) (void)hipHostFree(p);
}
extern "C" int acg_host_register(void* p, size_t bytes)
{
    if (!p || bytes == 0) return ACG_EINVAL;
    return hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess ? ACG_OK : ACG_EHIP;
}
extern "C" int acg_host_unregister(void* p)
{
    if (!p) return ACG_EINVAL;
    return hipHostUnregister(p) == hipSuccess ? ACG_OK : ACG_EHIP;
}

extern "C" int acg_selftest_sincos(const double* x_host, double* sin_host, double* cos_host, int n)
{
    if (!x_host || !sin_host || !cos_host || n < 1) return ACG_EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return ACG_ENODEV;
    double *dx = nullptr, *ds = nullptr, *dc = nullptr, *dt = nullptr;
    const size_t b = (size_t)n * sizeof(double);
    double sct[2 * ACG_SINCOS_N];
    acg_host_sincos_table(sct);
    int rc = ACG_EHIP;
    if (hipMalloc(&dx, b) == hipSuccess && hipMalloc(&ds, b) == hipSuccess && hipMalloc(&dc, b) == hipSuccess &&
        hipMalloc(&dt, sizeof(sct)) == hipSuccess && hipMemcpy(dt, sct, sizeof(sct), hipMemcpyHostToDevice) == hipSuccess &&
        hipMemcpy(dx, x_host, b, hipMemcpyHostToDevice) == hipSuccess &&
        acg_launch_sincos_selftest(dx, ds, dc, n, dt, nullptr) == 0 &&
        hipMemcpy(sin_host, ds, b, hipMemcpyDeviceToHost) == hipSuccess &&
        hipMemcpy(cos_host, dc, b, hipMemcpyDeviceToHost) == hipSuccess)
        rc = ACG_OK;
    hipFree(dx); hipFree(ds); hipFree(dc); hipFree(dt);
    return rc;
}

extern "C" int acg_selftest_div2(const double* n0_host, const double* n1_host, const double* d_host, double* out_host, int n)
{
    if (!n0_host || !n1_host || !d_host || !out_host || n < 1) return ACG_EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return ACG_ENODEV;
    double *a = nullptr, *b = nullptr, *d = nullptr, *o = nullptr;
    const size_t by = (size_t)n * sizeof(double);
    int rc = ACG_EHIP;
    if (hipMalloc(&a, by) == hipSuccess && hipMalloc(&b, by) == hipSuccess && hipMalloc(&d, by) == hipSuccess &&
        hipMalloc(&o, 8 * by) == hipSuccess && hipMemcpy(a, n0_host, by, hipMemcpyHostToDevice) == hipSuccess &&
        hipMemcpy(b, n1_host, by, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d, d_host, by, hipMemcpyHostToDevice) == hipSuccess &&
        acg_launch_div2_selftest(a, b, d, o, n, nullptr) == 0 && hipMemcpy(out_host, o, 8 * by, hipMemcpyDeviceToHost) == hipSuccess)
        rc = ACG_OK;
    hipFree(a); hipFree(b); hipFree(d); hipFree(o);
    return rc;
}

extern "C" int acg_fill_random_u8_dev(uint8_t* dev, size_t pitch_bytes, int nrows, size_t row_bytes,
                                      uint64_t seed, void* hip_stream)
{
    if (!dev || nrows < 1 || (row_bytes & 15) || (pitch_bytes & 15) || ((uintptr_t)dev & 15)) return ACG_EINVAL;
    const int e = acg_launch_fill_random(dev, pitch_bytes, nrows, row_bytes, seed, hip_stream);
    return e == 0 ? ACG_OK : ACG_EHIP;
}

#ifdef ACG_MSK_STAMP
// measurement build only: phase cycle sums of the LAST demodulator launch, [waves][10]
extern "C" int acg_msk_stamp_read(acg_ctx* ctx, unsigned long long* out, int nwaves)
{
    if (!ctx || !out || nwaves < 1 || nwaves > ctx->cfg.nch + 64) return ACG_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipDeviceSynchronize());
    HIPCHK(ctx, hipMemcpy(out, ctx->d_stamp, (size_t)nwaves * 10 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return ACG_OK;
}
extern "C" int acg_msk_lanes_per_channel(const acg_ctx* ctx) { return ctx ? ctx->msk_lpc : 0; }
#endif

extern "C" int acg_probe_read_dev(const void* dev, size_t bytes, int repeats, double* gb_per_s)
{
    if (!dev || bytes < 51200 || ((uintptr_t)dev & 15) || repeats < 1 || !gb_per_s) return ACG_EINVAL;
    unsigned int* sink = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int ncu = 256, devid = 0;
    int rc = ACG_EHIP;
    float ms = 0.f;
    if (hipGetDevice(&devid) == hipSuccess && hipMalloc(&sink, sizeof(unsigned int)) == hipSuccess &&
        hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) {
        (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, devid);
        bool ok = acg_launch_read_probe(dev, bytes, sink, ncu, nullptr) == 0;           // warm-up
        ok = ok && hipEventRecord(e0, nullptr) == hipSuccess;
        for (int i = 0; ok && i < repeats; ++i) ok = acg_launch_read_probe(dev, bytes, sink, ncu, nullptr) == 0;
        ok = ok && hipEventRecord(e1, nullptr) == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
             hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
        if (ok && ms > 0.f) {
            *gb_per_s = (double)(bytes / 51200 * 51200) * repeats / (ms * 1e-3) / 1e9;      // whole 50 KiB runs are read
            rc = ACG_OK;
        }
    }
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    hipFree(sink);
    return rc;
}

// measurement aid: what one host-to-device copy of `bytes` reaches on this box (the ceiling of the *_host entry points)
extern "C" int acg_probe_h2d(void* dev, const void* host, size_t bytes, int repeats, double* gb_per_s)
{
    if (!dev || !host || bytes == 0 || repeats < 1 || !gb_per_s) return ACG_EINVAL;
    if (hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice) != hipSuccess) return ACG_EHIP;      // warm-up
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < repeats; ++i)
        if (hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice) != hipSuccess) return ACG_EHIP;
    if (hipDeviceSynchronize() != hipSuccess) return ACG_EHIP;
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    *gb_per_s = (double)bytes * repeats / sec / 1e9;
    return ACG_OK;
}

extern "C" int acg_synth_iq_u8_dev(uint8_t* iq_dev, size_t pitch_bytes, int nrows, int nout, int decim,
                                   const float* env_dev, size_t env_pitch_floats, const int* env_index_dev,
                                   const float* off_hz_dev, const float* phase_dev, float scale, float noise_sigma,
                                   uint64_t seed, void* hip_stream)
{
    if (!iq_dev || !env_dev || !env_index_dev || !off_hz_dev || !phase_dev || nrows < 1 || nout < 1 || decim < 1 ||
        (decim % 8) || (pitch_bytes & 15) || ((uintptr_t)iq_dev & 15) || pitch_bytes < (size_t)nout * decim * 2)
        return ACG_EINVAL;
    const int e = acg_launch_synth_iq(iq_dev, pitch_bytes, nrows, nout, decim, env_dev, env_pitch_floats, env_index_dev,
                                      off_hz_dev, phase_dev, scale, noise_sigma, seed, hip_stream);
    return e == 0 ? ACG_OK : ACG_EHIP;
}
