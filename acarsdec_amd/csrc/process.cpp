// process.cpp -- the whole launch path: every acg_process_* / acg_feed_* entry point, the software pipeline of a call, the
// down-converter's kernel choice and the demodulator launch, the staging ring every *_host entry point copies through and the
// one loop of the carrying feeds, the placement trials and the launch timing.  One unit, so that the compiler inlines in it
// what it likes.
#include <dlfcn.h>
#include <chrono>
#include <mutex>

#include "acg_ctx.h"
#include "fir_mm_plan.h"
#include "fir_grid.h"

namespace {

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

// the dm blocks (and their guards) that len outputs per channel touch
static int blocks_of(const acg_ctx* ctx, int len)
{
    return std::min(ctx->cfg.max_blocks, (len + ACG_BLOCK - 1) / ACG_BLOCK);
}

// Windows per pipeline chunk: the u8 path's bytes per launch, for samples `per` times the u8 sample's size (2-byte samples: its
// callbacks; 4-byte samples: half of them; 8-byte samples: a quarter)
static int chunk_windows(const acg_ctx* ctx, int per)
{
    return (ctx->pipe_blocks > 0 ? (ctx->pipe_blocks + per - 1) / per : ctx->cfg.max_blocks) * ACG_BLOCK;
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

#ifndef ACG_FIR_MM1_DEFAULT
#define ACG_FIR_MM1_DEFAULT 0
#endif

// Which u8 I/Q down-converter kernel takes the launch a (nwin, ncu set by the caller) on this context; fills in the arguments that
// kernel needs.  Changes nothing in the context: launch_fir_u8 launches what this says, acg_lab_fir_launch_shape reports it.
enum FirU8Kernel { FIR_U8_GENERIC, FIR_U8_DIRECT, FIR_U8_SHARED, FIR_U8_MM, FIR_U8_MM1 };
static FirU8Kernel fir_u8_kernel(const acg_ctx* c, FirArgs& a)
{
    const acg_config& g = c->cfg;
    a.nseg = 1;
    // verification mode: rtl.c:335-353 in the reference's own order of operations (fir.hip, fir_u8_generic_kernel)
    // (ACG_FMT_CS8, a.s8: the exact-order kernel restates rtl.c's u8 loop and does not apply; fmt_args has checked decim % 8)
    if (!a.s8 && (c->exact_fir || !c->tile_path)) return FIR_U8_GENERIC;
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
    if (!a.s8 && c->ngroups == 0 && acg_tune_get("ACG_FIR_MM1", ACG_FIR_MM1_DEFAULT) && acg_fir_mm1_image_bytes(g.decim, 1) != 0) {
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
        if (v == 1 || v == 2 || v == 4 || v == 8 || v == 16) lpc = v;          // (16: on the context's CU mask as it is)
    }
    int e;
    {
        RoctxRange range("acg:demodulator");
        // lab build: the two-wave kernel (msk2.hip: the per-bit instruction stream split over a wave pair on two SIMDs);
        // bit-identical to the one-wave kernel, so the switch may change from launch to launch -- and slower
#ifdef ACG_LAB
        // (the two-wave kernel has 8 lanes per channel, also where the one-wave kernel has 16)
        if (lpc >= 8 && acg_tune_get("ACG_MSK_SPLIT", c->msk_split)) e = acg_launch_msk2(&a, c->fir_stream ? 2 : 1, s);
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
    if (ctx->rate_hz) return fail(ctx, ACG_ESTATE, RATE_SET_MSG);
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
        const int j1 = blocks_of(ctx, w0 + nw);
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

// ---- the staging ring (StageRing, acg_ctx.h): how every *_host entry point moves the caller's memory to the device ----
// A round of an entry point: stage_claim, copy into buf[cur] on the copy stream, stage_copied, the device path on the context's
// stream, stage_turn; stage_return before the caller gets its memory back, on the error paths too.  The one invariant all of them
// rest on: the only way to a buffer is stage_claim, which puts the wait for the buffer's last reader -- whichever entry point
// that was -- on the copy stream before any copy into it.  So the copy of a round runs beside the kernels of the round before,
// which read the other buffer.
static const char* const CARRY_MSG = "a host feed is carrying a partial window in the staging buffers (acg_reset drops it)";

// two buffers of at least `bytes` each
static int stage_reserve(acg_ctx* c, size_t bytes)
{
    StageRing& st = c->stage;
    if (!st.copy) {
        HIPCHK(c, hipStreamCreateWithFlags(&st.copy, hipStreamNonBlocking));
        HIPCHK(c, hipEventCreateWithFlags(&st.copied, hipEventDisableTiming));
        for (auto& e : st.free) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    if (st.bytes >= bytes) return ACG_OK;
    if (st.fill) return fail(c, ACG_ESTATE, "staging buffers cannot grow while a partial window is carried");
    HIPCHK(c, hipDeviceSynchronize());                    // nothing may still read the buffers that go away
    for (auto& p : st.buf) { (void)hipFree(p); p = nullptr; }
    st.bytes = 0;
    st.reset();                                           // (nothing is carried: checked above)
    for (auto& p : st.buf) HIPCHK(c, hipMalloc(&p, bytes));
    st.bytes = bytes;
    return ACG_OK;
}

// the copies into buf[cur] are enqueued: the context's stream, where the device path runs, waits for them
static int stage_copied(acg_ctx* c)
{
    HIPCHK(c, hipEventRecord(c->stage.copied, c->stage.copy));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->stage.copied, 0));
    return ACG_OK;
}

// The device path that reads buf[cur] is enqueued: the context's stream is ordered behind its last reader, whichever stream that
// ran on.  The other buffer becomes the current one.  (The wait for ITS last reader is stage_claim's: put on the copy stream
// here, while the kernels of the round before may still run, it cost bench.py's hostfed case 1.2 % of its input rate.)
static int stage_turn(acg_ctx* c)
{
    StageRing& st = c->stage;
    HIPCHK(c, hipEventRecord(st.free[st.cur], c->stream));
    st.free_valid[st.cur] = true;
    st.cur ^= 1;
    return ACG_OK;
}

// The current buffer, for copies into it: the copy stream waits for the buffer's last reader first (once: the stream runs in order).
static int stage_claim(acg_ctx* c, unsigned char*& buf)
{
    StageRing& st = c->stage;
    if (st.free_valid[st.cur]) HIPCHK(c, hipStreamWaitEvent(st.copy, st.free[st.cur], 0));
    st.free_valid[st.cur] = false;
    buf = (unsigned char*)st.buf[st.cur];
    return ACG_OK;
}

// The caller's memory is free again: the newest copy has left it, and the copy stream runs in order.  rc is what the entry
// point has to say so far: after an error too a copy may still be reading the caller's buffer, and must not after we return.
static int stage_return(acg_ctx* c, int rc)
{
    const hipError_t e = hipEventSynchronize(c->stage.copied);
    return rc != ACG_OK || e == hipSuccess ? rc : hip_fail(c, e, "hipEventSynchronize(stage.copied)");
}

// Host input: the call returns when the copy has left the caller's memory (rtl.c:314-330: the buffer belongs to the driver
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
    if (ctx->stage.fill) return fail(ctx, ACG_ESTATE, CARRY_MSG);          // (it waits at the head of the same buffers)
    if ((r = stage_reserve(ctx, max_row * ctx->cfg.nstreams)) != ACG_OK) return r;
    unsigned char* dev;
    if ((r = stage_claim(ctx, dev)) != ACG_OK) return r;
    HIPCHK(ctx, hipMemcpy2DAsync(dev, dpitch, iq_host, ctx->cfg.nstreams > 1 ? pitch_bytes : row, row, (size_t)ctx->cfg.nstreams,
                                 hipMemcpyHostToDevice, ctx->stage.copy));
    if ((r = stage_copied(ctx)) == ACG_OK) r = acg_process_iq_u8_dev(ctx, dev, dpitch, nblocks, nullptr);
    if (r == ACG_OK) r = stage_turn(ctx);
    return stage_return(ctx, r);
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
    if (len > 0 && (r = guard_record(ctx, 0, blocks_of(ctx, len))) != ACG_OK) return r;
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
        if ((r = guard_wait(ctx, s, 0, blocks_of(ctx, nframes))) != ACG_OK) return r;
        if ((r = launch_pcm(ctx, fmt, frames_dev, nframes, ctx->d_dm, ctx->dm_pitch, s)) != ACG_OK) return r;
        HIPCHK(ctx, hipEventRecord(ctx->in_ev, s));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->msk_stream, ctx->in_ev, 0));
    }
    if ((r = launch_msk(ctx, ctx->d_dm, ctx->dm_pitch, nframes, ctx->msk_stream)) != ACG_OK) return r;
    if (nframes > 0 && (r = guard_record(ctx, 0, blocks_of(ctx, nframes))) != ACG_OK) return r;
    return end_of_call(ctx);
}

// Host frames of any count: chunks of at most max_len frames, each ONE contiguous copy and one round of the staging ring (the
// copy of chunk k + 1 runs beside the kernels of chunk k), then the device path.  Returns when the last copy has left the
// caller's buffer.
extern "C" int acg_feed_pcm_host(acg_ctx* ctx, int fmt, const void* frames, size_t nframes)
{
    int r = check_pcm_args(ctx, fmt, frames);
    if (r != ACG_OK) return r;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    if (ctx->stage.fill) return fail(ctx, ACG_ESTATE, CARRY_MSG);
    if (nframes == 0) return acg_process_pcm_dev(ctx, fmt, frames, 0, nullptr);
    const size_t fb = (size_t)ctx->cfg.nch * pcm_elem(fmt);          // bytes per frame
    if ((r = stage_reserve(ctx, ((size_t)ctx->max_len * fb + 3) & ~(size_t)3)) != ACG_OK) return r;
    for (size_t done = 0; done < nframes && r == ACG_OK;) {
        const size_t take = std::min(nframes - done, (size_t)ctx->max_len);
        unsigned char* dev;
        if ((r = stage_claim(ctx, dev)) != ACG_OK) break;
        HIPCHK(ctx, hipMemcpyAsync(dev, (const unsigned char*)frames + done * fb, take * fb, hipMemcpyHostToDevice, ctx->stage.copy));
        // (the de-interleave kernel is the buffer's only reader)
        if ((r = stage_copied(ctx)) == ACG_OK) r = acg_process_pcm_dev(ctx, fmt, dev, (int)take, nullptr);
        if (r == ACG_OK) r = stage_turn(ctx);
        done += take;
    }
    return stage_return(ctx, r);
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

// ------------------------------------------------------------------------------------------
// The other front ends' sample formats: soapy.c (CS16), sdrplay.c (split int16),
// air.c (real f32), and the recordings' (SigMF ci8, cf32_le).  Same tile kernel; bytes per sample and plane by format.
static size_t fmt_sample_bytes(int fmt)
{
    return fmt == ACG_FMT_CS8 || fmt == ACG_FMT_S16_SPLIT ? 2 : fmt == ACG_FMT_CF32 ? 8 : 4;
}

// The limits of a sample format on a context of window length decim with ntaps_pad padded taps: NULL, or the rule broken.
// Host arithmetic only (acg_lab_samples_launch_shape reports the same answer without launching).
static const char* fmt_limits(int fmt, int decim, int ntaps_pad)
{
    if (fmt < ACG_FMT_CS16 || fmt > ACG_FMT_CF32) return "unknown sample format";
    if (fmt == ACG_FMT_CS8)
        return decim % 8 ? "int8 I/Q samples need decim % 8 == 0 (a 16-byte chunk is 8 samples)"
               : decim > ACG_MAXDECIM ? "int8 I/Q samples: decim above ACG_MAXDECIM (the u8 kernels' window limit)" : nullptr;
    if (fmt == ACG_FMT_CF32)
        return decim % 2 ? "complex float32 samples need decim % 2 == 0 (a 16-byte chunk is 2 samples)"
               : decim > ACG_MAXDECIM_SAMPLES ? "complex float32 samples: decim above ACG_MAXDECIM_SAMPLES"
               : ntaps_pad % 2 ? "complex float32 samples need ntaps % 2 == 0 when decim % 8 != 0" : nullptr;
    if (decim % (fmt == ACG_FMT_S16_SPLIT ? 8 : 4) || (fmt == ACG_FMT_S16_SPLIT && decim > 208))
        return "this sample format needs decim % 4 == 0 (split planes: % 8 and <= 208)";
    if (ntaps_pad % (fmt == ACG_FMT_S16_SPLIT ? 8 : 4)) return "this sample format needs ntaps % 4 == 0 when decim % 8 != 0";
    return nullptr;
}

static int fmt_args(acg_ctx* ctx, int fmt, FirArgs* a)
{
    const acg_config& g = ctx->cfg;
    if (const char* broken = fmt_limits(fmt, g.decim, ctx->ntaps_pad)) return fail(ctx, ACG_EINVAL, broken);
    if (fmt == ACG_FMT_CS8) {                           // the u8 window and the u8 kernel choice, signed (iq, pitch: the caller)
        *a = u8_args(ctx, nullptr, 0);
        a->s8 = 1;
        return ACG_OK;
    }
    *a = fir_args(ctx);
    a->row_bytes = (fmt == ACG_FMT_S16_SPLIT ? 2 : 1) * (int)fmt_sample_bytes(fmt) * g.decim;      // a window's bytes, both planes
    a->cpr_total = a->row_bytes / 16;
    a->kseg = (a->cpr_total + 51) / 52;                 // LDS slice <= 52 chunks per window (Airspy: 480 -> 3 x 40, 800 -> 4 x 50)
    a->cpr = (a->cpr_total + a->kseg - 1) / a->kseg;
    a->row_stride = 16 * ((a->cpr & 1) ? a->cpr : a->cpr + 1);
    a->cpr_magic = ((1u << 20) + (unsigned int)a->cpr - 1) / (unsigned int)a->cpr;
    a->nseg = 1;
    a->out_scale = fmt == ACG_FMT_CS16 ? 1.0f / 32768.0f : fmt == ACG_FMT_S16_SPLIT ? 0.25f : 1.0f;
    return ACG_OK;
}

// pipeline chunk of the formats (chunk_windows; split planes: two 2-byte samples)
static int fmt_chunk_win(const acg_ctx* ctx, int fmt)
{
    return chunk_windows(ctx, fmt == ACG_FMT_CS8 ? 1 : fmt == ACG_FMT_CF32 ? 4 : 2);
}

// the format's down-converter launch (see fir_launch)
static auto fmt_launch(int fmt)
{
    return [fmt](acg_ctx* c, FirArgs& f, hipStream_t s) { return fmt == ACG_FMT_CS8 ? launch_fir_u8(c, f, s) : acg_launch_fir_fmt(&f, fmt, s); };
}

extern "C" int acg_process_samples_dev(acg_ctx* ctx, int fmt, const void* dev, size_t pitch_bytes, size_t plane_bytes,
                                       int nblocks, void* hip_stream)
{
    if (!ctx || !dev) return ACG_EINVAL;
    if (ctx->rate_hz) return fail(ctx, ACG_ESTATE, RATE_SET_MSG);
    if (nblocks < 1 || nblocks > ctx->cfg.max_blocks) return fail(ctx, ACG_EINVAL, "nblocks out of range");
    if ((((uintptr_t)dev | pitch_bytes | plane_bytes) & 15)) return fail(ctx, ACG_EINVAL, "base, pitch and plane must be 16-byte aligned");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    FirArgs a;
    int r = fmt_args(ctx, fmt, &a);
    if (r != ACG_OK) return r;
    a.iq = (const uint8_t*)dev;
    a.pitch = pitch_bytes;
    a.plane = plane_bytes;
    const size_t win_bytes = (size_t)ctx->cfg.decim * fmt_sample_bytes(fmt);                   // of one plane
    return run_pipeline(ctx, hip_stream ? (hipStream_t)hip_stream : ctx->stream, a, win_bytes, nblocks * ACG_BLOCK, fmt_chunk_win(ctx, fmt),
                        fmt_launch(fmt));
}

// Host feed with carry: windows may straddle feeds of any size (soapy.c:232-254, sdrplay.c:215-236,
// air.c:299-338 carry D / the index across buffers; here the incomplete window's SAMPLES wait at the
// head of a device staging row -- the sums are then the same sequential windows).
// The one loop of acg_feed_samples_host and acg_feed_rate_host, a round of the staging ring each time: up to a staging row of
// samples (bps bytes each in the plane p0, and in p1 where the format has two) goes behind the carried ones; fit(have) says how
// many whole windows that makes and how many samples they use; run(base, pitch, plane, have, nwin) is their device path; the
// rest moves to the head of the buffer that is the current one from then on -- on the copy stream, beside the kernels.
struct FeedFit { int nwin; size_t used; };
template <class Fit, class Run>
static int feed_carry(acg_ctx* ctx, int fmt, size_t bps, const void* p0, const void* p1, size_t pitch_samples, size_t nsamples, Fit&& fit,
                      Run&& run)
{
    StageRing& st = ctx->stage;
    if (st.fmt != fmt) { st.fmt = fmt; st.fill = 0; }
    const size_t ns = (size_t)ctx->cfg.nstreams;
    const size_t cap = (size_t)ctx->max_len * (size_t)ctx->cfg.decim;         // samples a staging row holds: max_len windows always fit
    const size_t plane = ((cap * bps) + 15) & ~(size_t)15;
    const size_t rowb = p1 ? 2 * plane : plane, hpitch = (ns > 1 ? pitch_samples : nsamples) * bps;
    const void* const host[2] = {p0, p1};
    int r = stage_reserve(ctx, rowb * ns);
    if (r != ACG_OK) return r;
    // (no samples left: a round for whole windows that a launch capped at max_len left behind)
    for (size_t done = 0; done < nsamples || fit(st.fill).nwin > 0;) {
        const size_t take = std::min(nsamples - done, cap - st.fill), have = st.fill + take;
        unsigned char *base = nullptr, *next = nullptr;
        if ((r = stage_claim(ctx, base)) != ACG_OK) break;
        for (int k = 0; k < 2 && host[k] && take; ++k)
            HIPCHK_OL(ctx, hipMemcpy2DAsync(base + k * plane + st.fill * bps, rowb, (const unsigned char*)host[k] + done * bps, hpitch,
                                            take * bps, ns, hipMemcpyHostToDevice, st.copy));
        done += take;
        if ((r = stage_copied(ctx)) != ACG_OK) break;                      // (also where no window gets whole: stage_return waits for this)
        const FeedFit f = fit(have);
        if (f.nwin == 0) {
            st.fill = have;
            break;                                                          // (have < cap here: the input is used up)
        }
        if ((r = run(base, rowb, plane, have, f.nwin)) != ACG_OK || (r = stage_turn(ctx)) != ACG_OK) break;
        const size_t left = have - f.used;
        if (left && (r = stage_claim(ctx, next)) != ACG_OK) break;
        for (int k = 0; k < 2 && host[k] && left; ++k)
            HIPCHK_OL(ctx, hipMemcpy2DAsync(next + k * plane, rowb, base + k * plane + f.used * bps, rowb, left * bps,
                                            ns, hipMemcpyDeviceToDevice, st.copy));
        st.fill = left;
    }
    return stage_return(ctx, r);
}

extern "C" int acg_feed_samples_host(acg_ctx* ctx, int fmt, const void* p0, const void* p1, size_t pitch_samples,
                                     size_t nsamples)
{
    if (!ctx || !p0 || (fmt == ACG_FMT_S16_SPLIT && !p1)) return ACG_EINVAL;
    if (ctx->rate_hz) return fail(ctx, ACG_ESTATE, RATE_SET_MSG);
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    FirArgs a;
    int r = fmt_args(ctx, fmt, &a);
    if (r != ACG_OK) return r;
    const size_t M = (size_t)ctx->cfg.decim, bps = fmt_sample_bytes(fmt);      // bytes per sample per plane
    return feed_carry(ctx, fmt, bps, p0, fmt == ACG_FMT_S16_SPLIT ? p1 : nullptr, pitch_samples, nsamples,
                      [&](size_t have) { return FeedFit{(int)(have / M), have / M * M}; },
                      [&](const unsigned char* base, size_t pitch, size_t plane, size_t, int nwin) {
                          a.iq = base;
                          a.pitch = pitch;
                          a.plane = plane;
                          return run_pipeline(ctx, ctx->stream, a, M * bps, nwin, fmt_chunk_win(ctx, fmt), fmt_launch(fmt));
                      });
}

// ------------------------------------------------------------------------------------------
// Any input rate (acg_set_input_rate): windows on the grid s_k = floor(k P / Q).  The kernel is fir_rate.hip's; the CU partition
// and the FIR/demodulator stream pipeline are run_pipeline's, with no bytes per window: a chunk's launch finds its windows from
// the chunk's first window, which is where its dm begins.
static int rate_fmt(acg_ctx* ctx, int fmt, FirRateArgs* r)
{
    if (!ctx->rate_hz) return fail(ctx, ACG_ESTATE, "no input rate is set (acg_set_input_rate)");
    if (!acg_launch_fir_rate) return fail(ctx, ACG_ESTATE, "this build has no rate down-converter unit");
    if (ctx->long_nseg && !acg_launch_fir_long) return fail(ctx, ACG_ESTATE, "this build has no channel-filter unit");
    switch (fmt) {
    case ACG_FMT_CU8: r->fmt = RATE_CU8; break;
    case ACG_FMT_CS8: r->fmt = RATE_CS8; break;
    case ACG_FMT_CS16: r->fmt = RATE_CS16; break;
    case ACG_FMT_CF32: r->fmt = RATE_CF32; break;
    case ACG_FMT_S16_SPLIT:
    case ACG_FMT_F32_REAL:
        return fail(ctx, ACG_EINVAL, "split planes and real float32 belong to front ends that fix their own rates: the rate entry points take "
                                     "ACG_FMT_CU8, ACG_FMT_CS8, ACG_FMT_CS16 and ACG_FMT_CF32");
    default: return fail(ctx, ACG_EINVAL, "unknown sample format");
    }
    const acg_config& g = ctx->cfg;
    r->stream_of = ctx->d_stream_of;
    r->taps = ctx->d_taps;
    r->tapsum = ctx->d_rate_tapsum;
    r->grid = ctx->d_rate_grid;
    r->dm_pitch = ctx->dm_pitch;
    r->P = ctx->rate_P;
    r->Q = ctx->rate_Q;
    r->r0 = (unsigned int)(ctx->rate_k % ctx->rate_Q);
    r->nch = g.nch;
    r->decim = g.decim;
    const float scale = ACG_FIR_GRID_FMT[r->fmt].scale;
    r->scale_long = (float)((double)scale / g.decim);
    r->scale_short = (float)((double)scale / (g.decim - 1));
    acg_fir_rate_plan(r);
    return ACG_OK;
}

// s_(k0 + n) - s_k0 on the context's grid
static unsigned long long rate_span(const acg_ctx* ctx, unsigned long long n)
{
    const unsigned long long r0 = ctx->rate_k % ctx->rate_Q, i = r0 + n;
    return i / ctx->rate_Q * ctx->rate_P + ctx->rate_grid[(size_t)(i % ctx->rate_Q)] - ctx->rate_grid[(size_t)r0];
}

// the whole windows that fit into nsamples from the context's current window start, at most max_len
static int rate_windows_fit(const acg_ctx* ctx, size_t nsamples)
{
    unsigned long long n = (unsigned long long)((unsigned __int128)nsamples * ctx->rate_Q / ctx->rate_P);     // within one of the answer
    n = std::min<unsigned long long>(n, (unsigned long long)ctx->max_len);
    while (n < (unsigned long long)ctx->max_len && rate_span(ctx, n + 1) <= nsamples) ++n;
    while (n > 0 && rate_span(ctx, n) > nsamples) --n;
    return (int)n;
}

// nwin windows of the rows at dev (nsamples presented each) through the pipeline; advances the grid
static int rate_run(acg_ctx* ctx, FirRateArgs& r, const void* dev, size_t pitch, size_t nsamples, int nwin, hipStream_t s)
{
    r.in = (const uint8_t*)dev;
    r.pitch = pitch;
    r.valid_bytes = ((unsigned long long)nsamples * r.bps + 15) & ~15ull;
    FirArgs a = fir_args(ctx);
    a.iq = r.in;
    a.pitch = pitch;
    FirLongArgs l{};
    if (ctx->long_nseg) {
        // A channel filter (acg_set_channel_filter): the rows and the chunks are the same, the kernel is fir_long.hip's, and the
        // nseg - 1 windows before the call's first sample come from the context's history -- written behind the last launch of
        // the call before, on that call's stream: this call's launches wait for it, whatever their stream.
        if (ctx->long_fmt != r.fmt) { ctx->long_fmt = r.fmt; ctx->long_have = 0; }
        if (ctx->long_hist_ev_valid) HIPCHK_OL(ctx, hipStreamWaitEvent(s, ctx->long_hist_ev, 0));
        static_cast<FirGridArgs&>(l) = r;                        // the same rows, channels and windows
        l.hist = ctx->d_long_hist[ctx->long_hist_cur];
        l.hist_pitch = ctx->long_hist_pitch;
        l.taps = ctx->d_long_taps;
        l.tap_pitch = ((size_t)ctx->long_nseg * r.decim + 8) * 2;
        l.nseg = ctx->long_nseg;
        l.nprev = ctx->long_have;
        l.scale = ACG_FIR_GRID_FMT[r.fmt].scale;
        acg_fir_long_plan(&l);
    }
    // one chunk's launch (see fir_launch): the call's arguments with the chunk's windows
    const int rc = run_pipeline(ctx, s, a, 0, nwin, chunk_windows(ctx, r.bps / 2), [&](acg_ctx* c, FirArgs& f, hipStream_t st) {
        FirGridArgs& b = c->long_nseg ? static_cast<FirGridArgs&>(l) : r;
        b.dm = f.dm;
        b.win0 = (int)(f.dm - c->d_dm);                              // the chunk's first window
        b.nwin = f.nwin;
        b.ncu = f.ncu;
        return c->long_nseg ? acg_launch_fir_long(&l, st) : acg_launch_fir_rate(&r, st);
    });
    if (rc == ACG_OK) ctx->rate_k += (unsigned long long)nwin;
    if (rc == ACG_OK && ctx->long_nseg) {
        // The history of the next call: the last nseg - 1 windows of (this call's history, this call's windows), into the other
        // buffer (the launches just issued read this one), on the caller's stream, which run_pipeline has ordered behind the
        // call's last down-converter launch.  A call of fewer windows than that shifts what there was.
        const int keep = ctx->long_nseg - 1, nxt = ctx->long_hist_cur ^ 1;
        const size_t wb = (size_t)r.decim * r.bps, ns = (size_t)ctx->cfg.nstreams;
        unsigned char* dst = ctx->d_long_hist[nxt];
        if (nwin >= keep) {
            HIPCHK_OL(ctx, hipMemcpy2DAsync(dst, l.hist_pitch, r.in + (size_t)(nwin - keep) * wb, pitch, keep * wb, ns, hipMemcpyDeviceToDevice, s));
        } else {
            HIPCHK_OL(ctx, hipMemcpy2DAsync(dst, l.hist_pitch, l.hist + (size_t)nwin * wb, l.hist_pitch, (keep - nwin) * wb, ns, hipMemcpyDeviceToDevice, s));
            HIPCHK_OL(ctx, hipMemcpy2DAsync(dst + (keep - nwin) * wb, l.hist_pitch, r.in, pitch, nwin * wb, ns, hipMemcpyDeviceToDevice, s));
        }
        HIPCHK_OL(ctx, hipEventRecord(ctx->long_hist_ev, s));
        ctx->long_hist_ev_valid = true;
        ctx->long_hist_cur = nxt;
        ctx->long_have = std::min(keep, ctx->long_have + nwin);
    }
    return rc;
}

extern "C" int acg_process_rate_dev(acg_ctx* ctx, int fmt, const void* dev, size_t pitch_bytes, size_t nsamples, void* hip_stream,
                                    int* nwin, size_t* consumed)
{
    if (!ctx || !dev || !nwin || !consumed) return ACG_EINVAL;
    *nwin = 0;
    *consumed = 0;
    FirRateArgs r{};
    int rc = rate_fmt(ctx, fmt, &r);
    if (rc != ACG_OK) return rc;
    if ((((uintptr_t)dev | pitch_bytes) & 15)) return fail(ctx, ACG_EINVAL, "base and pitch must be 16-byte aligned");
    if (pitch_bytes < (((unsigned long long)nsamples * r.bps + 15) & ~15ull))
        return fail(ctx, ACG_EINVAL, "pitch smaller than a row: nsamples * bytes per sample, rounded up to 16");
    if (ctx->stage.fill) return fail(ctx, ACG_ESTATE, CARRY_MSG);
    HIPCHK_OL(ctx, hipSetDevice(ctx->cfg.device));
    const int n = rate_windows_fit(ctx, nsamples);
    if (n == 0) return ACG_OK;
    const unsigned long long span = rate_span(ctx, (unsigned long long)n);
    rc = rate_run(ctx, r, dev, pitch_bytes, nsamples, n, hip_stream ? (hipStream_t)hip_stream : ctx->stream);
    if (rc != ACG_OK) return rc;
    *nwin = n;
    *consumed = (size_t)span;
    return ACG_OK;
}

// acg_feed_samples_host's scheme with variable windows: the samples behind the last whole window wait at the head of the other
// staging row -- always a window start.
extern "C" int acg_feed_rate_host(acg_ctx* ctx, int fmt, const void* samples, size_t pitch_samples, size_t nsamples)
{
    if (!ctx || !samples) return ACG_EINVAL;
    FirRateArgs r{};
    int rc = rate_fmt(ctx, fmt, &r);
    if (rc != ACG_OK) return rc;
    HIPCHK_OL(ctx, hipSetDevice(ctx->cfg.device));
    return feed_carry(ctx, fmt, (size_t)r.bps, samples, nullptr, pitch_samples, nsamples,
                      [&](size_t have) {
                          const int n = rate_windows_fit(ctx, have);
                          return FeedFit{n, (size_t)rate_span(ctx, (unsigned long long)n)};
                      },
                      [&](const unsigned char* base, size_t pitch, size_t, size_t have, int nwin) {
                          r.r0 = (unsigned int)(ctx->rate_k % ctx->rate_Q);
                          return rate_run(ctx, r, base, pitch, have, nwin, ctx->stream);
                      });
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

// ---- lab: the kernel family one launch of `nblocks` callbacks of sample format fmt takes on this context -----------------------
extern "C" int acg_lab_samples_launch_shape(acg_ctx* ctx, int fmt, int nblocks, acg_lab_samples_launch* out)
{
    if (!ctx || !out) return ACG_EINVAL;
    if (nblocks < 1 || nblocks > ctx->cfg.max_blocks) return fail(ctx, ACG_EINVAL, "nblocks out of range");
    if (!acg_fir_choice) return fail(ctx, ACG_ESTATE, "this build has no down-converter unit");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    std::memset(out, 0, sizeof *out);
    FirArgs a;
    int r = fmt_args(ctx, fmt, &a);
    if (r != ACG_OK) return r;
    a.nwin = nblocks * ACG_BLOCK;
    if (ctx->fir_stream) a.ncu = ctx->fir_ncu;
    out->chunk_blocks = fmt_chunk_win(ctx, fmt) / ACG_BLOCK;
    if (fmt == ACG_FMT_CS8) {
        const FirU8Kernel k = fir_u8_kernel(ctx, a);
        if (k == FIR_U8_MM || k == FIR_U8_SHARED) {
            out->family = k == FIR_U8_MM ? ACG_LAB_FIR_MATRIX : ACG_LAB_FIR_SHARED_VECTOR;
            if (k == FIR_U8_MM) {
                int cus = 0;
                (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->cfg.device);
                const MmPlan p = acg_fir_mm_plan(&a, cus);
                out->tile_windows = 32;
                out->stages = p.stages;
                out->runs = p.runs;
                out->waves = p.waves;
            }
            return ACG_OK;
        }
    }
    FirChoice ch;
    if (int e = acg_fir_choice(&a, fmt, &ch)) {
        ctx->err = std::string("acg_lab_samples_launch_shape: ") + hipGetErrorString((hipError_t)e);
        return ACG_EHIP;
    }
    out->family = ch.family;
    out->tile_windows = ch.tile_win;
    out->runs = (unsigned int)ch.runs;
    out->waves = (unsigned int)ch.waves;
    out->waves_per_workgroup = ch.wpg;
    out->bodies_per_run = ch.pairs;
    return ACG_OK;
}
