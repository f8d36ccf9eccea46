// ctx.cpp -- a context's life: create, reset, destroy, its taps, stream map and channel numbers, the error text, and the small
// queries.  Host runtime only: buffers and their set-up.  There is deliberately no CPU compute path: without a GPU acg_create()
// fails with ACG_ENODEV.
#include "acg_ctx.h"
#include "fir_mm_plan.h"
#include "fir_grid.h"

int fail(acg_ctx* ctx, int code, const char* msg)
{
    if (ctx) ctx->err = msg;
    return code;
}

int hip_fail(acg_ctx* ctx, hipError_t e, const char* call)
{
    ctx->err = std::string(call) + ": " + hipGetErrorString(e);
    return ACG_EHIP;
}

// zero device memory and make sure it has happened before any later launch on any stream
int zero_sync(acg_ctx* c, void* p, size_t bytes)
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

static void free_all(acg_ctx* c)
{
    if (!c) return;
    hipFree(c->d_taps); hipFree(c->d_stream_of); hipFree(c->d_groups); hipFree(c->d_group_ch); hipFree(c->d_gtaps); hipFree(c->d_mm_img); hipFree(c->d_mm1_img); hipFree(c->d_mm_chan); hipFree(c->d_dm_all); hipFree(c->d_st);
    hipFree(c->d_h); hipFree(c->d_sctab); hipFree(c->d_txt); hipFree(c->d_frames); hipFree(c->d_frame_count);
    hipFree(c->d_stamp);
    hipFree(c->d_stats);
    hipFree(c->d_chnum);
    hipFree(c->d_rate_grid); hipFree(c->d_rate_tapsum);
    hipFree(c->d_long_taps); hipFree(c->d_long_hist[0]); hipFree(c->d_long_hist[1]);
    if (c->long_hist_ev) hipEventDestroy(c->long_hist_ev);
    hipFree(c->d_msgs); std::free(c->h_msgs);
    hipFree(c->d_kmsgs); hipFree(c->d_oooi); hipFree(c->d_kwork); std::free(c->h_oooi);
    if (c->flights) acg_fl_destroy(c->flights);
    c->flights = nullptr;
    if (c->reasm) acg_rs_destroy(c->reasm);
    c->reasm = nullptr;
    outputs_destroy(c->json);
    c->json = nullptr;
    outputs_destroy(c->text);
    c->text = nullptr;
    outputs_destroy(c->outs);
    c->outs = nullptr;
    hipFree(c->d_bits); hipFree(c->d_nbits); hipFree(c->d_work); hipFree(c->d_msk_done); std::free(c->h_stage); hipFree(c->d_crctab); hipFree(c->d_rep_upto);
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
    c->stage.destroy();
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
        c->per_call = (unsigned int)per_call;                                         // (results.cpp: how far the newest calls can be ahead of a collect's mark)
        c->lag_max = (int)std::min<unsigned long long>(acg_ctx::NCALL - 2, cap2 / per_call - 1);
    }
    c->exact_fir = (cfg->flags & ACG_F_EXACT_FIR) != 0;
    // MSK kernel shape: the chip has 1024 SIMDs; give every channel as many lanes as keeps the
    // wave count around one per SIMD (latency mode), down to one lane per channel (throughput mode)
    c->msk_lpc = cfg->nch <= 8192 ? 8 : cfg->nch <= 16384 ? 4 : cfg->nch <= 32768 ? 2 : 1;
    // Up to 1024 channels: 16 lanes per channel (msk_lean_wide.hip, round 12).  The 8-lane kernel fills 128 of the chip's SIMDs
    // there and 48 of its partition's 80 CUs carry no demodulator wave; a segment is cut wave-wide, so 4 channels per wave
    // instead of 8 halve the cuts (6.91 -> 7.43 periods per segment on the bench's traffic).  Measured at 1024 channels: the
    // kernel alone 0.944 -> 0.911 ms per call; the headline step, parent commit against this tree, 21.189 21.237 21.252 -> 20.496
    // 20.528 20.529 ms (medians -3.3 %: the worst run of 16 lanes beats the best of 8 by 0.66 ms, ten times the 8-lane arm's
    // max - min); the down-converter keeps its 176 CUs.  32 lanes (512 waves, a partition of 128 CUs) gave the same step
    // (20.53-20.59 against 20.54-20.62 ms) with the down-converter 10-20 % longer: not in the tree.  2048 channels stay at 8
    // lanes: 16 need 128 CUs, and the step went 9.67-10.58 -> 12.48-12.56 ms (the down-converter 1.08-1.20 -> 1.44-1.45 ms per
    // launch, no longer hidden); ACG_MSK_LPC=16 selects them there.  profiles/LEDGER.md, round 12.
#ifndef ACG_MSK_STAMP                              // (the stamp build measures msk.hip's kernel: 8 lanes)
    if (cfg->nch <= 1024) c->msk_lpc = 16;
#endif
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
        const int need = std::max(1, (cfg->nch * 8 / 64 + 3) / 4);          // (n of the 8-lane kernel, whatever width runs)
        c->msk_cus_default = std::min(80, (5 * need + 1) / 2);
    }
    c->msk_high_prio = acg_tune_get("ACG_MSK_PRIO", c->msk_high_prio) ? 1 : 0;
    {
        const int v = acg_tune_get("ACG_MSK_LPC", c->msk_lpc);
        if (v == 1 || v == 2 || v == 4 || v == 8 || v == 16) c->msk_lpc = v;
    }
    // 16 lanes per channel (msk_lean_wide.hip) run in the four-wave workgroups of a context with a CU partition, one wave per
    // SIMD: the partition grows to cover them, up to half the chip (2048 channels: 128 CUs); a context too wide for that keeps
    // 8 lanes.  (Without a partition -- ACG_MSK_CUS=0 -- acg_launch_msk falls back to 8 lanes launch by launch.)
    if (c->msk_lpc > 8) {
#ifdef ACG_MSK_STAMP
        c->msk_lpc = 8;
#else
        const int need = (cfg->nch * c->msk_lpc / 64 + 3) / 4;
        if (cfg->nch <= 2048 && need <= 128) c->msk_cus_default = std::max(c->msk_cus_default, need);
        else c->msk_lpc = 8;
#endif
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
            if (c->msk_lpc > 8 && !c->fir_stream) c->msk_lpc = 8;       // (no partition: one-wave workgroups, which have no wide kernel)
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
        free_all(c);
        delete c;
        return rc;
    }
    *out = c;
    return ACG_OK;
}

// the statistics table as acg_stats_enable and acg_reset leave it: all zero (AcgChanStats: its "none yet" values are zeros)
int stats_zero(acg_ctx* ctx)
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
    ctx->stage.reset();                                  // no reader is left and the carried samples are dropped
    ctx->rate_k = 0;                                     // the grid restarts at window 0
    ctx->long_have = 0;                                  // ... and a channel filter, which stays on, has nothing before it
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
    if (ctx->reasm && acg_rs_reset(ctx->reasm) != ACG_OK) return fail(ctx, ACG_EHIP, "reassembly table reset");
    if (ctx->d_stats) return stats_zero(ctx);
    return ACG_OK;
}

// The u8 / int8 constant of the rate kernel: sum (x - c) t = sum x t - c (1 + j) sum_{i < L} t[i] needs the taps' sum for both
// window lengths, L = decim - 1 and decim.  Made from the table as the device holds it, in double, whenever taps or rate change.
static int rate_tapsums(acg_ctx* ctx)
{
    if (!ctx->d_rate_tapsum) return ACG_OK;
    const size_t nch = (size_t)ctx->cfg.nch, pad = (size_t)ctx->ntaps_pad, n = (size_t)ctx->cfg.decim;
    std::vector<float> t(nch * pad * 2), sums(nch * 4);
    HIPCHK_OL(ctx, hipMemcpy(t.data(), ctx->d_taps, t.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t c = 0; c < nch; ++c) {
        double sr = 0, si = 0;
        for (size_t i = 0; i + 1 < n; ++i) { sr += t[(c * pad + i) * 2]; si += t[(c * pad + i) * 2 + 1]; }
        sums[4 * c] = (float)sr;
        sums[4 * c + 1] = (float)si;
        sums[4 * c + 2] = (float)(sr + t[(c * pad + n - 1) * 2]);
        sums[4 * c + 3] = (float)(si + t[(c * pad + n - 1) * 2 + 1]);
    }
    HIPCHK_OL(ctx, hipMemcpy(ctx->d_rate_tapsum, sums.data(), sums.size() * sizeof(float), hipMemcpyHostToDevice));
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
    return ctx->rate_hz ? rate_tapsums(ctx) : ACG_OK;
}

// ---- any input rate: the window grid of the context (include/acarsdec_amd.h; the kernel: fir_rate.hip) --------------------
const char* const RATE_SET_MSG = "an input rate is set (acg_set_input_rate): this entry point takes whole windows of decim samples, use acg_process_rate_dev / acg_feed_rate_host";

extern "C" int acg_set_input_rate(acg_ctx* ctx, unsigned int rate_hz)
{
    if (!ctx) return ACG_EINVAL;
    if (ctx->stage.fill) return fail(ctx, ACG_ESTATE, "the input rate cannot change while a host feed carries samples (acg_reset drops them)");
    if (rate_hz != 0 && (acg_rate_decim(rate_hz) != ctx->cfg.decim || ctx->cfg.ntaps != ctx->cfg.decim))
        return fail(ctx, ACG_EINVAL, "input rate: the context needs decim == ntaps == acg_rate_decim(rate_hz)");
    HIPCHK_OL(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK_OL(ctx, hipDeviceSynchronize());                 // down-converter launches that read the grid run on the callers' streams
    ctx->rate_k = 0;
    ctx->rate_hz = 0;
    ctx->long_nseg = 0;                                     // a channel filter belongs to the rate it was made for: off
    ctx->long_have = 0;
    if (rate_hz == 0) return ACG_OK;
    unsigned int g = rate_hz, b = ACG_INTRATE;
    while (b) { const unsigned int r = g % b; g = b; b = r; }
    const unsigned int P = rate_hz / g, Q = ACG_INTRATE / g;
    ctx->rate_grid.resize((size_t)Q + 1);
    for (unsigned int r = 0; r <= Q; ++r) ctx->rate_grid[r] = (unsigned int)((unsigned long long)r * P / Q);
    if (!ctx->d_rate_grid) HIPCHK_OL(ctx, hipMalloc(&ctx->d_rate_grid, ((size_t)ACG_INTRATE + 1) * sizeof(unsigned int)));
    if (!ctx->d_rate_tapsum) HIPCHK_OL(ctx, hipMalloc(&ctx->d_rate_tapsum, (size_t)ctx->cfg.nch * 4 * sizeof(float)));
    HIPCHK_OL(ctx, hipMemcpy(ctx->d_rate_grid, ctx->rate_grid.data(), ctx->rate_grid.size() * sizeof(unsigned int), hipMemcpyHostToDevice));
    const int r = rate_tapsums(ctx);
    if (r != ACG_OK) return r;
    ctx->rate_P = P;
    ctx->rate_Q = Q;
    ctx->rate_hz = rate_hz;
    return ACG_OK;
}

// ---- channel filters over several windows (include/acarsdec_amd.h; the kernel: fir_long.hip) -----------------------------
extern "C" int acg_set_channel_filter(acg_ctx* ctx, int nseg, const float* taps)
{
    if (!ctx) return ACG_EINVAL;
    const bool off = nseg == 0 || !taps;
    if (!ctx->rate_hz) return fail(ctx, ACG_ESTATE, "channel filter: no input rate is set (acg_set_input_rate)");
    if (ctx->rate_Q != 1) return fail(ctx, ACG_EINVAL, "channel filter: the input rate must be a multiple of 12 500 Hz");
    if (!off && (nseg < 2 || nseg > ACG_MAXSEG)) return fail(ctx, ACG_EINVAL, "channel filter: nseg outside 2 .. ACG_MAXSEG (0 = off)");
    if (ctx->stage.fill) return fail(ctx, ACG_ESTATE, "the channel filter cannot change while a host feed carries samples (acg_reset drops them)");
    if (!off && !acg_launch_fir_long) return fail(ctx, ACG_ESTATE, "this build has no channel-filter unit");
    HIPCHK_OL(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK_OL(ctx, hipDeviceSynchronize());                 // down-converter launches that read the table run on the callers' streams
    ctx->rate_k = 0;
    ctx->long_have = 0;
    ctx->long_hist_ev_valid = false;
    if (off) {
        ctx->long_nseg = 0;
        return ACG_OK;
    }
    const acg_config& g = ctx->cfg;
    // a channel's table on the device: its nseg * decim taps and 8 zeros (fir_grid.h: what a window's last chunk reads past a segment)
    const size_t tap_bytes = (size_t)nseg * g.decim * 2 * sizeof(float), tap_pitch = tap_bytes + 8 * 2 * sizeof(float);
    if (nseg != ctx->long_nseg || !ctx->d_long_taps) {
        ctx->long_nseg = 0;
        hipFree(ctx->d_long_taps); hipFree(ctx->d_long_hist[0]); hipFree(ctx->d_long_hist[1]);
        ctx->d_long_taps = nullptr;
        ctx->d_long_hist[0] = ctx->d_long_hist[1] = nullptr;
        // the history in the widest format (8 bytes per sample), a chunk of room behind it: every aligned 16-byte read of a
        // row stays inside its pitch
        ctx->long_hist_pitch = (((size_t)(nseg - 1) * g.decim * 8 + 15) & ~(size_t)15) + 16;
        HIPCHK_OL(ctx, hipMalloc(&ctx->d_long_taps, (size_t)g.nch * tap_pitch));
        HIPCHK_OL(ctx, hipMemset(ctx->d_long_taps, 0, (size_t)g.nch * tap_pitch));
        for (auto& h : ctx->d_long_hist) {
            HIPCHK_OL(ctx, hipMalloc(&h, ctx->long_hist_pitch * (size_t)g.nstreams));
            HIPCHK_OL(ctx, hipMemset(h, 0, ctx->long_hist_pitch * (size_t)g.nstreams));
        }
        if (!ctx->long_hist_ev) HIPCHK_OL(ctx, hipEventCreateWithFlags(&ctx->long_hist_ev, hipEventDisableTiming));
    }
    HIPCHK_OL(ctx, hipMemcpy2D(ctx->d_long_taps, tap_pitch, taps, tap_bytes, tap_bytes, (size_t)g.nch, hipMemcpyHostToDevice));
    HIPCHK_OL(ctx, hipDeviceSynchronize());
    ctx->long_nseg = nseg;
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

extern "C" int acg_sync(acg_ctx* ctx)
{
    if (!ctx) return ACG_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->msk_stream));
    if (ctx->post_stream) HIPCHK(ctx, hipStreamSynchronize(ctx->post_stream));
    return ACG_OK;
}

extern "C" int acg_bit_capacity(const acg_ctx* ctx) { return ctx ? ctx->bit_cap : 0; }
extern "C" int acg_max_lag(const acg_ctx* ctx) { return ctx ? ctx->lag_max : 0; }

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
