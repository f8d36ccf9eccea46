// results.cpp -- the host's side of the block ring: collect and drain of frames and messages, the staging behind them, the
// message filter, the flight table's entry points and the per-channel statistics.
#include "acg_ctx.h"

// ------------------------------------------------------------------------------------------
// The host's side of the block ring.  A collect hands out blocks up to the mark of the call `lag` calls behind the newest
// (the queue length when that call ended), a drain (lag = DRAIN) up to the device's count once everything has finished:
// the oldest min(pending, max) records of [consumed, upto), ordered by (chn, end_bit) within the call.  What does not fit
// STAYS queued (ACG_EAGAIN: call again, nothing lost); only a ring that the device has lapped loses blocks (ACG_EOVERFLOW,
// the count is in acg_last_error).
//
// The rule (include/acarsdec_amd.h, ACG_EOVERFLOW; tests/ring_model.py restates it, tests/test_gpu_ring_laps.py holds every entry
// point to it).  With live = the device's count once every ISSUED call has finished:
//     lost    = max(0, live - cap - consumed), consumed += lost       -- ACG_EOVERFLOW iff lost > 0
//     pending = max(0, upto - consumed)                               -- a collect's mark may lie behind the consumer
//     take    = min(pending, max), the blocks [consumed, consumed + take) go out, consumed += take
// The loss is judged against `live`, not against a collect's own mark: the calls newer than that mark write into the ring whether
// the host has waited for them or not, and what they overwrote is gone for this collect as well.

// Where this collect / drain ends (RingSpan, acg_ctx.h), and the device's live count where only that can tell what was overwritten
int ring_upto(acg_ctx* ctx, int lag, RingSpan* span)
{
    *span = RingSpan{};
    if (lag != DRAIN && lag > ctx->lag_max) return fail(ctx, ACG_EINVAL, "lag above acg_max_lag(): the block queue of this context holds fewer calls");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    if (lag == DRAIN) {
        HIPCHK(ctx, hipDeviceSynchronize());
        HIPCHK(ctx, hipMemcpy(&span->upto, ctx->d_frame_count, sizeof(span->upto), hipMemcpyDeviceToHost));
        span->live = span->upto;
        span->any = true;
        return ACG_OK;
    }
    if (ctx->call_seq <= (unsigned long long)lag) return ACG_OK;              // nothing old enough yet
    const unsigned long long call = ctx->call_seq - 1 - (unsigned long long)lag;
    const int slot = (int)(call % acg_ctx::NCALL);
    HIPCHK(ctx, hipEventSynchronize(ctx->call_done[slot]));                   // only that call, not newer ones
    span->upto = span->live = ctx->h_call_count[slot];
    // (a drain may already have handed out more than that call had queued: its mark then lies BEHIND the consumer -- nothing
    //  is pending; the counters are monotonic and wrap, so the comparison is a signed difference)
    const long long behind = (int)(span->upto - ctx->consumed);
    // The `lag` newer calls have queued at most per_call blocks each behind that mark: live <= upto + lag * per_call.  While that
    // bound stays inside the ring they cannot have reached the consumer, whether they have run yet or not, and nothing more is
    // waited for or read (`upto` stands for the live count).  A host that collects after every call is always here: the ring
    // holds (lag_max + 1) * per_call.
    if (behind + (long long)lag * (long long)ctx->per_call <= (long long)ctx->frame_cap) {
        span->any = behind > 0;
        return ACG_OK;
    }
    // A host that fell behind (it skipped collects, or left a remainder through a small buffer): the newest calls may have
    // overwritten what it has not consumed.  Only the device's count tells, once everything issued has finished -- the same
    // outcome whether the newest call had run yet or not; the loss is ring_claim's to account.
    // (one error text for both steps: the product library has no room for HIPCHK's two, tests/test_host_logic.py's size rule)
    if (hipEventSynchronize(ctx->call_done[(int)((ctx->call_seq - 1) % acg_ctx::NCALL)]) != hipSuccess ||
        hipMemcpy(&span->live, ctx->d_frame_count, sizeof(span->live), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(ctx, ACG_EHIP, "block queue: the live count could not be read");
    span->any = true;
    return ACG_OK;
}

// Accounts what the device has overwritten (ACG_EOVERFLOW), then claims the oldest min(pending, max) blocks of [consumed, upto)
int ring_claim(acg_ctx* ctx, const RingSpan& span, int max, unsigned int* pending, unsigned int* take)
{
    int rc = ACG_OK;
    unsigned int queued = span.live - ctx->consumed;              // monotonic counters, wrap-safe
    if (queued > ctx->frame_cap) {                                // the device lapped the host: oldest lost
        const unsigned int lost = queued - ctx->frame_cap;
        char msg[96];
        std::snprintf(msg, sizeof(msg), "block queue lapped: the %u oldest blocks are lost", lost);
        ctx->err = msg;
        if (ctx->d_stats) ctx->lost_blocks += lost;               // (they belong to no channel: their records are gone)
        ctx->consumed += lost;
        queued = ctx->frame_cap;
        rc = ACG_EOVERFLOW;
    }
    *pending = span.upto - ctx->consumed;
    if (*pending > queued) *pending = 0;                          // a collect's mark behind the consumer (the loss moved it there)
    *take = std::min(*pending, (unsigned int)std::max(0, max));
    return rc;
}

// ... and what the call returns once the claimed records are out: the lap (its text is already in ctx->err), or `again`
// when some stayed queued
int ring_result(acg_ctx* ctx, int rc, unsigned int pending, unsigned int take, const char* again)
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
    unsigned int pending = 0, take = 0;
    RingSpan span;
    int rc = ring_upto(ctx, lag, &span);
    if (rc != ACG_OK || !span.any) return rc;
    rc = ring_claim(ctx, span, max_frames, &pending, &take);
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
// the message entry points' staging (fetch_msgs, outputs_fetch), grown on demand: the split's records, device and host ...
int grow_msg_stage(acg_ctx* ctx, unsigned int take)
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
int grow_label_stage(acg_ctx* ctx, unsigned int take)
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
int commit_imports(acg_ctx* ctx)
{
    if (!ctx->flights || !acg_fl_imports_queued(ctx->flights)) return ACG_OK;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    const int rc = acg_fl_commit(ctx->flights, ctx->copy_stream);
    return rc == ACG_OK ? rc : fail(ctx, rc, "flight table: the pass over the imported events failed");
}

// The split of the `take` oldest blocks into d_msgs on the copy stream (it writes every byte of a record, text tail zeroed, so
// nothing stale crosses the ABI); with `labels`, label.hip's pass behind it into d_kmsgs / d_oooi (the caller has grown the label
// stage) and, the flight table on, its pass; the reassembly table on, its pass over the split's records behind them.  *d_total: the
// label pass's count of kept records, a device word.
int launch_split(acg_ctx* ctx, unsigned int take, bool labels, unsigned int** d_total)
{
    *d_total = ctx->d_kwork + ctx->kmsgs_cap / 256 + 1;
    AcgLabelPass pass{&ctx->msg_filter, ctx->d_kwork, ctx->d_kmsgs, ctx->d_oooi, *d_total, nullptr, nullptr};
    const AcgReasmPass* rp = nullptr;
    if (ctx->reasm) {                                             // the same blocks through the reassembly table, behind the label pass
        const int rr = acg_rs_prepare(ctx->reasm, take, ctx->copy_stream, ctx->d_chnum, (unsigned int)ctx->cfg.nch, &rp);
        if (rr != ACG_OK) return fail(ctx, rr, "reassembly table: work space");
        pass.keep_out = rp->keep;                                 // (which records the label pass kept: the statuses' way to them)
    }
    if (ctx->flights) {                                           // over exactly the blocks this call consumes, before -e drops any
        const int fr = acg_fl_prepare(ctx->flights, take, ctx->copy_stream, &pass.flights);
        if (fr != ACG_OK) return fail(ctx, fr, "flight table: work space");
    }
    if (acg_launch_msg_split(ctx->d_frames, ctx->frame_cap, ctx->consumed, take, ctx->d_msgs, ctx->copy_stream, labels ? &pass : nullptr) != 0)
        return fail(ctx, ACG_EHIP, "message split launch failed");
    if (rp && acg_rs_launch(ctx->reasm, ctx->d_msgs, take, &ctx->msg_filter, ctx->copy_stream) != ACG_OK)
        return fail(ctx, ACG_EHIP, "reassembly pass launch failed");
    return launch_stats(ctx, take, true);
}

static int fetch_msgs(acg_ctx* ctx, int lag, acg_msg* out, acg_oooi* oooi, int max_msgs, int* nmsgs, unsigned char* status = nullptr)
{
    if (status && !ctx->reasm) return fail(ctx, ACG_ESTATE, "reassembly is off (acg_reasm_enable first)");
    unsigned int pending = 0, take = 0;
    RingSpan span;
    int rc = ring_upto(ctx, lag, &span);
    if (rc != ACG_OK) return rc;
    if (!span.any) return commit_imports(ctx);
    if (!ctx->d_crctab) return fail(ctx, ACG_ESTATE, "context created without ACG_F_REPAIR");
    // A call splits and copies the oldest min(pending, max_msgs) blocks only (a block yields at most one message, so they
    // all fit) and consumes exactly those: draining a long queue through a small buffer costs what it hands out, not the
    // square of it, and the staging follows the caller's buffer, not the ring.
    rc = ring_claim(ctx, span, max_msgs, &pending, &take);
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
    // the statuses are per consumed block: kept record j is the j-th block the label pass kept
    std::vector<unsigned char> rs_status;                         // [take] statuses, [take] keep
    std::vector<unsigned int> rs_block;
    if (status && take) {
        rs_status.resize(2 * (size_t)take);
        if (acg_rs_fetch_status(ctx->reasm, ctx->copy_stream, take, rs_status.data(), labels ? rs_status.data() + take : nullptr) != ACG_OK)
            return fail(ctx, ACG_EHIP, "reassembly: statuses");
        for (unsigned int i = 0; i < take; ++i)
            if (!labels || rs_status[take + i]) rs_block.push_back(i);
        if (rs_block.size() != nrec) return fail(ctx, ACG_EHIP, "reassembly: statuses");
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
        if (status) status[kept - 1] = rs_status[rs_block[i]];
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

extern "C" int acg_collect_msgs_reasm(acg_ctx* ctx, int lag, acg_msg* out, acg_oooi* oooi, unsigned char* status, int max_msgs, int* nmsgs)
{
    if (!ctx || !nmsgs || (max_msgs > 0 && (!out || !status)) || lag < 0 || lag >= acg_ctx::NCALL - 1) return ACG_EINVAL;
    *nmsgs = 0;
    unsigned char none;
    return fetch_msgs(ctx, lag, out, oooi, max_msgs, nmsgs, status ? status : &none);
}

extern "C" int acg_drain_msgs_reasm(acg_ctx* ctx, acg_msg* out, acg_oooi* oooi, unsigned char* status, int max_msgs, int* nmsgs)
{
    if (!ctx || !nmsgs || (max_msgs > 0 && (!out || !status))) return ACG_EINVAL;
    *nmsgs = 0;
    unsigned char none;
    return fetch_msgs(ctx, DRAIN, out, oooi, max_msgs, nmsgs, status ? status : &none);
}

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
int label_filter_dev(const acg_msg_filter* f, AcgLabelFilter* d)
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

// ---- reassembly of multi-block messages (reasm.hip; host side: flights.cpp) ------------------------------------------------
extern "C" int acg_reasm_enable(acg_ctx* ctx, const acg_reasm_config* cfg)
{
    acg_reasm_config eff;
    if (!ctx || (cfg && !acg_rs_config_ok(cfg, &eff))) return ACG_EINVAL;
    // (one text for each code: the product library has no room for more, tests/test_host_logic.py's size rule)
    if (hipSetDevice(ctx->cfg.device) != hipSuccess || (ctx->reasm && hipStreamSynchronize(ctx->copy_stream) != hipSuccess)) return fail(ctx, ACG_EHIP, "reassembly: device");
    if (ctx->reasm) acg_rs_destroy(ctx->reasm);
    ctx->reasm = nullptr;
    if (!cfg) return ACG_OK;
    if (!acg_rs_create || !ctx->d_crctab) return fail(ctx, ACG_ESTATE, "reassembly: context created without ACG_F_REPAIR");
    if (ctx->cfg.nch > (1 << 20)) return fail(ctx, ACG_EINVAL, "reassembly: more than 2^20 channels");
    const int rc = acg_rs_create(&ctx->reasm, cfg);
    return rc == ACG_OK ? rc : fail(ctx, rc, "reassembly: allocation failed");
}

extern "C" int acg_drain_reassembled(acg_ctx* ctx, acg_reasm_msg* out, int max, int* n, char* text, size_t cap, size_t* nbytes, int* dropped)
{
    if (!ctx || !n || !nbytes || max < 0 || (max > 0 && !out) || (cap > 0 && !text)) return ACG_EINVAL;
    *n = 0;
    *nbytes = 0;
    if (!ctx->reasm) return fail(ctx, ACG_ESTATE, "reassembly is off");
    if (hipSetDevice(ctx->cfg.device) != hipSuccess) return fail(ctx, ACG_EHIP, "reassembly: device");
    const int rc = acg_rs_drain(ctx->reasm, ctx->copy_stream, out, max, n, text, cap, nbytes, dropped);
    return rc == ACG_OK ? rc : fail(ctx, rc, rc == ACG_EAGAIN ? "more completed messages queued than fit: call again" : "reassembly: hand-over");
}

extern "C" const char* acg_reasm_status_name(int status)
{
    static const char* const name[8] = {"unknown", "complete", "in progress", "skipped", "duplicate", "out of sequence", "invalid args", "overflow"};
    return name[status >= 0 && status < 8 ? status : 0];
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
