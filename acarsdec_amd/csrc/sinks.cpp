// sinks.cpp -- the batch sinks' host runtime: ONE object (AcgOutputs: a take ordered once, up to ACG_OUT_LEGS_MAX legs rendered from
// it by outs.hip's sequence), one fetch and one hand-out.  The JSON sink and the text sink are one-leg instances behind entry points
// that keep their own arguments and texts; the outputs are an instance with the legs the host asks for.  The flight table's text,
// its configuration and entry points, in between.
#include <climits>

#include "acg_ctx.h"

// ---- the rendered kinds (json.hip: buildjson()'s lines; text.hip: printoneline(), printmsg(), Netoutpp(), Netoutsv()).  A kind
// supplies the check of its configuration and what it renders once on the host (its AcgJsonDev / AcgTextDev and the channels'
// frequency tokens), further down; its sink supplies the argument checks and the texts of its entry points.
static_assert(ACG_JS_LINE_MAX == ACG_JSON_LINE_MAX, "line bound");
static_assert(ACG_TX_REC_MAX == ACG_TEXT_REC_MAX, "record bound");
static_assert(ACG_OUT_MSGS > ACG_TEXT_SV && ACG_OUT_JSON > ACG_TEXT_SV && ACG_OUT_MSGS != ACG_OUT_JSON, "leg kinds are distinct");

struct AcgSinkFormat {
    size_t rec_max;                         // the longest record
    unsigned int max_take;                  // the most records one pass takes: their offsets are 32-bit
    bool json;                              // json.hip's kernels, else text.hip's
};
static const AcgSinkFormat SINK_JSON = {ACG_JSON_LINE_MAX, (1u << 31) / ACG_JSON_LINE_MAX, true};
static const AcgSinkFormat SINK_TEXT = {ACG_TEXT_REC_MAX, (1u << 31) / ACG_TEXT_REC_MAX, false};
static const unsigned int MAX_TAKE = std::min(SINK_JSON.max_take, SINK_TEXT.max_take);     // what a lab entry takes whatever its legs

static const char* const JSON_OFF = "JSON sink is off: acg_json_enable first";
static const char* const TEXT_OFF = "text sink is off: acg_text_enable first";
static const char* const OUTPUTS_OFF = "outputs are off: acg_outputs_enable first";

static bool leg_is_text(int kind) { return kind >= ACG_TEXT_ONELINE && kind <= ACG_TEXT_SV; }

static const AcgSinkFormat* leg_format(int kind) { return kind == ACG_OUT_JSON ? &SINK_JSON : leg_is_text(kind) ? &SINK_TEXT : nullptr; }

static size_t leg_rec_max(int kind) { return kind == ACG_OUT_MSGS ? sizeof(acg_msg) : leg_format(kind)->rec_max; }

// what a kind renders once on the host
struct SinkBlob {
    int rc = ACG_OK;                        // ACG_EINVAL: a stretch does not fit (cannot happen); outputs_create hands it on
    std::vector<unsigned char> cfg, freq;
};
static bool json_config_ok(const acg_json_config* c);
static bool text_config_ok(const acg_text_config* c);
static SinkBlob json_blob(const acg_json_config* cfg, const int* Fr_hz, int nch);
static SinkBlob text_blob(const acg_text_config* cfg, const int* Fr_hz, int nch);

// ---- the configuration: acg_outputs_config; a sink's own configuration is the one-leg case of it ---------------------------------
static acg_outputs_config json_as_outputs(const acg_json_config* j)
{
    acg_outputs_config c;
    std::memset(&c, 0, sizeof(c));
    c.nlegs = 1;
    c.leg[0].kind = ACG_OUT_JSON;
    c.t0_sec = j->t0_sec;
    c.t0_usec = j->t0_usec;
    std::memcpy(c.station_id, j->station_id, sizeof(c.station_id));
    std::memcpy(c.app_name, j->app_name, sizeof(c.app_name));
    std::memcpy(c.app_ver, j->app_ver, sizeof(c.app_ver));
    return c;
}

static acg_outputs_config text_as_outputs(const acg_text_config* t)
{
    acg_outputs_config c;
    std::memset(&c, 0, sizeof(c));
    c.nlegs = 1;
    c.leg[0].kind = t->format;
    c.leg[0].flags = t->flags;
    c.t0_sec = t->t0_sec;
    c.t0_usec = t->t0_usec;
    std::memcpy(c.station_id, t->station_id, sizeof(c.station_id));
    return c;
}

// the configuration as the JSON kind's and as leg l's text kind's: what json_config_ok / text_config_ok check and the blobs render
static acg_json_config outputs_json_config(const acg_outputs_config* c)
{
    acg_json_config j;
    std::memset(&j, 0, sizeof(j));
    j.t0_sec = c->t0_sec;
    j.t0_usec = c->t0_usec;
    std::memcpy(j.station_id, c->station_id, sizeof(j.station_id));
    std::memcpy(j.app_name, c->app_name, sizeof(j.app_name));
    std::memcpy(j.app_ver, c->app_ver, sizeof(j.app_ver));
    return j;
}

static acg_text_config outputs_text_config(const acg_outputs_config* c, int l)
{
    acg_text_config t;
    std::memset(&t, 0, sizeof(t));
    t.format = c->leg[l].kind;
    t.flags = c->leg[l].flags;
    t.t0_sec = c->t0_sec;
    t.t0_usec = c->t0_usec;
    std::memcpy(t.station_id, c->station_id, sizeof(t.station_id));
    return t;
}

static bool outputs_config_ok(const acg_outputs_config* c)
{
    if (!c || c->nlegs < 1 || c->nlegs > ACG_OUT_LEGS_MAX) return false;
    const acg_json_config j = outputs_json_config(c);
    if (!json_config_ok(&j)) return false;                        // t0 and the three strings, whatever the legs
    for (int l = 0; l < c->nlegs; ++l) {
        const int kind = c->leg[l].kind;
        if (leg_is_text(kind)) {
            const acg_text_config t = outputs_text_config(c, l);
            if (!text_config_ok(&t)) return false;                // the flags the format takes
        } else if ((kind != ACG_OUT_MSGS && kind != ACG_OUT_JSON) || c->leg[l].flags) {
            return false;
        }
        for (int k = 0; k < l; ++k)
            if (c->leg[k].kind == kind) return false;
    }
    return true;
}

extern "C" int acg_outputs_config_check(const acg_outputs_config* cfg) { return outputs_config_ok(cfg) ? ACG_OK : ACG_EINVAL; }

// ---- the object: the legs of one configuration over one order.  It owns the four order arrays, ONE block of counters (four words
// per leg: bytes, records of the last pass; the level guard; unused -- one small copy brings every leg's counts) and the keys of
// what it last handed out; a rendered leg owns its configuration on the device and its lengths, offsets and bytes; the MSGS leg
// has only the packed arrays outs.hip's gather fills and word 1 of its four counters.
struct AcgLeg {
    const AcgSinkFormat* fmt = nullptr;     // null: the MSGS leg, or no leg
    void* d_cfg = nullptr;                  // AcgJsonDev / AcgTextDev
    unsigned char* d_freq = nullptr;        // [nch] frequency tokens: [8] "%3.3f" / [ACG_TX_FREQ_SLOT] "F:%3.3f "
    unsigned int *d_len = nullptr, *d_off = nullptr, *d_wg = nullptr;
    unsigned char* d_out = nullptr;         // cap * fmt->rec_max bytes
};
struct AcgOutputs {
    acg_outputs_config cfg{};
    AcgLeg leg[ACG_OUT_LEGS_MAX];
    int msgs_leg = -1;
    unsigned int* d_cnt = nullptr;          // [4 * ACG_OUT_LEGS_MAX]
    size_t cap = 0;                         // records the work space below and the legs' hold
    unsigned long long *d_key = nullptr, *d_key_s = nullptr;
    unsigned int *d_idx = nullptr, *d_idx_s = nullptr;
    AcgMsgRec* d_gmsgs = nullptr;           // the MSGS leg
    acg_oooi* d_goooi = nullptr;
    unsigned int last_nrecs = 0;            // records the most recent fetch handed out: the first keys of d_key_s (acg_sink_keys)
};

static void outputs_free_work(AcgOutputs* o)
{
    for (AcgLeg& g : o->leg) {
        hipFree(g.d_len); hipFree(g.d_off); hipFree(g.d_wg); hipFree(g.d_out);
        g.d_len = g.d_off = g.d_wg = nullptr;
        g.d_out = nullptr;
    }
    hipFree(o->d_key); hipFree(o->d_key_s); hipFree(o->d_idx); hipFree(o->d_idx_s);
    hipFree(o->d_gmsgs); hipFree(o->d_goooi);
    o->d_key = o->d_key_s = nullptr;
    o->d_idx = o->d_idx_s = nullptr;
    o->d_gmsgs = nullptr;
    o->d_goooi = nullptr;
    o->cap = 0;
}

void outputs_destroy(AcgOutputs* o)
{
    if (!o) return;
    outputs_free_work(o);
    for (AcgLeg& g : o->leg) { hipFree(g.d_cfg); hipFree(g.d_freq); }
    hipFree(o->d_cnt);
    delete o;
}

// cfg has passed outputs_config_ok.  ACG_OK, ACG_ENOMEM or ACG_EHIP (or a blob's own verdict)
static int outputs_create(AcgOutputs** out, const acg_outputs_config* cfg, const int* Fr_hz, int nch)
{
    AcgOutputs* o = new (std::nothrow) AcgOutputs();
    if (!o) return ACG_ENOMEM;
    o->cfg = *cfg;
    int rc = ACG_OK;
    if (hipMalloc(&o->d_cnt, 4 * ACG_OUT_LEGS_MAX * sizeof(unsigned int)) != hipSuccess) rc = ACG_ENOMEM;
    else if (hipMemset(o->d_cnt, 0, 4 * ACG_OUT_LEGS_MAX * sizeof(unsigned int)) != hipSuccess) rc = ACG_EHIP;
    for (int l = 0; l < cfg->nlegs && rc == ACG_OK; ++l) {
        AcgLeg& g = o->leg[l];
        g.fmt = leg_format(cfg->leg[l].kind);
        if (!g.fmt) {
            o->msgs_leg = l;
            continue;
        }
        const acg_json_config j = outputs_json_config(cfg);
        const acg_text_config t = outputs_text_config(cfg, l);
        const SinkBlob blob = g.fmt->json ? json_blob(&j, Fr_hz, nch) : text_blob(&t, Fr_hz, nch);
        if (blob.rc != ACG_OK) rc = blob.rc;
        else if (hipMalloc(&g.d_cfg, blob.cfg.size()) != hipSuccess || hipMalloc(&g.d_freq, blob.freq.size()) != hipSuccess) rc = ACG_ENOMEM;
        else if (hipMemcpy(g.d_cfg, blob.cfg.data(), blob.cfg.size(), hipMemcpyHostToDevice) != hipSuccess ||
                 hipMemcpy(g.d_freq, blob.freq.data(), blob.freq.size(), hipMemcpyHostToDevice) != hipSuccess)
            rc = ACG_EHIP;
    }
    if (rc == ACG_OK && hipDeviceSynchronize() != hipSuccess) rc = ACG_EHIP;
    if (rc != ACG_OK) {
        outputs_destroy(o);
        return rc;
    }
    *out = o;
    return ACG_OK;
}

// the order arrays and every leg's work space and output buffer for n records, grown on demand as d_kmsgs is
static int outputs_reserve(AcgOutputs* o, size_t n)
{
    if (n <= o->cap) return ACG_OK;
    outputs_free_work(o);
    const size_t want = std::max<size_t>(n, 4096);
    bool ok = hipMalloc(&o->d_key, want * 8) == hipSuccess && hipMalloc(&o->d_key_s, want * 8) == hipSuccess &&
              hipMalloc(&o->d_idx, want * 4) == hipSuccess && hipMalloc(&o->d_idx_s, want * 4) == hipSuccess;
    if (ok && o->msgs_leg >= 0)
        ok = hipMalloc(&o->d_gmsgs, want * sizeof(AcgMsgRec)) == hipSuccess && hipMalloc(&o->d_goooi, want * sizeof(acg_oooi)) == hipSuccess;
    for (AcgLeg& g : o->leg)
        if (ok && g.fmt)
            ok = hipMalloc(&g.d_len, want * 4) == hipSuccess && hipMalloc(&g.d_off, want * 4) == hipSuccess &&
                 hipMalloc(&g.d_wg, 2 * (want / 256 + 1) * 4) == hipSuccess && hipMalloc(&g.d_out, want * g.fmt->rec_max) == hipSuccess;
    if (!ok) {
        outputs_free_work(o);
        return ACG_ENOMEM;
    }
    o->cap = want;
    return ACG_OK;
}

static AcgOutsPass outputs_pass(const AcgOutputs* o, const AcgMsgRec* recs, const void* oooi, const unsigned int* total, unsigned int nmax, bool lvl_from_rec,
                                const int* chmap, unsigned int nmap)
{
    AcgOutsPass p;
    std::memset(&p, 0, sizeof(p));
    p.order.recs = recs;
    p.order.oooi = (const unsigned char*)oooi;
    p.order.total = total;
    p.order.nmax = nmax;
    p.order.key = o->d_key; p.order.key_s = o->d_key_s;
    p.order.idx = o->d_idx; p.order.idx_s = o->d_idx_s;
    p.order.chmap = chmap;
    p.order.nmap = nmap;
    for (int l = 0; l < o->cfg.nlegs; ++l) {
        const AcgLeg& g = o->leg[l];
        if (!g.fmt) continue;
        AcgSinkPass& sp = p.leg[p.nrender];
        sp = p.order;                                             // the records, their order and the map: every leg's
        sp.cfg = g.d_cfg;
        sp.freq = g.d_freq;
        sp.lvl_from_rec = lvl_from_rec ? 1 : 0;
        sp.len = g.d_len; sp.off = g.d_off;
        sp.wg_sum = g.d_wg; sp.wg_cnt = g.d_wg + (o->cap / 256 + 1);
        sp.counters = o->d_cnt + 4 * l;
        sp.out = g.d_out;
        sp.out_cap = (unsigned int)std::min<size_t>(o->cap * g.fmt->rec_max, 0xffffffffu);
        p.is_json[p.nrender++] = g.fmt->json;
    }
    if (o->msgs_leg >= 0) {
        p.g_recs = o->d_gmsgs;
        p.g_oooi = (unsigned char*)o->d_goooi;
        p.g_count = o->d_cnt + 4 * o->msgs_leg + 1;
    }
    return p;
}

// the MSGS leg's records as they came from the device, turned into what fetch_msgs hands out, in place (lab: the level is the
// record's own, as the lab entries take it)
static void outputs_finish_msgs(acg_msg* m, unsigned int n, const std::vector<int>* chnum, bool lab)
{
    for (unsigned int i = 0; i < n; ++i) {
        AcgMsgRec r;
        std::memcpy(&r, &m[i], sizeof(r));
        if (!lab) m[i].lvl = acg_host_level_db(r.lvlsum, r.bitcount);         // acars.c:351
        m[i].soh_sample = r.end_sample - (long long)r.soh_back;               // acars.c:290
        m[i].reserved1 = 0;
        m[i].reserved2 = 0;
        m[i].reserved3 = 0;
        if (chnum && (size_t)(unsigned int)r.chn < chnum->size()) m[i].chn = (*chnum)[(size_t)r.chn];
    }
}

// Behind acg_launch_outs on `stream`: ONE copy of all legs' counters and a sync, their check, then the legs' bytes and tables
// and a sync.  take: the records the pass ran over.  A rendered leg's table is handed out where the caller has room for one (the
// JSON sink's entry points have none).  lab: a leg that does not fit says ACG_EAGAIN with every leg's nbytes and *nrecs set and
// nothing written (a fetch has sized the take so that everything fits).  ACG_EHIP with *what set, ACG_EAGAIN or ACG_OK.
static int outputs_hand_out(const AcgOutputs* o, hipStream_t stream, unsigned int take, acg_out_buf* bufs, const std::vector<int>* chnum, bool lab,
                            unsigned int* nrecs, const char** what)
{
    unsigned int cnt[4 * ACG_OUT_LEGS_MAX] = {};
    *what = "sink pass: copy failed";
    if (hipMemcpyAsync(cnt, o->d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return ACG_EHIP;
    const unsigned int n = cnt[1];                                // (leg 0's records: every leg counts in word 1 of its four)
    *nrecs = n;                                                   // (to be believed with ACG_OK and ACG_EAGAIN)
    bool fits = true;
    for (int l = 0; l < o->cfg.nlegs; ++l) {
        const AcgSinkFormat* fmt = o->leg[l].fmt;
        const unsigned int c0 = cnt[4 * l], c1 = cnt[4 * l + 1];
        *what = "sink pass: counts out of range";
        if (c1 > take || (fmt && (size_t)c0 > (size_t)take * fmt->rec_max)) return ACG_EHIP;
        *what = "sink pass: the legs disagree on the number of records";
        if (c1 != n) return ACG_EHIP;
        bufs[l].nbytes = fmt ? (size_t)c0 : (size_t)c1 * sizeof(acg_msg);
        if (bufs[l].nbytes > bufs[l].cap) fits = false;
    }
    *what = "sink pass: counts out of range";
    if (!fits) return lab ? ACG_EAGAIN : ACG_EHIP;
    *what = "sink pass: copy failed";
    for (int l = 0; l < o->cfg.nlegs && n; ++l) {                 // (kept records sort in front of dropped ones: the first n of everything)
        const AcgLeg& g = o->leg[l];
        if (g.fmt) {
            if (hipMemcpyAsync(bufs[l].out, g.d_out, bufs[l].nbytes, hipMemcpyDeviceToHost, stream) != hipSuccess ||
                (bufs[l].offs && hipMemcpyAsync(bufs[l].offs, g.d_off, (size_t)n * sizeof(unsigned int), hipMemcpyDeviceToHost, stream) != hipSuccess))
                return ACG_EHIP;
        } else if (hipMemcpyAsync(bufs[l].out, o->d_gmsgs, (size_t)n * sizeof(AcgMsgRec), hipMemcpyDeviceToHost, stream) != hipSuccess ||
                   hipMemcpyAsync(bufs[l].oooi, o->d_goooi, (size_t)n * sizeof(acg_oooi), hipMemcpyDeviceToHost, stream) != hipSuccess) {
            return ACG_EHIP;
        }
    }
    if (n && hipStreamSynchronize(stream) != hipSuccess) return ACG_EHIP;
    for (int l = 0; l < o->cfg.nlegs; ++l) {
        if (!o->leg[l].fmt) outputs_finish_msgs((acg_msg*)bufs[l].out, n, chnum, lab);
        else if (bufs[l].offs) bufs[l].offs[n] = (unsigned int)bufs[l].nbytes;
    }
    *what = nullptr;
    return ACG_OK;
}

// the buffers of a caller of the outputs' own entry points against the legs: everything a leg writes to is there, a rendered
// leg's table included.  one_record: every leg holds at least one record
static bool outputs_bufs_ok(const acg_outputs_config* c, acg_out_buf* bufs, bool one_record)
{
    if (!bufs) return false;
    for (int l = 0; l < c->nlegs; ++l) {
        const bool msgs = c->leg[l].kind == ACG_OUT_MSGS;
        if ((bufs[l].cap > 0 && !bufs[l].out) || (!msgs && !bufs[l].offs) || (msgs && bufs[l].cap >= sizeof(acg_msg) && !bufs[l].oooi)) return false;
        if (one_record && bufs[l].cap < leg_rec_max(c->leg[l].kind)) return false;
    }
    for (int l = 0; l < c->nlegs; ++l) {
        bufs[l].nbytes = 0;
        if (bufs[l].offs) bufs[l].offs[0] = 0;
    }
    return true;
}

// What acg_json_enable, acg_text_enable and acg_outputs_enable share, behind the check of their configuration: the old instance
// leaves behind a stream sync; cfg == null leaves the slot off.  name: the first words of the messages
static int outputs_enable(acg_ctx* ctx, AcgOutputs** slot, const char* name, const acg_outputs_config* cfg, const int* Fr_hz)
{
    const auto said = [&](int code, const char* rest) { return fail(ctx, code, (std::string(name) + rest).c_str()); };
    if (hipSetDevice(ctx->cfg.device) != hipSuccess || (*slot && hipStreamSynchronize(ctx->copy_stream) != hipSuccess))
        return said(ACG_EHIP, ": the device does not answer");
    outputs_destroy(*slot);
    *slot = nullptr;
    if (!cfg) return ACG_OK;
    if (!acg_launch_outs) return said(ACG_ESTATE, ": not in this build");
    if (!ctx->d_crctab) return said(ACG_ESTATE, ": context created without ACG_F_REPAIR");
    if (ctx->cfg.nch > (1 << 20)) return said(ACG_EINVAL, ": more than 2^20 channels");
    const int rc = outputs_create(slot, cfg, Fr_hz, ctx->cfg.nch);
    return rc == ACG_OK ? rc : said(rc, ": allocation failed");
}

// fetch_msgs' sibling, for the sinks and the outputs: the same claim, split, label pass, flight pass and statistics, ONCE; then
// outs.hip's passes for every leg of `o` on the same stream, and only the legs' packed bytes, their counters and their tables cross
// to the host, in two round trips.  A block yields at most one record of at most recmax bytes per leg: the oldest min(max_recs,
// min over legs of cap / recmax) always fit every leg.  is_off: what the entry point says while its instance is off.  own_bufs: an
// entry point of the outputs, whose caller's buffers are checked here; a sink's entry point has checked its own arguments and
// hands in its one leg's buffer, with or without a table.
static int outputs_fetch(acg_ctx* ctx, AcgOutputs* o, const char* is_off, int lag, acg_out_buf* bufs, bool own_bufs, int max_recs, int* nrecs)
{
    if (!ctx->d_crctab) return fail(ctx, ACG_ESTATE, "context created without ACG_F_REPAIR");
    if (!o) return fail(ctx, ACG_ESTATE, is_off);
    if (own_bufs && (max_recs < 1 || !outputs_bufs_ok(&o->cfg, bufs, true)))
        return fail(ctx, ACG_EINVAL, "outputs: a leg's buffer holds less than one record, a buffer or table is missing, or max_recs < 1");
    o->last_nrecs = 0;
    size_t fit = (size_t)max_recs;
    for (int l = 0; l < o->cfg.nlegs; ++l) {
        fit = std::min(fit, bufs[l].cap / leg_rec_max(o->cfg.leg[l].kind));
        if (o->leg[l].fmt) fit = std::min<size_t>(fit, o->leg[l].fmt->max_take);
    }
    unsigned int pending = 0, take = 0;
    RingSpan span;
    int rc = ring_upto(ctx, lag, &span);
    if (rc != ACG_OK) return rc;
    if (!span.any) return commit_imports(ctx);
    rc = ring_claim(ctx, span, (int)std::min<size_t>(fit, INT_MAX), &pending, &take);
    if (!take) {
        if (const int cr = commit_imports(ctx)) return cr;
        return ring_result(ctx, rc, pending, take, "more messages queued than fit: call again");
    }
    if (const int gr = grow_msg_stage(ctx, take)) return gr;
    if (const int gr = grow_label_stage(ctx, take)) return gr;
    if (outputs_reserve(o, take) != ACG_OK) return fail(ctx, ACG_ENOMEM, "sink: work space");
    unsigned int* d_total = nullptr;
    if (const int lr = launch_split(ctx, take, true, &d_total)) return lr;
    // the map in force at hand-out (acg_set_channel_numbers)
    const AcgOutsPass op = outputs_pass(o, ctx->d_kmsgs, ctx->d_oooi, d_total, take, false, ctx->d_chnum, ctx->d_chnum ? (unsigned int)ctx->cfg.nch : 0u);
    if (acg_launch_outs(&op, ctx->copy_stream) != 0) return fail(ctx, ACG_EHIP, "sink pass launch failed");
    unsigned int n = 0;
    const char* what = nullptr;
    if (const int hr = outputs_hand_out(o, ctx->copy_stream, take, bufs, &ctx->chnum, false, &n, &what)) return fail(ctx, hr, what);
    ctx->consumed += take;
    o->last_nrecs = n;
    *nrecs = (int)n;
    return ring_result(ctx, rc, pending, take, "more messages queued than fit: call again");
}

// a sink's fetch: its one leg's buffer (offs == null: no table), and the leg's bytes where records came
static int sink_fetch(acg_ctx* ctx, AcgOutputs* o, const char* is_off, int lag, char* out, size_t cap, size_t* nbytes, unsigned int* offs, int max_recs,
                      int* nrecs)
{
    acg_out_buf b = {out, cap, offs, nullptr, 0};
    const int rc = outputs_fetch(ctx, o, is_off, lag, &b, false, max_recs, nrecs);
    if (*nrecs) *nbytes = b.nbytes;
    return rc;
}

// word 2 of leg `leg`'s counters
static int sink_level_guard(acg_ctx* ctx, const AcgOutputs* o, const char* is_off, int leg, unsigned int* near_midpoint)
{
    *near_midpoint = 0;
    if (!o) return fail(ctx, ACG_ESTATE, is_off);
    if (leg < 0 || leg >= o->cfg.nlegs || !o->leg[leg].fmt) return fail(ctx, ACG_EINVAL, "outputs: not a JSON or text leg");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
    HIPCHK(ctx, hipMemcpy(near_midpoint, o->d_cnt + 4 * leg + 2, sizeof(unsigned int), hipMemcpyDeviceToHost));
    return ACG_OK;
}

// the order keys of the records the most recent fetch of an instance handed out: one small copy, no kernel
extern "C" int acg_sink_keys(acg_ctx* ctx, int sink, unsigned long long* keys, int max, int* n)
{
    if (!ctx || !n || max < 0 || (max > 0 && !keys) || (sink != ACG_SINK_JSON && sink != ACG_SINK_TEXT && sink != ACG_SINK_OUTPUTS)) return ACG_EINVAL;
    *n = 0;
    const AcgOutputs* o = sink == ACG_SINK_JSON ? ctx->json : sink == ACG_SINK_TEXT ? ctx->text : ctx->outs;
    if (!o) return fail(ctx, ACG_ESTATE, sink == ACG_SINK_JSON ? JSON_OFF : sink == ACG_SINK_TEXT ? TEXT_OFF : OUTPUTS_OFF);
    *n = (int)o->last_nrecs;
    if (o->last_nrecs > (unsigned int)max) return fail(ctx, ACG_EAGAIN, "sink keys: *n keys do not fit");
    // (kept records sort in front of dropped ones: the first keys; the pass that wrote them has been waited for)
    if (o->last_nrecs && (hipSetDevice(ctx->cfg.device) != hipSuccess ||
                          hipMemcpy(keys, o->d_key_s, (size_t)o->last_nrecs * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess))
        return fail(ctx, ACG_EHIP, "sink keys: copy failed");
    return ACG_OK;
}

// ---- the lab entries' runtime: designed records through the label pass and outs.hip's sequence, no context ---------------------
// records a lab entry may hand to a renderer
static bool sink_records_ok(const acg_msg* in, int n, int nch)
{
    for (int i = 0; i < n; ++i)
        if (in[i].chn < 0 || in[i].chn >= nch || in[i].end_bit < 0 || in[i].end_bit >= (1ll << 44)) return false;
    return true;
}

// The self tests behind their own argument checks (cfg has passed outputs_config_ok): label pass and every leg of cfg over n
// records, handed out as a fetch hands out.  own_bufs as outputs_fetch's.  check: null, or what the entry holds the pass against
// before it believes it.  *got: the records, with ACG_OK and with ACG_EAGAIN (a leg does not fit: every leg's nbytes says what it
// needs, nothing is written).  n == 0 is ACG_OK; ACG_ENODEV without a device.
typedef int (*OutputsCheck)(const AcgOutputs* o, unsigned int n, const unsigned int* d_kept, const acg_out_buf* bufs);
static int outputs_selftest(const acg_msg* in, int n, const acg_msg_filter* f, const acg_outputs_config* cfg, const int* Fr_hz, int nch, acg_out_buf* bufs,
                            bool own_bufs, unsigned int* got, OutputsCheck check)
{
    AcgLabelFilter d;
    *got = 0;
    if (label_filter_dev(f, &d) != ACG_OK || !sink_records_ok(in, n, nch) || (own_bufs && !outputs_bufs_ok(cfg, bufs, false))) return ACG_EINVAL;
    if (n == 0) return ACG_OK;
    int ndev = 0;
    if (!acg_launch_outs || hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return ACG_ENODEV;
    AcgOutputs* o = nullptr;
    int rc = outputs_create(&o, cfg, Fr_hz, nch);
    if (rc != ACG_OK) return rc;
    rc = outputs_reserve(o, (size_t)n);
    if (rc == ACG_OK) {
        LabStage lab((size_t)n);
        lab.stage(in, (unsigned int)n, true, true);
        const AcgOutsPass op = outputs_pass(o, lab.d_out, lab.d_oooi, lab.d_total(), (unsigned int)n, true, nullptr, 0u);
        const char* what = nullptr;
        if (!lab.ok()) rc = ACG_ENOMEM;
        else if (lab.label((unsigned int)n, &d) != 0 || acg_launch_outs(&op, nullptr) != 0) rc = ACG_EHIP;
        else rc = outputs_hand_out(o, nullptr, (unsigned int)n, bufs, nullptr, true, got, &what);
        if (rc == ACG_OK && check) rc = check(o, *got, lab.d_total(), bufs);
    }
    outputs_destroy(o);
    return rc;
}

// a sink's self test: its one leg's buffer (offs == null: no table); the bytes and the records with ACG_OK and with ACG_EAGAIN
static int sink_selftest(const acg_outputs_config& cfg, const acg_msg* in, int n, const acg_msg_filter* f, const int* Fr_hz, int nch, char* out, size_t cap,
                         size_t* nbytes, unsigned int* offs, int* nrecs)
{
    acg_out_buf b = {out, cap, offs, nullptr, 0};
    unsigned int got = 0;
    const int rc = outputs_selftest(in, n, f, &cfg, Fr_hz, nch, &b, false, &got, nullptr);
    if (rc == ACG_EINVAL) return rc;
    const bool said = rc == ACG_OK || rc == ACG_EAGAIN;
    *nbytes = said ? b.nbytes : 0;
    *nrecs = said ? (int)got : 0;
    if (n == 0 && offs) offs[0] = 0;
    return rc;
}

// What the two timing entries share, behind their argument checks: n designed records staged and labelled once (no filter), the
// channel map under ACG_SINK_MAP (slot l -> nch - 1 - l: what the look-up costs), the event pair and the alternating loop -- in
// every round arm a launches the passes of arm[a][0] and, where there is one, arm[a][1], one behind the other, between two
// events on the null stream; ms[a * reps + r].  The instances are the caller's and keep what the last round left on the device.
static int time_passes(const acg_msg* in, int n, int nch, int warmup, int reps, AcgOutputs* const arm[2][2], float* ms)
{
    AcgLabelFilter none;
    std::memset(&none, 0, sizeof(none));
    hipEvent_t ev[2] = {nullptr, nullptr};
    int* d_map = nullptr;
    int rc = ACG_OK;
    for (int a = 0; a < 4 && rc == ACG_OK; ++a)
        if (arm[a / 2][a % 2]) rc = outputs_reserve(arm[a / 2][a % 2], (size_t)n);
    if (rc == ACG_OK) {
        LabStage lab((size_t)n);
        lab.stage(in, (unsigned int)n, true, true);
        if (!lab.ok()) rc = ACG_ENOMEM;
        if (rc == ACG_OK && acg_tune_get("ACG_SINK_MAP", 0)) {
            std::vector<int> m((size_t)nch);
            for (int l = 0; l < nch; ++l) m[(size_t)l] = nch - 1 - l;
            if (hipMalloc(&d_map, m.size() * sizeof(int)) != hipSuccess || hipMemcpy(d_map, m.data(), m.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
                rc = ACG_EHIP;
        }
        if (rc == ACG_OK && (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess)) rc = ACG_EHIP;
        if (rc == ACG_OK && (lab.label((unsigned int)n, &none) != 0 || hipDeviceSynchronize() != hipSuccess)) rc = ACG_EHIP;
        AcgOutsPass op[2][2];
        for (int a = 0; a < 4 && rc == ACG_OK; ++a)
            if (arm[a / 2][a % 2])
                op[a / 2][a % 2] = outputs_pass(arm[a / 2][a % 2], lab.d_out, lab.d_oooi, lab.d_total(), (unsigned int)n, true, d_map, d_map ? (unsigned int)nch : 0u);
        for (int r = -warmup; r < reps && rc == ACG_OK; ++r)
            for (int a = 0; a < 2 && rc == ACG_OK; ++a) {
                float t = 0.0f;
                if (hipEventRecord(ev[0], nullptr) != hipSuccess || acg_launch_outs(&op[a][0], nullptr) != 0 ||
                    (arm[a][1] && acg_launch_outs(&op[a][1], nullptr) != 0) || hipEventRecord(ev[1], nullptr) != hipSuccess ||
                    hipEventSynchronize(ev[1]) != hipSuccess || hipEventElapsedTime(&t, ev[0], ev[1]) != hipSuccess)
                    rc = ACG_EHIP;
                else if (r >= 0) ms[a * reps + r] = t;
            }
    }
    if (ev[0]) hipEventDestroy(ev[0]);
    if (ev[1]) hipEventDestroy(ev[1]);
    hipFree(d_map);
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
    if (!cfg) return outputs_enable(ctx, &ctx->json, "JSON sink", nullptr, nullptr);
    if (!json_config_ok(cfg)) return fail(ctx, ACG_EINVAL, "JSON sink: t0 outside [10^9, 4 * 10^9) s / 0..999999 us, or an unterminated string");
    const acg_outputs_config one = json_as_outputs(cfg);
    return outputs_enable(ctx, &ctx->json, "JSON sink", &one, Fr_hz);
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
    return sink_fetch(ctx, ctx->json, JSON_OFF, lag, out, cap, nbytes, nullptr, INT_MAX, nlines);
}

extern "C" int acg_drain_json(acg_ctx* ctx, char* out, size_t cap, size_t* nbytes, int* nlines)
{
    if (const int rc = json_args(ctx, out, cap, nbytes, nlines)) return rc;
    return sink_fetch(ctx, ctx->json, JSON_OFF, DRAIN, out, cap, nbytes, nullptr, INT_MAX, nlines);
}

extern "C" int acg_lab_json_level_guard(acg_ctx* ctx, unsigned int* near_midpoint)
{
    if (!ctx || !near_midpoint) return ACG_EINVAL;
    return sink_level_guard(ctx, ctx->json, JSON_OFF, 0, near_midpoint);
}

extern "C" int acg_selftest_msg_json(const acg_msg* in, int n, const acg_msg_filter* f, const acg_json_config* cfg, const int* Fr_hz, int nch,
                                     char* out, size_t cap, size_t* nbytes, int* nlines)
{
    if (n < 0 || (n > 0 && !in) || !json_config_ok(cfg) || nch < 1 || nch > (1 << 20) || !nbytes || !nlines || (cap > 0 && !out) ||
        (unsigned int)n > SINK_JSON.max_take)
        return ACG_EINVAL;
    return sink_selftest(json_as_outputs(cfg), in, n, f, Fr_hz, nch, out, cap, nbytes, nullptr, nlines);
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
    if (!cfg) return outputs_enable(ctx, &ctx->text, "text sink", nullptr, nullptr);
    if (!text_config_ok(cfg))
        return fail(ctx, ACG_EINVAL, "text sink: unknown format, a flag the format does not take, t0 outside [10^9, 4 * 10^9) s / 0..999999 us, or an unterminated station_id");
    const acg_outputs_config one = text_as_outputs(cfg);
    return outputs_enable(ctx, &ctx->text, "text sink", &one, Fr_hz);
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
    return sink_fetch(ctx, ctx->text, TEXT_OFF, lag, out, cap, nbytes, offs, max_recs, nrecs);
}

extern "C" int acg_drain_text(acg_ctx* ctx, char* out, size_t cap, size_t* nbytes, unsigned int* offs, int max_recs, int* nrecs)
{
    if (const int rc = text_args(ctx, out, cap, nbytes, offs, max_recs, nrecs)) return rc;
    return sink_fetch(ctx, ctx->text, TEXT_OFF, DRAIN, out, cap, nbytes, offs, max_recs, nrecs);
}

extern "C" int acg_lab_text_level_guard(acg_ctx* ctx, unsigned int* near_midpoint)
{
    if (!ctx || !near_midpoint) return ACG_EINVAL;
    return sink_level_guard(ctx, ctx->text, TEXT_OFF, 0, near_midpoint);
}

extern "C" int acg_selftest_msg_text(const acg_msg* in, int n, const acg_msg_filter* f, const acg_text_config* cfg, const int* Fr_hz, int nch,
                                     char* out, size_t cap, size_t* nbytes, unsigned int* offs, int* nrecs)
{
    if (n < 0 || (n > 0 && !in) || !text_config_ok(cfg) || nch < 1 || nch > (1 << 20) || !nbytes || !nrecs || !offs || (cap > 0 && !out) ||
        (unsigned int)n > SINK_TEXT.max_take)
        return ACG_EINVAL;
    return sink_selftest(text_as_outputs(cfg), in, n, f, Fr_hz, nch, out, cap, nbytes, offs, nrecs);
}

// the JSON passes and the text passes over the same records, alternated: ms[0 .. reps) JSON, ms[reps .. 2 reps) text
extern "C" int acg_lab_time_sink_passes(const acg_msg* in, int n, const acg_json_config* jcfg, const acg_text_config* tcfg, int nch, int warmup,
                                        int reps, float* ms)
{
    if (n < 1 || !in || !json_config_ok(jcfg) || !text_config_ok(tcfg) || nch < 1 || nch > (1 << 20) || warmup < 0 || reps < 1 || !ms ||
        (unsigned int)n > MAX_TAKE || !sink_records_ok(in, n, nch))
        return ACG_EINVAL;
    int ndev = 0;
    if (!acg_launch_outs || hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return ACG_ENODEV;
    const acg_outputs_config jc = json_as_outputs(jcfg), tc = text_as_outputs(tcfg);
    AcgOutputs* arm[2][2] = {};                                   // the arms: JSON, text
    int rc = outputs_create(&arm[0][0], &jc, nullptr, nch);
    if (rc == ACG_OK) rc = outputs_create(&arm[1][0], &tc, nullptr, nch);
    if (rc == ACG_OK) rc = time_passes(in, n, nch, warmup, reps, arm, ms);
    outputs_destroy(arm[0][0]);
    outputs_destroy(arm[1][0]);
    return rc;
}

// ---- the outputs: their entry points ------------------------------------------------------------------------------------------------
extern "C" int acg_outputs_enable(acg_ctx* ctx, const acg_outputs_config* cfg, const int* Fr_hz)
{
    if (!ctx) return ACG_EINVAL;
    if (cfg && !outputs_config_ok(cfg))
        return fail(ctx, ACG_EINVAL, "outputs: 1 .. ACG_OUT_LEGS_MAX legs of pairwise distinct known kinds, a flag the kind does not take, t0 outside [10^9, 4 * 10^9) s / 0..999999 us, or an unterminated string");
    return outputs_enable(ctx, &ctx->outs, "outputs", cfg, Fr_hz);
}

extern "C" int acg_collect_outputs(acg_ctx* ctx, int lag, acg_out_buf* bufs, int max_recs, int* nrecs)
{
    if (!ctx || !nrecs || lag < 0 || lag >= acg_ctx::NCALL - 1) return ACG_EINVAL;
    *nrecs = 0;
    return outputs_fetch(ctx, ctx->outs, OUTPUTS_OFF, lag, bufs, true, max_recs, nrecs);
}

extern "C" int acg_drain_outputs(acg_ctx* ctx, acg_out_buf* bufs, int max_recs, int* nrecs)
{
    if (!ctx || !nrecs) return ACG_EINVAL;
    *nrecs = 0;
    return outputs_fetch(ctx, ctx->outs, OUTPUTS_OFF, DRAIN, bufs, true, max_recs, nrecs);
}

// The outputs' three lab entries are compiled into the lab library only (this unit sees ACG_LAB: _build.SEES): the product library
// is held below 0.82 of the lab library's size (tests/test_host_logic.py; LEDGER, "Combined outputs"), and exports the three
// names as functions that say ACG_ESTATE.
#ifndef ACG_LAB
extern "C" int acg_lab_outputs_level_guard(acg_ctx*, int, unsigned int*) { return ACG_ESTATE; }

extern "C" int acg_selftest_outputs(const acg_msg*, int, const acg_msg_filter*, const acg_outputs_config*, const int*, int, acg_out_buf*, int*) { return ACG_ESTATE; }

extern "C" int acg_lab_time_output_passes(const acg_msg*, int, const acg_outputs_config*, int, int, int, float*) { return ACG_ESTATE; }

// (the reassembly table's self test: the same rule)
extern "C" int acg_selftest_reasm(const acg_msg*, const int*, int, const acg_reasm_config*, const acg_msg_filter*, unsigned char*, acg_reasm_msg*, int, char*, size_t,
                                  int*, int*, float*) { return ACG_ESTATE; }
#else
extern "C" int acg_selftest_reasm(const acg_msg* in, const int* batch, int nbatch, const acg_reasm_config* cfg, const acg_msg_filter* f, unsigned char* status,
                                  acg_reasm_msg* done, int done_cap, char* text, size_t text_cap, int* ndone, int* dropped, float* pass_ms)
{
    acg_reasm_config eff;
    if (nbatch < 0 || !acg_rs_config_ok(cfg, &eff) || done_cap < 0 || !ndone || (nbatch > 0 && !batch) || (done_cap > 0 && !done) || (text_cap > 0 && !text))
        return ACG_EINVAL;
    AcgLabelFilter d;
    if (label_filter_dev(f, &d) != ACG_OK) return ACG_EINVAL;
    size_t total = 0, biggest = 0;
    for (int b = 0; b < nbatch; ++b) {
        if (batch[b] < 0) return ACG_EINVAL;
        total += (size_t)batch[b];
        biggest = std::max(biggest, (size_t)batch[b]);
    }
    if (total > 0 && (!in || !status)) return ACG_EINVAL;
    *ndone = 0;
    int ndev = 0;
    if (!acg_rs_create || hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return ACG_ENODEV;
    AcgReasm* t = nullptr;
    int rc = acg_rs_create(&t, cfg);
    if (rc != ACG_OK) return rc;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (pass_ms && (hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess)) rc = ACG_EHIP;
    if (rc == ACG_OK) {
        LabStage lab(biggest);
        if (!lab.ok()) rc = ACG_ENOMEM;
        size_t at = 0;
        for (int b = 0; b < nbatch && rc == ACG_OK; ++b) {
            const unsigned int n = (unsigned int)batch[b];
            if (pass_ms) pass_ms[b] = 0.f;
            if (!n) continue;
            lab.stage(in + at, n, false, true);
            const AcgReasmPass* rp = nullptr;
            if (lab.upload(n) != 0) rc = ACG_EHIP;
            if (rc == ACG_OK) rc = acg_rs_prepare(t, n, nullptr, nullptr, 0, &rp);
            if (rc == ACG_OK && pass_ms && hipEventRecord(ev0, nullptr) != hipSuccess) rc = ACG_EHIP;
            if (rc == ACG_OK) rc = acg_rs_launch(t, lab.d_in, n, &d, nullptr);
            if (rc == ACG_OK && pass_ms &&
                (hipEventRecord(ev1, nullptr) != hipSuccess || hipEventSynchronize(ev1) != hipSuccess || hipEventElapsedTime(&pass_ms[b], ev0, ev1) != hipSuccess))
                rc = ACG_EHIP;
            if (rc == ACG_OK) rc = acg_rs_fetch_status(t, nullptr, n, status + at, nullptr);
            at += n;
        }
        size_t nbytes = 0;
        if (rc == ACG_OK) rc = acg_rs_drain(t, nullptr, done, done_cap, ndone, text, text_cap, &nbytes, dropped);
    }
    acg_rs_destroy(t);
    if (ev0) hipEventDestroy(ev0);
    if (ev1) hipEventDestroy(ev1);
    return rc;
}

extern "C" int acg_lab_outputs_level_guard(acg_ctx* ctx, int leg, unsigned int* near_midpoint)
{
    if (!ctx || !near_midpoint) return ACG_EINVAL;
    return sink_level_guard(ctx, ctx->outs, OUTPUTS_OFF, leg, near_midpoint);
}

// The self test's own check, as acg_selftest_msg_labels has one: what the pass left on the device against what was handed out.
// The first n sorted keys are real and ascending, equal keys in input order, their records distinct ones of the `kept` the label
// pass kept; every table starts at 0, ascends strictly and ends at the leg's bytes; record i of the MSGS leg carries key i.
// ACG_ESTATE when the legs do not index alike.
static int outputs_aligned(const AcgOutputs* o, unsigned int n, const unsigned int* d_kept, const acg_out_buf* bufs)
{
    std::vector<unsigned long long> key(n);
    std::vector<unsigned int> idx(n);
    unsigned int kept = 0;
    if (hipMemcpy(&kept, d_kept, sizeof(kept), hipMemcpyDeviceToHost) != hipSuccess ||
        (n && (hipMemcpy(key.data(), o->d_key_s, (size_t)n * 8, hipMemcpyDeviceToHost) != hipSuccess ||
               hipMemcpy(idx.data(), o->d_idx_s, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess)))
        return ACG_EHIP;
    if (n > kept) return ACG_ESTATE;
    std::vector<bool> seen(kept, false);
    for (unsigned int i = 0; i < n; ++i) {
        if (key[i] == ~0ull || idx[i] >= kept || seen[idx[i]]) return ACG_ESTATE;
        if (i && (key[i] < key[i - 1] || (key[i] == key[i - 1] && idx[i] < idx[i - 1]))) return ACG_ESTATE;
        seen[idx[i]] = true;
    }
    for (int l = 0; l < o->cfg.nlegs; ++l) {
        if (o->leg[l].fmt) {
            const unsigned int* offs = bufs[l].offs;
            if (offs[0] != 0 || offs[n] != bufs[l].nbytes) return ACG_ESTATE;
            for (unsigned int i = 0; i < n; ++i)
                if (offs[i + 1] <= offs[i] || offs[i + 1] - offs[i] > o->leg[l].fmt->rec_max) return ACG_ESTATE;
        } else {
            const acg_msg* m = (const acg_msg*)bufs[l].out;
            for (unsigned int i = 0; i < n; ++i)
                if (key[i] != (((unsigned long long)(unsigned int)m[i].chn << 44) | (unsigned long long)m[i].end_bit)) return ACG_ESTATE;
        }
    }
    return ACG_OK;
}

extern "C" int acg_selftest_outputs(const acg_msg* in, int n, const acg_msg_filter* f, const acg_outputs_config* cfg, const int* Fr_hz, int nch,
                                    acg_out_buf* bufs, int* nrecs)
{
    if (n < 0 || (n > 0 && !in) || !outputs_config_ok(cfg) || nch < 1 || nch > (1 << 20) || !nrecs || (unsigned int)n > MAX_TAKE) return ACG_EINVAL;
    unsigned int got = 0;
    const int rc = outputs_selftest(in, n, f, cfg, Fr_hz, nch, bufs, true, &got, outputs_aligned);
    if (rc != ACG_EINVAL) *nrecs = rc == ACG_OK ? (int)got : 0;
    return rc;
}

// leg l of a configuration alone: what a sink of its own for that leg is configured with
static acg_outputs_config outputs_one_leg(const acg_outputs_config* c, int l)
{
    acg_outputs_config one = *c;
    std::memset(one.leg, 0, sizeof(one.leg));
    one.nlegs = 1;
    one.leg[0] = c->leg[l];
    return one;
}

// arm A: the JSON leg's pass and the text leg's pass, each an instance with an order of its own, what two separate fetches launch;
// arm B: the two legs' one pass.  ms[0 .. reps) A, ms[reps .. 2 reps) B
extern "C" int acg_lab_time_output_passes(const acg_msg* in, int n, const acg_outputs_config* cfg, int nch, int warmup, int reps, float* ms)
{
    if (n < 1 || !in || !outputs_config_ok(cfg) || cfg->nlegs != 2 || nch < 1 || nch > (1 << 20) || warmup < 0 || reps < 1 || !ms ||
        (unsigned int)n > MAX_TAKE || !sink_records_ok(in, n, nch))
        return ACG_EINVAL;
    const int jl = cfg->leg[0].kind == ACG_OUT_JSON ? 0 : 1, tl = 1 - jl;
    if (cfg->leg[jl].kind != ACG_OUT_JSON || !leg_is_text(cfg->leg[tl].kind)) return ACG_EINVAL;
    int ndev = 0;
    if (!acg_launch_outs || hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return ACG_ENODEV;
    const acg_outputs_config jc = outputs_one_leg(cfg, jl), tc = outputs_one_leg(cfg, tl);
    AcgOutputs* arm[2][2] = {};
    int rc = outputs_create(&arm[0][0], &jc, nullptr, nch);
    if (rc == ACG_OK) rc = outputs_create(&arm[0][1], &tc, nullptr, nch);
    if (rc == ACG_OK) rc = outputs_create(&arm[1][0], cfg, nullptr, nch);
    if (rc == ACG_OK) rc = time_passes(in, n, nch, warmup, reps, arm, ms);
    // faster and different is not faster: what the last round of arm B left on the device is what arm A left, leg by leg --
    // counters, offset table, bytes -- or the figures are refused (ACG_ESTATE)
    for (int a = 0; a < 2 && rc == ACG_OK; ++a) {
        const AcgOutputs *one = arm[0][a], *both = arm[1][0];
        const int l = a == 0 ? jl : tl;
        const AcgLeg &ga = one->leg[0], &gb = both->leg[l];
        unsigned int ca[2] = {0, 0}, cb[2] = {0, 0};
        if (hipMemcpy(ca, one->d_cnt, sizeof(ca), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(cb, both->d_cnt + 4 * l, sizeof(cb), hipMemcpyDeviceToHost) != hipSuccess) {
            rc = ACG_EHIP;
            break;
        }
        if (ca[0] != cb[0] || ca[1] != cb[1] || ca[1] > (unsigned int)n || (size_t)ca[0] > (size_t)n * ga.fmt->rec_max) {
            rc = ACG_ESTATE;
            break;
        }
        std::vector<unsigned char> ba(ca[0]), bb(ca[0]);
        std::vector<unsigned int> oa(ca[1]), ob(ca[1]);
        if ((ca[0] && (hipMemcpy(ba.data(), ga.d_out, ca[0], hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(bb.data(), gb.d_out, ca[0], hipMemcpyDeviceToHost) != hipSuccess)) ||
            (ca[1] && (hipMemcpy(oa.data(), ga.d_off, (size_t)ca[1] * 4, hipMemcpyDeviceToHost) != hipSuccess ||
                       hipMemcpy(ob.data(), gb.d_off, (size_t)ca[1] * 4, hipMemcpyDeviceToHost) != hipSuccess)))
            rc = ACG_EHIP;
        else if (ba != bb || oa != ob) rc = ACG_ESTATE;
    }
    outputs_destroy(arm[0][0]);
    outputs_destroy(arm[0][1]);
    outputs_destroy(arm[1][0]);
    return rc;
}
#endif
