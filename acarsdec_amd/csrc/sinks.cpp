// sinks.cpp -- the batch sinks' host runtime: JSON, text and the flight table's text, their configuration, entry points, level
// guards and self tests; and the outputs, several legs rendered from one take (outs.hip), at the end.
#include <climits>

#include "acg_ctx.h"

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
    bool borrows = false;                   // a leg of the outputs: d_cnt and the four order arrays are AcgOutputs' own, shared by its legs
};

static void sink_free_work(AcgSinkState* st)
{
    if (!st->borrows) { hipFree(st->d_key); hipFree(st->d_key_s); hipFree(st->d_idx); hipFree(st->d_idx_s); }
    hipFree(st->d_len); hipFree(st->d_off);
    hipFree(st->d_wg); hipFree(st->d_out);
    st->d_key = st->d_key_s = nullptr;
    st->d_idx = st->d_idx_s = st->d_len = st->d_off = st->d_wg = nullptr;
    st->d_out = nullptr;
    st->cap = 0;
}

void sink_destroy(AcgSinkState* st)
{
    if (!st) return;
    sink_free_work(st);
    hipFree(st->d_cfg); hipFree(st->d_freq);
    if (!st->borrows) hipFree(st->d_cnt);
    delete st;
}

// what a format renders once on the host
struct SinkBlob {
    int rc = ACG_OK;                        // ACG_EINVAL: a stretch does not fit (cannot happen); sink_create hands it on
    std::vector<unsigned char> cfg, freq;
};

// ACG_OK, ACG_ENOMEM or ACG_EHIP (or the blob's own verdict).  cnt: a leg of the outputs counts in its four words of their block
static int sink_create(AcgSinkState** out, const AcgSinkFormat* fmt, const SinkBlob& blob, unsigned int* cnt = nullptr)
{
    if (blob.rc != ACG_OK) return blob.rc;
    AcgSinkState* st = new (std::nothrow) AcgSinkState();
    if (!st) return ACG_ENOMEM;
    st->fmt = fmt;
    st->borrows = cnt != nullptr;
    st->d_cnt = cnt;
    if (hipMalloc(&st->d_cfg, blob.cfg.size()) != hipSuccess || hipMalloc(&st->d_freq, blob.freq.size()) != hipSuccess ||
        (!cnt && hipMalloc(&st->d_cnt, 4 * sizeof(unsigned int)) != hipSuccess)) {
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

// work space and output buffer for n records, grown on demand as d_kmsgs is.  order: a leg of the outputs takes their order
// arrays (they hold as many records as it asks for) and allocates only what is its own
static int sink_reserve(AcgSinkState* st, size_t n, const AcgSinkState* order = nullptr)
{
    if (n <= st->cap) return ACG_OK;
    sink_free_work(st);
    const size_t want = std::max<size_t>(n, 4096);
    if (order) {
        st->d_key = order->d_key; st->d_key_s = order->d_key_s;
        st->d_idx = order->d_idx; st->d_idx_s = order->d_idx_s;
    }
    if ((!order && (hipMalloc(&st->d_key, want * 8) != hipSuccess || hipMalloc(&st->d_key_s, want * 8) != hipSuccess ||
                    hipMalloc(&st->d_idx, want * 4) != hipSuccess || hipMalloc(&st->d_idx_s, want * 4) != hipSuccess)) ||
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

// the outputs (acg_outputs_enable): up to ACG_OUT_LEGS_MAX legs over one order.  `order` is a sink state without a format: it owns
// the four order arrays and ONE block of counters, four words per leg, which the rendered legs' states borrow (st[l]->borrows);
// the MSGS leg has no state, only the packed arrays outs.hip's gather fills and word 1 of its four counters.
struct AcgOutputs {
    acg_outputs_config cfg{};
    AcgSinkState order;
    AcgSinkState* st[ACG_OUT_LEGS_MAX] = {};    // JSON and text legs; null: the MSGS leg
    int msgs_leg = -1;
    AcgMsgRec* d_gmsgs = nullptr;               // order.cap records each
    acg_oooi* d_goooi = nullptr;
};
static const char* const OUTPUTS_OFF = "outputs are off: acg_outputs_enable first";

static const AcgSinkState* outputs_order(const AcgOutputs* o) { return o ? &o->order : nullptr; }

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
    unsigned int pending = 0, take = 0;
    RingSpan span;
    int rc = ring_upto(ctx, lag, &span);
    if (rc != ACG_OK) return rc;
    if (!span.any) return commit_imports(ctx);
    rc = ring_claim(ctx, span, (int)fit, &pending, &take);
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
    if (!ctx || !n || max < 0 || (max > 0 && !keys) || (sink != ACG_SINK_JSON && sink != ACG_SINK_TEXT && sink != ACG_SINK_OUTPUTS)) return ACG_EINVAL;
    *n = 0;
    const AcgSinkState* st = sink == ACG_SINK_JSON ? ctx->json : sink == ACG_SINK_TEXT ? ctx->text : outputs_order(ctx->outs);
    if (!st) return fail(ctx, ACG_ESTATE, sink == ACG_SINK_JSON ? SINK_JSON.is_off : sink == ACG_SINK_TEXT ? SINK_TEXT.is_off : OUTPUTS_OFF);
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

// ---- the outputs: one take, ordered once, every leg rendered from it (outs.hip) --------------------------------------------------
static_assert(ACG_OUT_MSGS > ACG_TEXT_SV && ACG_OUT_JSON > ACG_TEXT_SV && ACG_OUT_MSGS != ACG_OUT_JSON, "leg kinds are distinct");

static bool leg_is_text(int kind) { return kind >= ACG_TEXT_ONELINE && kind <= ACG_TEXT_SV; }

static const AcgSinkFormat* leg_format(int kind) { return kind == ACG_OUT_JSON ? &SINK_JSON : leg_is_text(kind) ? &SINK_TEXT : nullptr; }

static size_t leg_rec_max(int kind) { return kind == ACG_OUT_MSGS ? sizeof(acg_msg) : leg_format(kind)->rec_max; }

// the configuration as the JSON sink's and as leg l's text sink's: what json_config_ok / text_config_ok check and the blobs render
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

static void outputs_free_work(AcgOutputs* o)
{
    for (AcgSinkState* st : o->st)
        if (st) sink_free_work(st);
    sink_free_work(&o->order);
    hipFree(o->d_gmsgs); hipFree(o->d_goooi);
    o->d_gmsgs = nullptr;
    o->d_goooi = nullptr;
}

void outputs_destroy(AcgOutputs* o)
{
    if (!o) return;
    outputs_free_work(o);
    for (AcgSinkState* st : o->st) sink_destroy(st);
    hipFree(o->order.d_cnt);
    delete o;
}

// cfg has passed outputs_config_ok.  ACG_OK, ACG_ENOMEM or ACG_EHIP
static int outputs_create(AcgOutputs** out, const acg_outputs_config* cfg, const int* Fr_hz, int nch)
{
    AcgOutputs* o = new (std::nothrow) AcgOutputs();
    if (!o) return ACG_ENOMEM;
    o->cfg = *cfg;
    int rc = ACG_OK;
    if (hipMalloc(&o->order.d_cnt, 4 * ACG_OUT_LEGS_MAX * sizeof(unsigned int)) != hipSuccess) rc = ACG_ENOMEM;
    else if (hipMemset(o->order.d_cnt, 0, 4 * ACG_OUT_LEGS_MAX * sizeof(unsigned int)) != hipSuccess) rc = ACG_EHIP;
    for (int l = 0; l < cfg->nlegs && rc == ACG_OK; ++l) {
        const int kind = cfg->leg[l].kind;
        if (kind == ACG_OUT_MSGS) {
            o->msgs_leg = l;
        } else if (kind == ACG_OUT_JSON) {
            const acg_json_config j = outputs_json_config(cfg);
            rc = sink_create(&o->st[l], &SINK_JSON, json_blob(&j, Fr_hz, nch), o->order.d_cnt + 4 * l);
        } else {
            const acg_text_config t = outputs_text_config(cfg, l);
            rc = sink_create(&o->st[l], &SINK_TEXT, text_blob(&t, Fr_hz, nch), o->order.d_cnt + 4 * l);
        }
    }
    if (rc != ACG_OK) {
        outputs_destroy(o);
        return rc == ACG_EHIP ? rc : ACG_ENOMEM;
    }
    *out = o;
    return ACG_OK;
}

// work space of every leg for n records, grown on demand: the order arrays first, the legs borrow them
static int outputs_reserve(AcgOutputs* o, size_t n)
{
    if (n <= o->order.cap) return ACG_OK;
    outputs_free_work(o);
    const size_t want = std::max<size_t>(n, 4096);
    AcgSinkState* od = &o->order;
    bool ok = hipMalloc(&od->d_key, want * 8) == hipSuccess && hipMalloc(&od->d_key_s, want * 8) == hipSuccess &&
              hipMalloc(&od->d_idx, want * 4) == hipSuccess && hipMalloc(&od->d_idx_s, want * 4) == hipSuccess;
    if (ok && o->msgs_leg >= 0)
        ok = hipMalloc(&o->d_gmsgs, want * sizeof(AcgMsgRec)) == hipSuccess && hipMalloc(&o->d_goooi, want * sizeof(acg_oooi)) == hipSuccess;
    for (int l = 0; l < o->cfg.nlegs && ok; ++l)
        if (o->st[l]) ok = sink_reserve(o->st[l], want, od) == ACG_OK;
    if (!ok) {
        outputs_free_work(o);
        return ACG_ENOMEM;
    }
    od->cap = want;
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
    p.order.key = o->order.d_key; p.order.key_s = o->order.d_key_s;
    p.order.idx = o->order.d_idx; p.order.idx_s = o->order.d_idx_s;
    p.order.chmap = chmap;
    p.order.nmap = nmap;
    for (int l = 0; l < o->cfg.nlegs; ++l) {
        if (!o->st[l]) continue;
        AcgSinkPass& sp = p.leg[p.nrender];
        sp = sink_pass(o->st[l], recs, oooi, total, nmax, lvl_from_rec);
        sp.chmap = chmap;
        sp.nmap = nmap;
        p.is_json[p.nrender++] = o->st[l]->fmt == &SINK_JSON;
    }
    if (o->msgs_leg >= 0) {
        p.g_recs = o->d_gmsgs;
        p.g_oooi = (unsigned char*)o->d_goooi;
        p.g_count = o->order.d_cnt + 4 * o->msgs_leg + 1;
    }
    return p;
}

// the MSGS leg's records as they came from the device, turned into what fetch_msgs hands out, in place (lab: the level is the
// record's own, as the lab entries of the sinks take it)
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
// and a sync.  take: the records the pass ran over.  lab: a leg that does not fit says ACG_EAGAIN with every leg's nbytes set
// and nothing written (a fetch has sized the take so that everything fits).  ACG_EHIP with *what set, ACG_EAGAIN or ACG_OK.
static int outputs_hand_out(const AcgOutputs* o, hipStream_t stream, unsigned int take, acg_out_buf* bufs, const std::vector<int>* chnum, bool lab,
                            unsigned int* nrecs, const char** what)
{
    unsigned int cnt[4 * ACG_OUT_LEGS_MAX] = {};
    *what = "outputs: copy failed";
    if (hipMemcpyAsync(cnt, o->order.d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return ACG_EHIP;
    const unsigned int n = cnt[1];                                // (leg 0's records: every leg counts in word 1 of its four)
    bool fits = true;
    for (int l = 0; l < o->cfg.nlegs; ++l) {
        const unsigned int c0 = cnt[4 * l], c1 = cnt[4 * l + 1];
        *what = "outputs pass: counts out of range";
        if (c1 > take || (o->st[l] && (size_t)c0 > (size_t)take * o->st[l]->fmt->rec_max)) return ACG_EHIP;
        *what = "outputs pass: the legs disagree on the number of records";
        if (c1 != n) return ACG_EHIP;
        bufs[l].nbytes = o->st[l] ? (size_t)c0 : (size_t)c1 * sizeof(acg_msg);
        if (bufs[l].nbytes > bufs[l].cap) fits = false;
    }
    *what = "outputs pass: counts out of range";
    if (!fits) return lab ? ACG_EAGAIN : ACG_EHIP;
    *what = "outputs: copy failed";
    for (int l = 0; l < o->cfg.nlegs && n; ++l) {                 // (kept records sort in front of dropped ones: the first n of everything)
        if (o->st[l]) {
            if (hipMemcpyAsync(bufs[l].out, o->st[l]->d_out, bufs[l].nbytes, hipMemcpyDeviceToHost, stream) != hipSuccess ||
                hipMemcpyAsync(bufs[l].offs, o->st[l]->d_off, (size_t)n * sizeof(unsigned int), hipMemcpyDeviceToHost, stream) != hipSuccess)
                return ACG_EHIP;
        } else if (hipMemcpyAsync(bufs[l].out, o->d_gmsgs, (size_t)n * sizeof(AcgMsgRec), hipMemcpyDeviceToHost, stream) != hipSuccess ||
                   hipMemcpyAsync(bufs[l].oooi, o->d_goooi, (size_t)n * sizeof(acg_oooi), hipMemcpyDeviceToHost, stream) != hipSuccess) {
            return ACG_EHIP;
        }
    }
    if (n && hipStreamSynchronize(stream) != hipSuccess) return ACG_EHIP;
    for (int l = 0; l < o->cfg.nlegs; ++l) {
        if (o->st[l]) bufs[l].offs[n] = (unsigned int)bufs[l].nbytes;
        else outputs_finish_msgs((acg_msg*)bufs[l].out, n, chnum, lab);
    }
    *nrecs = n;
    *what = nullptr;
    return ACG_OK;
}

// the caller's buffers against the legs: everything a leg writes to is there.  min_cap: what a leg must hold at least
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

extern "C" int acg_outputs_enable(acg_ctx* ctx, const acg_outputs_config* cfg, const int* Fr_hz)
{
    if (!ctx) return ACG_EINVAL;
    if (cfg && !outputs_config_ok(cfg))
        return fail(ctx, ACG_EINVAL, "outputs: 1 .. ACG_OUT_LEGS_MAX legs of pairwise distinct known kinds, a flag the kind does not take, t0 outside [10^9, 4 * 10^9) s / 0..999999 us, or an unterminated string");
    if (hipSetDevice(ctx->cfg.device) != hipSuccess || (ctx->outs && hipStreamSynchronize(ctx->copy_stream) != hipSuccess))
        return fail(ctx, ACG_EHIP, "outputs: the device does not answer");
    if (ctx->outs) {
        outputs_destroy(ctx->outs);
        ctx->outs = nullptr;
    }
    if (!cfg) return ACG_OK;
    if (!acg_launch_outs || !acg_launch_json || !acg_launch_text) return fail(ctx, ACG_ESTATE, "outputs: not in this build");
    if (!ctx->d_crctab) return fail(ctx, ACG_ESTATE, "outputs: context created without ACG_F_REPAIR");
    if (ctx->cfg.nch > (1 << 20)) return fail(ctx, ACG_EINVAL, "outputs: more than 2^20 channels");
    const int rc = outputs_create(&ctx->outs, cfg, Fr_hz, ctx->cfg.nch);
    return rc == ACG_OK ? rc : fail(ctx, rc, "outputs: allocation failed");
}

// sink_fetch's sibling: the same claim, split, label pass, flight pass and statistics, ONCE; then outs.hip's passes for every leg on
// the same stream, and the two round trips of a single sink fetch.  A block yields at most one record of at most recmax bytes per
// leg: the oldest min(max_recs, min over legs of cap / recmax) always fit every leg.
static int outputs_fetch(acg_ctx* ctx, int lag, acg_out_buf* bufs, int max_recs, int* nrecs)
{
    if (!ctx->d_crctab) return fail(ctx, ACG_ESTATE, "context created without ACG_F_REPAIR");
    AcgOutputs* o = ctx->outs;
    if (!o) return fail(ctx, ACG_ESTATE, OUTPUTS_OFF);
    if (max_recs < 1 || !outputs_bufs_ok(&o->cfg, bufs, true))
        return fail(ctx, ACG_EINVAL, "outputs: a leg's buffer holds less than one record, a buffer or table is missing, or max_recs < 1");
    o->order.last_nrecs = 0;
    size_t fit = (size_t)max_recs;
    for (int l = 0; l < o->cfg.nlegs; ++l) {
        fit = std::min(fit, bufs[l].cap / leg_rec_max(o->cfg.leg[l].kind));
        if (o->st[l]) fit = std::min<size_t>(fit, o->st[l]->fmt->max_take);
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
    if (outputs_reserve(o, take) != ACG_OK) return fail(ctx, ACG_ENOMEM, "outputs: work space");
    unsigned int* d_total = nullptr;
    if (const int lr = launch_split(ctx, take, true, &d_total)) return lr;
    // the map in force at hand-out (acg_set_channel_numbers)
    const AcgOutsPass op = outputs_pass(o, ctx->d_kmsgs, ctx->d_oooi, d_total, take, false, ctx->d_chnum, ctx->d_chnum ? (unsigned int)ctx->cfg.nch : 0u);
    if (acg_launch_outs(&op, ctx->copy_stream) != 0) return fail(ctx, ACG_EHIP, "outputs pass launch failed");
    unsigned int n = 0;
    const char* what = nullptr;
    if (const int hr = outputs_hand_out(o, ctx->copy_stream, take, bufs, &ctx->chnum, false, &n, &what)) return fail(ctx, hr, what);
    ctx->consumed += take;
    o->order.last_nrecs = n;
    *nrecs = (int)n;
    return ring_result(ctx, rc, pending, take, "more messages queued than fit: call again");
}

extern "C" int acg_collect_outputs(acg_ctx* ctx, int lag, acg_out_buf* bufs, int max_recs, int* nrecs)
{
    if (!ctx || !nrecs || lag < 0 || lag >= acg_ctx::NCALL - 1) return ACG_EINVAL;
    *nrecs = 0;
    return outputs_fetch(ctx, lag, bufs, max_recs, nrecs);
}

extern "C" int acg_drain_outputs(acg_ctx* ctx, acg_out_buf* bufs, int max_recs, int* nrecs)
{
    if (!ctx || !nrecs) return ACG_EINVAL;
    *nrecs = 0;
    return outputs_fetch(ctx, DRAIN, bufs, max_recs, nrecs);
}

// The outputs' three lab entries are compiled into the lab library only (this unit sees ACG_LAB: _build.SEES): the product library
// is held below 0.82 of the lab library's size (tests/test_host_logic.py; LEDGER, "Combined outputs"), and exports the three
// names as functions that say ACG_ESTATE.
#ifndef ACG_LAB
extern "C" int acg_lab_outputs_level_guard(acg_ctx*, int, unsigned int*) { return ACG_ESTATE; }

extern "C" int acg_selftest_outputs(const acg_msg*, int, const acg_msg_filter*, const acg_outputs_config*, const int*, int, acg_out_buf*, int*) { return ACG_ESTATE; }

extern "C" int acg_lab_time_output_passes(const acg_msg*, int, const acg_outputs_config*, int, int, int, float*) { return ACG_ESTATE; }
#else
extern "C" int acg_lab_outputs_level_guard(acg_ctx* ctx, int leg, unsigned int* near_midpoint)
{
    if (!ctx || !near_midpoint) return ACG_EINVAL;
    *near_midpoint = 0;
    if (!ctx->outs) return fail(ctx, ACG_ESTATE, OUTPUTS_OFF);
    if (leg < 0 || leg >= ctx->outs->cfg.nlegs || !ctx->outs->st[leg]) return fail(ctx, ACG_EINVAL, "outputs: not a JSON or text leg");
    return sink_level_guard(ctx, ctx->outs->st[leg]->fmt, ctx->outs->st[leg], near_midpoint);
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
        (n && (hipMemcpy(key.data(), o->order.d_key_s, (size_t)n * 8, hipMemcpyDeviceToHost) != hipSuccess ||
               hipMemcpy(idx.data(), o->order.d_idx_s, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess)))
        return ACG_EHIP;
    if (n > kept) return ACG_ESTATE;
    std::vector<bool> seen(kept, false);
    for (unsigned int i = 0; i < n; ++i) {
        if (key[i] == ~0ull || idx[i] >= kept || seen[idx[i]]) return ACG_ESTATE;
        if (i && (key[i] < key[i - 1] || (key[i] == key[i - 1] && idx[i] < idx[i - 1]))) return ACG_ESTATE;
        seen[idx[i]] = true;
    }
    for (int l = 0; l < o->cfg.nlegs; ++l) {
        if (o->st[l]) {
            const unsigned int* offs = bufs[l].offs;
            if (offs[0] != 0 || offs[n] != bufs[l].nbytes) return ACG_ESTATE;
            for (unsigned int i = 0; i < n; ++i)
                if (offs[i + 1] <= offs[i] || offs[i + 1] - offs[i] > o->st[l]->fmt->rec_max) return ACG_ESTATE;
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
    AcgLabelFilter d;
    if (n < 0 || (n > 0 && !in) || !outputs_config_ok(cfg) || nch < 1 || nch > (1 << 20) || !nrecs ||
        (unsigned int)n > std::min(SINK_JSON.max_take, SINK_TEXT.max_take) || label_filter_dev(f, &d) != ACG_OK || !sink_records_ok(in, n, nch) ||
        !outputs_bufs_ok(cfg, bufs, false))
        return ACG_EINVAL;
    *nrecs = 0;
    if (n == 0) return ACG_OK;
    int ndev = 0;
    if (!acg_launch_outs || !acg_launch_json || !acg_launch_text || hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return ACG_ENODEV;
    AcgOutputs* o = nullptr;
    int rc = outputs_create(&o, cfg, Fr_hz, nch);
    if (rc != ACG_OK) return rc;
    rc = outputs_reserve(o, (size_t)n);
    if (rc == ACG_OK) {
        LabStage lab((size_t)n);
        lab.stage(in, (unsigned int)n, true, true);
        const AcgOutsPass op = outputs_pass(o, lab.d_out, lab.d_oooi, lab.d_total(), (unsigned int)n, true, nullptr, 0u);
        unsigned int got = 0;
        const char* what = nullptr;
        if (!lab.ok()) rc = ACG_ENOMEM;
        else if (lab.label((unsigned int)n, &d) != 0 || acg_launch_outs(&op, nullptr) != 0) rc = ACG_EHIP;
        else rc = outputs_hand_out(o, nullptr, (unsigned int)n, bufs, nullptr, true, &got, &what);
        if (rc == ACG_OK) rc = outputs_aligned(o, got, lab.d_total(), bufs);
        if (rc == ACG_OK) *nrecs = (int)got;
    }
    outputs_destroy(o);
    return rc;
}

extern "C" int acg_lab_time_output_passes(const acg_msg* in, int n, const acg_outputs_config* cfg, int nch, int warmup, int reps, float* ms)
{
    if (n < 1 || !in || !outputs_config_ok(cfg) || cfg->nlegs != 2 || nch < 1 || nch > (1 << 20) || warmup < 0 || reps < 1 || !ms ||
        (unsigned int)n > std::min(SINK_JSON.max_take, SINK_TEXT.max_take) || !sink_records_ok(in, n, nch))
        return ACG_EINVAL;
    const int jl = cfg->leg[0].kind == ACG_OUT_JSON ? 0 : 1, tl = 1 - jl;
    if (cfg->leg[jl].kind != ACG_OUT_JSON || !leg_is_text(cfg->leg[tl].kind)) return ACG_EINVAL;
    int ndev = 0;
    if (!acg_launch_outs || !acg_launch_json || !acg_launch_text || hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return ACG_ENODEV;
    AcgSinkState* st[2] = {nullptr, nullptr};                      // arm A: the JSON sink and the text sink, each with an order of its own
    AcgOutputs* o = nullptr;                                       // arm B
    AcgLabelFilter none;
    std::memset(&none, 0, sizeof(none));
    hipEvent_t ev[2] = {nullptr, nullptr};
    int* d_map = nullptr;
    const acg_json_config j = outputs_json_config(cfg);
    const acg_text_config t = outputs_text_config(cfg, tl);
    int rc = sink_create(&st[0], &SINK_JSON, json_blob(&j, nullptr, nch));
    if (rc == ACG_OK) rc = sink_create(&st[1], &SINK_TEXT, text_blob(&t, nullptr, nch));
    if (rc == ACG_OK) rc = sink_reserve(st[0], (size_t)n);
    if (rc == ACG_OK) rc = sink_reserve(st[1], (size_t)n);
    if (rc == ACG_OK) rc = outputs_create(&o, cfg, nullptr, nch);
    if (rc == ACG_OK) rc = outputs_reserve(o, (size_t)n);
    if (rc == ACG_OK) {
        LabStage lab((size_t)n);
        lab.stage(in, (unsigned int)n, true, true);
        if (!lab.ok()) rc = ACG_ENOMEM;
        if (rc == ACG_OK && (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess)) rc = ACG_EHIP;
        if (rc == ACG_OK && (lab.label((unsigned int)n, &none) != 0 || hipDeviceSynchronize() != hipSuccess)) rc = ACG_EHIP;
        if (rc == ACG_OK && acg_tune_get("ACG_SINK_MAP", 0)) {    // both arms under a channel map (slot l -> nch - 1 - l), as acg_lab_time_sink_passes
            std::vector<int> m((size_t)nch);
            for (int l = 0; l < nch; ++l) m[(size_t)l] = nch - 1 - l;
            if (hipMalloc(&d_map, m.size() * sizeof(int)) != hipSuccess || hipMemcpy(d_map, m.data(), m.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
                rc = ACG_EHIP;
        }
        const unsigned int nmap = d_map ? (unsigned int)nch : 0u;
        AcgSinkPass spj = sink_pass(st[0], lab.d_out, lab.d_oooi, lab.d_total(), (unsigned int)n, true);
        AcgSinkPass spt = sink_pass(st[1], lab.d_out, lab.d_oooi, lab.d_total(), (unsigned int)n, true);
        spj.chmap = spt.chmap = d_map;
        spj.nmap = spt.nmap = nmap;
        const AcgOutsPass op = outputs_pass(o, lab.d_out, lab.d_oooi, lab.d_total(), (unsigned int)n, true, d_map, nmap);
        for (int r = -warmup; r < reps && rc == ACG_OK; ++r)
            for (int arm = 0; arm < 2 && rc == ACG_OK; ++arm) {
                float el = 0.0f;
                if (hipEventRecord(ev[0], nullptr) != hipSuccess ||
                    (arm == 0 ? (acg_launch_json(&spj, nullptr) != 0 || acg_launch_text(&spt, nullptr) != 0) : acg_launch_outs(&op, nullptr) != 0) ||
                    hipEventRecord(ev[1], nullptr) != hipSuccess || hipEventSynchronize(ev[1]) != hipSuccess ||
                    hipEventElapsedTime(&el, ev[0], ev[1]) != hipSuccess)
                    rc = ACG_EHIP;
                else if (r >= 0) ms[arm * reps + r] = el;
            }
        // faster and different is not faster: what the last round of arm B left on the device is what arm A left, leg by leg --
        // counters, offset table, bytes -- or the figures are refused (ACG_ESTATE)
        for (int a = 0; a < 2 && rc == ACG_OK; ++a) {
            const AcgSinkState* one = st[a];
            const AcgSinkState* leg = o->st[a == 0 ? jl : tl];
            unsigned int ca[2] = {0, 0}, cb[2] = {0, 0};
            if (hipMemcpy(ca, one->d_cnt, sizeof(ca), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(cb, leg->d_cnt, sizeof(cb), hipMemcpyDeviceToHost) != hipSuccess) {
                rc = ACG_EHIP;
                break;
            }
            if (ca[0] != cb[0] || ca[1] != cb[1] || ca[1] > (unsigned int)n || (size_t)ca[0] > (size_t)n * one->fmt->rec_max) {
                rc = ACG_ESTATE;
                break;
            }
            std::vector<unsigned char> ba(ca[0]), bb(ca[0]);
            std::vector<unsigned int> oa(ca[1]), ob(ca[1]);
            if ((ca[0] && (hipMemcpy(ba.data(), one->d_out, ca[0], hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(bb.data(), leg->d_out, ca[0], hipMemcpyDeviceToHost) != hipSuccess)) ||
                (ca[1] && (hipMemcpy(oa.data(), one->d_off, (size_t)ca[1] * 4, hipMemcpyDeviceToHost) != hipSuccess ||
                           hipMemcpy(ob.data(), leg->d_off, (size_t)ca[1] * 4, hipMemcpyDeviceToHost) != hipSuccess)))
                rc = ACG_EHIP;
            else if (ba != bb || oa != ob) rc = ACG_ESTATE;
        }
    }
    if (ev[0]) hipEventDestroy(ev[0]);
    if (ev[1]) hipEventDestroy(ev[1]);
    hipFree(d_map);
    sink_destroy(st[0]);
    sink_destroy(st[1]);
    outputs_destroy(o);
    return rc;
}
#endif
