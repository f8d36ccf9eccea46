// sinks.cpp -- the batch sinks' host runtime: JSON, text and the flight table's text, their configuration, entry points, level
// guards and self tests.
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

void sink_destroy(AcgSinkState* st)
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
