// flights.cpp -- host side of the flight table (flight.hip): the table and its work space in device memory, grown on demand
// like the message staging of results.cpp, the snapshot and the route hand-over; the channel map, the export queue and the import
// queue of a table kept for the channels of several contexts.  Used by a context (acg_flights_enable) and, without one, by
// acg_selftest_flights and acg_selftest_flights_sharded.  Behind it, the same for the reassembly table (reasm.hip): AcgReasm.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <new>
#include <vector>

#include "acarsdec_amd.h"
#include "acg_internal.h"
#include "flights.h"

struct AcgFlights {
    AcgFlightPass p{};                  // configuration + device pointers, as the kernels take them
    size_t work_cap = 0;                // records the per-pass work space holds
    void* work = nullptr;               // one allocation behind p.ev ... p.segs
    unsigned long long* snap_key = nullptr;   // [2][cap] + values + records: the snapshot's work space
    unsigned int* snap_val = nullptr;
    unsigned char* snap_out = nullptr;
    size_t route_bound = 0;             // no more routes than this can be queued on the device
    std::deque<acg_route> pending;      // routes already fetched and ordered, not yet handed out
    // ---- the table's text (flight_text.hip), acg_fl_text_enable
    AcgFlightTextDev* d_tcfg = nullptr; // null: the renderer is off
    unsigned int* t_cnt = nullptr;      // [4]: bytes, records of the last pass; dropped; the route pass's lines
    void* m_work = nullptr;             // monitor: len, off [cap], wg_sum, wg_cnt, the frame
    unsigned int *m_len = nullptr, *m_wg = nullptr;
    unsigned char* m_out = nullptr;
    size_t m_out_cap = 0;
    void* r_work = nullptr;             // routes, grown on demand: keys, indices, len, off [r_cap], wg_sum, wg_cnt, the lines
    size_t r_cap = 0;
    // ---- one table for several contexts: this one exports its events (p.xq set) or takes in those of others
    int* d_chmap = nullptr;             // p.chmap, or null
    const int* d_ctxmap = nullptr;      // the context's map (not owned): p.chmap while d_chmap is null
    unsigned int n_ctxmap = 0;
    size_t xq_bound = 0;                // no more events than this can be queued for export
    std::deque<acg_flight_event> xpending;      // events already fetched, not yet handed out
    std::vector<acg_flight_event> imp_pending;  // imported, waiting for the next pass
    std::vector<acg_flight_event> imp_up;       // the upload of the last pass (alive until the stream has taken it)
    void* d_imp = nullptr;              // p.imp
    size_t imp_cap = 0;
};

#define FLCHK(call)                          \
    do {                                     \
        if ((call) != hipSuccess) return ACG_EHIP; \
    } while (0)

static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

static void free_work(AcgFlights* t)
{
    hipFree(t->work);
    t->work = nullptr;
    t->work_cap = 0;
}

static void free_text(AcgFlights* t)
{
    hipFree(t->d_tcfg); hipFree(t->t_cnt); hipFree(t->m_work); hipFree(t->r_work);
    t->d_tcfg = nullptr;
    t->t_cnt = nullptr;
    t->m_work = t->r_work = nullptr;
    t->r_cap = 0;
}

void acg_fl_destroy(AcgFlights* t)
{
    if (!t) return;
    free_work(t);
    free_text(t);
    hipFree(t->p.slots); hipFree(t->p.st); hipFree(t->p.routes);
    hipFree(t->snap_key); hipFree(t->snap_val); hipFree(t->snap_out);
    hipFree(t->d_chmap); hipFree(t->p.xq); hipFree(t->d_imp);
    delete t;
}

int acg_fl_reset(AcgFlights* t)
{
    AcgFlightState st{};
    st.G = LLONG_MIN;
    FLCHK(hipDeviceSynchronize());
    FLCHK(hipMemset(t->p.slots, 0, (size_t)t->p.cap * sizeof(AcgFlightSlot)));
    FLCHK(hipMemcpy(t->p.st, &st, sizeof(st), hipMemcpyHostToDevice));
    FLCHK(hipDeviceSynchronize());
    t->p.pass = 0;
    t->route_bound = 0;
    t->pending.clear();
    t->xq_bound = 0;                                                  // (the channel map and the export switch stay)
    t->xpending.clear();
    t->imp_pending.clear();
    t->p.n_import = 0;
    return ACG_OK;
}

int acg_fl_create(AcgFlights** out, const acg_flight_config* cfg)
{
    *out = nullptr;
    if (!acg_fl_config_ok(cfg)) return ACG_EINVAL;
    AcgFlights* t = new (std::nothrow) AcgFlights;
    if (!t) return ACG_ENOMEM;
    unsigned int cap = 1;
    while (cap < (unsigned int)cfg->max_flights) cap <<= 1;
    t->p.t0_sec = cfg->t0_sec;
    t->p.t0_usec = cfg->t0_usec;
    t->p.mdly = cfg->mdly;
    t->p.cap = cap;
    t->p.route_cap = 4096;
    const bool ok = hipMalloc(&t->p.slots, (size_t)cap * sizeof(AcgFlightSlot)) == hipSuccess &&
                    hipMalloc(&t->p.st, sizeof(AcgFlightState)) == hipSuccess &&
                    hipMalloc(&t->p.routes, (size_t)t->p.route_cap * sizeof(AcgRouteRec)) == hipSuccess &&
                    hipMalloc(&t->snap_key, (size_t)cap * 2 * sizeof(unsigned long long)) == hipSuccess &&
                    hipMalloc(&t->snap_val, (size_t)cap * 2 * sizeof(unsigned int)) == hipSuccess &&
                    hipMalloc(&t->snap_out, (size_t)cap * sizeof(acg_flight)) == hipSuccess;
    int rc = ok ? acg_fl_reset(t) : ACG_ENOMEM;
    if (rc != ACG_OK) {
        acg_fl_destroy(t);
        return rc;
    }
    *out = t;
    return ACG_OK;
}

// work space for n records
static int ensure_work(AcgFlights* t, unsigned int n, hipStream_t s)
{
    if (n <= t->work_cap) return ACG_OK;
    FLCHK(hipStreamSynchronize(s));                                   // an earlier pass may still use the old buffers
    free_work(t);
    const size_t want = std::max<size_t>(n, 4096);
    const size_t b_ev = up256(want * sizeof(AcgFlightEv)), b_64 = up256(want * 8), b_32 = up256(want * 4);
    FLCHK(hipMalloc(&t->work, b_ev + 6 * b_64 + 4 * b_32));
    unsigned char* w = (unsigned char*)t->work;
    t->p.ev = (AcgFlightEv*)w; w += b_ev;
    t->p.key1 = (unsigned long long*)w; w += b_64;
    t->p.key1s = (unsigned long long*)w; w += b_64;
    t->p.key2 = (unsigned long long*)w; w += b_64;
    t->p.key2s = (unsigned long long*)w; w += b_64;
    t->p.pmax = (long long*)w; w += b_64;
    t->p.segs = (uint2*)w; w += b_64;
    t->p.idx1 = (unsigned int*)w; w += b_32;
    t->p.idx1s = (unsigned int*)w; w += b_32;
    t->p.rank2 = (unsigned int*)w; w += b_32;
    t->p.rank2s = (unsigned int*)w; w += b_32;
    t->work_cap = want;
    return ACG_OK;
}

// Room for `n` more records in a device queue (the routes, the exported events) that is appended to through the counter *d_count.
// *bound counts records that MAY have been queued since the last drain, not records queued: before the queue grows on its account,
// ask the device how many it really holds (the stream is idle here: every entry point ends with a synchronise), so a host that
// never drains pays for what it leaves queued, not for the records it has seen
static int queue_room(void** q, unsigned int* cap, size_t rec, size_t* bound, const unsigned int* d_count, size_t n, hipStream_t s)
{
    if (*bound + n > *cap) {
        unsigned int queued = 0;
        FLCHK(hipMemcpyAsync(&queued, d_count, sizeof(queued), hipMemcpyDeviceToHost, s));
        FLCHK(hipStreamSynchronize(s));
        *bound = std::min(queued, *cap);
    }
    if (*bound + n > *cap) {
        const size_t want = std::max<size_t>(2 * (size_t)*cap, *bound + n);
        if (want > 0xffffffffull) return ACG_ENOMEM;
        void* bigger = nullptr;
        FLCHK(hipMalloc(&bigger, want * rec));
        FLCHK(hipMemcpyAsync(bigger, *q, (size_t)*cap * rec, hipMemcpyDeviceToDevice, s));
        FLCHK(hipStreamSynchronize(s));
        hipFree(*q);
        *q = bigger;
        *cap = (unsigned int)want;
    }
    *bound += n;
    return ACG_OK;
}

int acg_fl_prepare(AcgFlights* t, unsigned int n, void* stream, const AcgFlightPass** pass)
{
    hipStream_t s = (hipStream_t)stream;
    t->p.n_import = 0;
    if (t->p.xq) {                                                    // a peer: the pass ends behind the extraction, its events are queued
        int rc = ensure_work(t, n, s);
        if (rc == ACG_OK) rc = queue_room(&t->p.xq, &t->p.xq_cap, sizeof(acg_flight_event), &t->xq_bound, &t->p.st->nexport, n, s);
        if (rc != ACG_OK) return rc;
        t->p.pass += 1;
        *pass = &t->p;
        return ACG_OK;
    }
    // the owner of a shared table: the events imported since the last pass join this one
    const size_t n_imp = t->imp_pending.size(), tot = (size_t)n + n_imp;
    if (tot > (1u << 30)) return ACG_ENOMEM;
    int rc = ensure_work(t, (unsigned int)tot, s);
    if (rc != ACG_OK) return rc;
    if (n_imp) {
        if (n_imp > t->imp_cap) {
            FLCHK(hipStreamSynchronize(s));
            hipFree(t->d_imp);
            t->d_imp = nullptr;
            t->imp_cap = 0;
            const size_t want = std::max<size_t>(n_imp, 4096);
            FLCHK(hipMalloc(&t->d_imp, want * sizeof(acg_flight_event)));
            t->imp_cap = want;
        }
        t->imp_up.swap(t->imp_pending);                               // (the previous upload is long done: every entry point ends with a synchronise)
        t->imp_pending.clear();
        FLCHK(hipMemcpyAsync(t->d_imp, t->imp_up.data(), n_imp * sizeof(acg_flight_event), hipMemcpyHostToDevice, s));
        t->p.imp = t->d_imp;
        t->p.n_import = (unsigned int)n_imp;
    }
    // a pass of tot events queues at most tot routes
    void* rq = t->p.routes;
    rc = queue_room(&rq, &t->p.route_cap, sizeof(AcgRouteRec), &t->route_bound, &t->p.st->nroutes, tot, s);
    t->p.routes = (AcgRouteRec*)rq;
    if (rc != ACG_OK) return rc;
    t->p.pass += 1;
    *pass = &t->p;
    return ACG_OK;
}

// ---- one table for several contexts ----------------------------------------------------------------------------------------------
int acg_fl_set_channels(AcgFlights* t, const int* chn, int nch)
{
    FLCHK(hipDeviceSynchronize());
    hipFree(t->d_chmap);
    t->d_chmap = nullptr;
    t->p.chmap = t->d_ctxmap;                                         // no map of its own: the context's
    t->p.nmap = t->n_ctxmap;
    if (!chn || nch <= 0) return ACG_OK;
    FLCHK(hipMalloc(&t->d_chmap, (size_t)nch * sizeof(int)));
    FLCHK(hipMemcpy(t->d_chmap, chn, (size_t)nch * sizeof(int), hipMemcpyHostToDevice));
    t->p.chmap = t->d_chmap;
    t->p.nmap = (unsigned int)nch;
    return ACG_OK;
}

void acg_fl_context_channels(AcgFlights* t, const int* d_chn, unsigned int n)
{
    t->d_ctxmap = d_chn;
    t->n_ctxmap = d_chn ? n : 0;
    if (t->d_chmap) return;                                           // a map of its own keeps precedence
    t->p.chmap = t->d_ctxmap;
    t->p.nmap = t->n_ctxmap;
}

int acg_fl_exporting(const AcgFlights* t) { return t->p.xq != nullptr; }

int acg_fl_export(AcgFlights* t, int on)
{
    const int rc = acg_fl_reset(t);                                   // the table and both queues are emptied either way
    if (rc != ACG_OK) return rc;
    hipFree(t->p.xq);
    t->p.xq = nullptr;
    t->p.xq_cap = 0;
    if (!on) return ACG_OK;
    FLCHK(hipMalloc(&t->p.xq, 4096 * sizeof(acg_flight_event)));
    t->p.xq_cap = 4096;
    return ACG_OK;
}

int acg_fl_drain_events(AcgFlights* t, void* stream, acg_flight_event* out, int max, int* n)
{
    hipStream_t s = (hipStream_t)stream;
    unsigned int queued = 0;
    FLCHK(hipMemcpyAsync(&queued, &t->p.st->nexport, sizeof(queued), hipMemcpyDeviceToHost, s));
    FLCHK(hipStreamSynchronize(s));
    const unsigned int got = std::min(queued, t->p.xq_cap);
    if (got) {
        std::vector<acg_flight_event> h(got);
        FLCHK(hipMemcpyAsync(h.data(), t->p.xq, (size_t)got * sizeof(acg_flight_event), hipMemcpyDeviceToHost, s));
        FLCHK(hipMemsetAsync(&t->p.st->nexport, 0, sizeof(unsigned int), s));
        FLCHK(hipStreamSynchronize(s));
        t->xpending.insert(t->xpending.end(), h.begin(), h.end());
    }
    t->xq_bound = 0;
    int k = 0;
    while (k < max && !t->xpending.empty()) {
        out[k++] = t->xpending.front();
        t->xpending.pop_front();
    }
    *n = k;
    return t->xpending.empty() ? ACG_OK : ACG_EAGAIN;
}

int acg_fl_import(AcgFlights* t, const acg_flight_event* ev, int n)
{
    if (t->imp_pending.size() + (size_t)n > (1u << 30)) return ACG_ENOMEM;
    t->imp_pending.insert(t->imp_pending.end(), ev, ev + n);
    return ACG_OK;
}

int acg_fl_imports_queued(const AcgFlights* t) { return !t->imp_pending.empty(); }

int acg_fl_commit(AcgFlights* t, void* stream)
{
    if (t->imp_pending.empty()) return ACG_OK;
    const AcgFlightPass* fp = nullptr;
    const int rc = acg_fl_prepare(t, 0, stream, &fp);
    if (rc != ACG_OK) return rc;
    if (acg_launch_flight_pass(nullptr, 0, nullptr, fp, stream) != 0) return ACG_EHIP;
    FLCHK(hipStreamSynchronize((hipStream_t)stream));
    return ACG_OK;
}

int acg_fl_snapshot(AcgFlights* t, void* stream, acg_flight* out, int max, int* n, int* dropped)
{
    hipStream_t s = (hipStream_t)stream;
    const unsigned int cap = t->p.cap;
    if (acg_launch_flight_snapshot(&t->p, t->snap_key, t->snap_key + cap, t->snap_val, t->snap_val + cap, t->snap_out, stream) != 0) return ACG_EHIP;
    AcgFlightState st{};
    FLCHK(hipMemcpyAsync(&st, t->p.st, sizeof(st), hipMemcpyDeviceToHost, s));
    FLCHK(hipStreamSynchronize(s));
    if (st.nlive > cap) return ACG_EHIP;
    if (dropped) *dropped = (int)st.dropped;
    *n = (int)st.nlive;
    if ((int)st.nlive > max) return ACG_EAGAIN;
    if (st.nlive) {
        FLCHK(hipMemcpyAsync(out, t->snap_out, (size_t)st.nlive * sizeof(acg_flight), hipMemcpyDeviceToHost, s));
        FLCHK(hipStreamSynchronize(s));
    }
    return ACG_OK;
}

int acg_fl_drain_routes(AcgFlights* t, void* stream, acg_route* out, int max, int* n)
{
    hipStream_t s = (hipStream_t)stream;
    AcgFlightState st{};
    FLCHK(hipMemcpyAsync(&st, t->p.st, sizeof(st), hipMemcpyDeviceToHost, s));
    FLCHK(hipStreamSynchronize(s));
    const unsigned int got = std::min(st.nroutes, t->p.route_cap);
    if (got) {
        std::vector<AcgRouteRec> h(got);
        FLCHK(hipMemcpyAsync(h.data(), t->p.routes, (size_t)got * sizeof(AcgRouteRec), hipMemcpyDeviceToHost, s));
        FLCHK(hipMemsetAsync(&t->p.st->nroutes, 0, sizeof(unsigned int), s));
        FLCHK(hipStreamSynchronize(s));
        // the waves queued them in the order they got there: by (pass, rank of the triggering event) they are in the order of
        // their messages
        std::sort(h.begin(), h.end(), [](const AcgRouteRec& a, const AcgRouteRec& b) { return a.order < b.order; });
        for (const AcgRouteRec& r : h) {
            acg_route x;
            std::memcpy(&x, r.r, sizeof(x));
            t->pending.push_back(x);
        }
    }
    t->route_bound = 0;
    int k = 0;
    while (k < max && !t->pending.empty()) {
        out[k++] = t->pending.front();
        t->pending.pop_front();
    }
    *n = k;
    return t->pending.empty() ? ACG_OK : ACG_EAGAIN;
}

// ---- the table's text (flight_text.hip) ---------------------------------------------------------------------------------------
static size_t wg_words(size_t n) { return n / 256 + 1; }

int acg_fl_text_on(const AcgFlights* t) { return t->d_tcfg != nullptr; }

int acg_fl_text_enable(AcgFlights* t, const AcgFlightTextDev* cfg)
{
    FLCHK(hipDeviceSynchronize());
    free_text(t);
    if (!cfg) return ACG_OK;
    // the monitor's work space is sized like the snapshot's: for every slot of the table
    const size_t cap = t->p.cap, b_32 = up256(cap * 4), b_wg = up256(wg_words(cap) * 4);
    t->m_out_cap = ACG_FT_HDR_LEN + cap * ACG_FT_ROW_MAX;
    if (t->m_out_cap > 0xffffffffull) return ACG_EINVAL;             // (cannot happen: 2^24 slots of 78 bytes)
    if (hipMalloc(&t->d_tcfg, sizeof(*cfg)) != hipSuccess || hipMalloc(&t->t_cnt, 4 * sizeof(unsigned int)) != hipSuccess ||
        hipMalloc(&t->m_work, 2 * b_32 + 2 * b_wg + up256(t->m_out_cap + 16)) != hipSuccess) {
        free_text(t);
        return ACG_ENOMEM;
    }
    unsigned char* w = (unsigned char*)t->m_work;
    t->m_len = (unsigned int*)w; w += 2 * b_32;
    t->m_wg = (unsigned int*)w; w += 2 * b_wg;
    t->m_out = w;
    if (hipMemcpy(t->d_tcfg, cfg, sizeof(*cfg), hipMemcpyHostToDevice) != hipSuccess || hipMemset(t->t_cnt, 0, 4 * sizeof(unsigned int)) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        free_text(t);
        return ACG_EHIP;
    }
    return ACG_OK;
}

static AcgFlightTextPass text_pass(const AcgFlights* t)
{
    AcgFlightTextPass q;
    std::memset(&q, 0, sizeof(q));
    q.cfg = t->d_tcfg;
    q.t0_sec = t->p.t0_sec;
    q.t0_usec = t->p.t0_usec;
    q.slots = t->p.slots;
    q.st = t->p.st;
    q.routes = t->p.routes;
    q.counters = t->t_cnt;
    return q;
}

int acg_fl_monitor_text(AcgFlights* t, void* stream, long long hdr_soh, char* out, size_t cap, size_t* nbytes, int* nrows, int* dropped)
{
    if (!t->d_tcfg) return ACG_ESTATE;
    hipStream_t s = (hipStream_t)stream;
    const unsigned int slots = t->p.cap;
    if (acg_launch_flight_snapkeys(&t->p, t->snap_key, t->snap_key + slots, t->snap_val, t->snap_val + slots, stream) != 0) return ACG_EHIP;
    AcgFlightTextPass q = text_pass(t);
    q.hdr_soh = hdr_soh;
    q.total = &t->p.st->nlive;
    q.nmax = slots;
    q.base = ACG_FT_HDR_LEN;
    q.idx_s = t->snap_val + slots;
    q.len = t->m_len; q.off = t->m_len + up256((size_t)slots * 4) / 4;
    q.wg_sum = t->m_wg; q.wg_cnt = t->m_wg + up256(wg_words(slots) * 4) / 4;
    q.out = t->m_out;
    q.out_cap = (unsigned int)t->m_out_cap;
    if (acg_launch_flight_monitor_text(&q, stream) != 0) return ACG_EHIP;
    unsigned int cnt[4] = {0, 0, 0, 0};
    FLCHK(hipMemcpyAsync(cnt, t->t_cnt, sizeof(cnt), hipMemcpyDeviceToHost, s));
    FLCHK(hipStreamSynchronize(s));
    if (cnt[1] > slots || (size_t)cnt[0] > (size_t)cnt[1] * ACG_FT_ROW_MAX) return ACG_EHIP;
    *nbytes = (size_t)ACG_FT_HDR_LEN + cnt[0];
    *nrows = (int)cnt[1];
    if (dropped) *dropped = (int)cnt[2];
    if (*nbytes > cap) return ACG_EAGAIN;
    FLCHK(hipMemcpyAsync(out, t->m_out, *nbytes, hipMemcpyDeviceToHost, s));
    FLCHK(hipStreamSynchronize(s));
    return ACG_OK;
}

// work space for the lines of n routes
static int ensure_route_text(AcgFlights* t, size_t n, hipStream_t s)
{
    if (n <= t->r_cap) return ACG_OK;
    FLCHK(hipStreamSynchronize(s));
    hipFree(t->r_work);
    t->r_work = nullptr;
    t->r_cap = 0;
    const size_t want = std::max<size_t>(n, 1024);
    FLCHK(hipMalloc(&t->r_work, 2 * up256(want * 8) + 4 * up256(want * 4) + 2 * up256(wg_words(want) * 4) + up256(want * ACG_FT_LINE_MAX + 16)));
    t->r_cap = want;
    return ACG_OK;
}

int acg_fl_routes_json(AcgFlights* t, void* stream, char* out, size_t cap, size_t* nbytes, int* nlines)
{
    if (!t->d_tcfg || !t->pending.empty()) return ACG_ESTATE;
    hipStream_t s = (hipStream_t)stream;
    unsigned int queued = 0;
    FLCHK(hipMemcpyAsync(&queued, &t->p.st->nroutes, sizeof(queued), hipMemcpyDeviceToHost, s));
    FLCHK(hipStreamSynchronize(s));
    const unsigned int got = std::min(queued, t->p.route_cap);
    *nbytes = 0;
    *nlines = 0;
    if (!got) {
        t->route_bound = 0;
        return ACG_OK;
    }
    if ((size_t)got * ACG_FT_LINE_MAX > 0xffffffffull) return ACG_ENOMEM;
    const int rc = ensure_route_text(t, got, s);
    if (rc != ACG_OK) return rc;
    const size_t b_64 = up256(t->r_cap * 8), b_32 = up256(t->r_cap * 4), b_wg = up256(wg_words(t->r_cap) * 4);
    unsigned char* w = (unsigned char*)t->r_work;
    AcgFlightTextPass q = text_pass(t);
    q.total = t->t_cnt + 3;
    q.nmax = got;
    q.key = (unsigned long long*)w; w += b_64;
    q.key_s = (unsigned long long*)w; w += b_64;
    q.idx = (unsigned int*)w; w += b_32;
    q.idx_s = (unsigned int*)w; w += b_32;
    q.len = (unsigned int*)w; w += b_32;
    q.off = (unsigned int*)w; w += b_32;
    q.wg_sum = (unsigned int*)w; w += b_wg;
    q.wg_cnt = (unsigned int*)w; w += b_wg;
    q.out = w;
    q.out_cap = (unsigned int)((size_t)got * ACG_FT_LINE_MAX);
    if (acg_launch_flight_route_text(&q, got, stream) != 0) return ACG_EHIP;
    unsigned int cnt[4] = {0, 0, 0, 0};
    FLCHK(hipMemcpyAsync(cnt, t->t_cnt, sizeof(cnt), hipMemcpyDeviceToHost, s));
    FLCHK(hipStreamSynchronize(s));
    if (cnt[1] != got || cnt[0] > q.out_cap) return ACG_EHIP;       // (every route has a line)
    *nbytes = cnt[0];
    *nlines = (int)cnt[1];
    if (cnt[0] > cap) return ACG_EAGAIN;                             // nothing consumed
    FLCHK(hipMemcpyAsync(out, q.out, cnt[0], hipMemcpyDeviceToHost, s));
    FLCHK(hipMemsetAsync(&t->p.st->nroutes, 0, sizeof(unsigned int), s));
    FLCHK(hipStreamSynchronize(s));
    t->route_bound = 0;
    return ACG_OK;
}

// a C string of at most n bytes as a word, NUL padded
static unsigned long long str_word(const char* src, size_t n)
{
    unsigned long long v = 0;
    for (size_t i = 0; i < n && src[i]; ++i) v |= (unsigned long long)(unsigned char)src[i] << (8 * i);
    return v;
}

int acg_fl_load_designed(AcgFlights* t, const acg_flight* in, int n, const acg_route* rt, int nr)
{
    if (n < 0 || nr < 0 || (unsigned int)n > t->p.cap) return ACG_EINVAL;
    int rc = acg_fl_reset(t);
    if (rc != ACG_OK) return rc;
    std::vector<AcgFlightSlot> slots((size_t)n);
    for (int i = 0; i < n; ++i) {
        AcgFlightSlot& S = slots[(size_t)i];
        const acg_flight& f = in[i];
        std::memset(&S, 0, sizeof(S));
        S.key = str_word(f.addr, 7) | (1ull << 63);
        S.seq = (unsigned long long)(n - i);                          // in[0]: the latest update
        S.fid = str_word(f.fid, 7);
        S.chm = f.chm;
        S.ts_sample = f.ts_sample; S.tl_sample = f.tl_sample; S.ts_sec = f.ts_sec; S.tl_sec = f.tl_sec;
        S.ts_usec = f.ts_usec; S.tl_usec = f.tl_usec; S.first_chn = f.first_chn; S.last_chn = f.last_chn;
        S.nbm = f.nbm;
        S.rt = f.rt ? 1u : 0u;
        const char* fl[7] = {f.da, f.sa, f.eta, f.gout, f.gin, f.woff, f.won};
        for (int k = 0; k < 7; ++k) S.fld[k] = (unsigned int)str_word(fl[k], 4);
    }
    if (n) FLCHK(hipMemcpy(t->p.slots, slots.data(), (size_t)n * sizeof(AcgFlightSlot), hipMemcpyHostToDevice));   // (G = LLONG_MIN: all live)
    if ((unsigned int)nr > t->p.route_cap) {
        AcgRouteRec* bigger = nullptr;
        FLCHK(hipMalloc(&bigger, (size_t)nr * sizeof(AcgRouteRec)));
        hipFree(t->p.routes);
        t->p.routes = bigger;
        t->p.route_cap = (unsigned int)nr;
    }
    if (nr) {
        // stored in a shuffled order (a fixed linear congruential walk), tagged (pass, rank) ascending with the index
        std::vector<unsigned int> at((size_t)nr);
        for (int i = 0; i < nr; ++i) at[(size_t)i] = (unsigned int)i;
        unsigned long long x = 0x9e3779b97f4a7c15ull;
        for (int i = nr - 1; i > 0; --i) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            std::swap(at[(size_t)i], at[(size_t)((x >> 33) % (unsigned long long)(i + 1))]);
        }
        std::vector<AcgRouteRec> h((size_t)nr);
        for (int i = 0; i < nr; ++i) {
            AcgRouteRec& R = h[at[(size_t)i]];
            R.order = ((unsigned long long)(i / 7 + 1) << 32) | (unsigned long long)(i % 7);
            std::memcpy(R.r, rt + i, sizeof(R.r));
        }
        const unsigned int cnt = (unsigned int)nr;
        FLCHK(hipMemcpy(t->p.routes, h.data(), (size_t)nr * sizeof(AcgRouteRec), hipMemcpyHostToDevice));
        FLCHK(hipMemcpy(&t->p.st->nroutes, &cnt, sizeof(cnt), hipMemcpyHostToDevice));
    }
    FLCHK(hipDeviceSynchronize());
    t->route_bound = (size_t)nr;
    return ACG_OK;
}

// ---- the reassembly table (reasm.hip): the table, its rows and work space in device memory, the two queues of completed messages
// (fixed records; texts, each on a 16-byte boundary) grown on demand like the route queue, and their hand-over in final order ----
struct AcgReasm {
    AcgReasmPass p{};
    size_t work_cap = 0;                // records the per-pass work space holds
    void* work = nullptr;               // one allocation behind p.ev ... p.keep
    size_t done_bound = 0;              // no more completed records than this can be queued on the device ...
    unsigned long long text_bound = 0;  // ... and no more bytes of text
    unsigned long long in_table = 0;    // no more bytes than this lie in the table's rows
    std::vector<acg_reasm_msg> pending; // fetched and ordered, not yet handed out: [pend_head, size), text_off into pend_text
    std::vector<char> pend_text;
    size_t pend_head = 0;
};

void acg_rs_destroy(AcgReasm* t)
{
    if (!t) return;
    hipFree(t->work);
    hipFree(t->p.slots); hipFree(t->p.rows); hipFree(t->p.st); hipFree(t->p.done); hipFree(t->p.texts);
    delete t;
}

int acg_rs_reset(AcgReasm* t)
{
    AcgReasmState st{};
    st.G = st.Gnext = LLONG_MIN;
    FLCHK(hipDeviceSynchronize());
    FLCHK(hipMemset(t->p.slots, 0, (size_t)t->p.cap * sizeof(AcgReasmSlot)));
    FLCHK(hipMemcpy(t->p.st, &st, sizeof(st), hipMemcpyHostToDevice));
    FLCHK(hipDeviceSynchronize());
    t->p.pass = 0;
    t->done_bound = 0;
    t->text_bound = t->in_table = 0;
    t->pending.clear();
    t->pend_text.clear();
    t->pend_head = 0;
    return ACG_OK;
}

int acg_rs_create(AcgReasm** out, const acg_reasm_config* cfg)
{
    *out = nullptr;
    acg_reasm_config c;
    if (!acg_rs_config_ok(cfg, &c)) return ACG_EINVAL;
    AcgReasm* t = new (std::nothrow) AcgReasm;
    if (!t) return ACG_ENOMEM;
    unsigned int cap = 1;
    while (cap < (unsigned int)c.max_msgs) cap <<= 1;
    t->p.t0_us = c.t0_sec * 1000000ll + c.t0_usec;
    t->p.cap = cap;
    t->p.max_text = (unsigned int)c.max_text;
    t->p.done_cap = 1024;
    t->p.text_cap = (unsigned long long)std::max(c.max_text, 1 << 18);
    const bool ok = hipMalloc(&t->p.slots, (size_t)cap * sizeof(AcgReasmSlot)) == hipSuccess &&
                    hipMalloc(&t->p.rows, (size_t)cap * (size_t)c.max_text) == hipSuccess && hipMalloc(&t->p.st, sizeof(AcgReasmState)) == hipSuccess &&
                    hipMalloc(&t->p.done, (size_t)t->p.done_cap * sizeof(AcgReasmDone)) == hipSuccess &&
                    hipMalloc(&t->p.texts, (size_t)t->p.text_cap) == hipSuccess;
    const int rc = ok ? acg_rs_reset(t) : ACG_ENOMEM;
    if (rc != ACG_OK) {
        acg_rs_destroy(t);
        return rc;
    }
    *out = t;
    return ACG_OK;
}

int acg_rs_prepare(AcgReasm* t, unsigned int n, void* stream, const int* chmap, unsigned int nmap, const AcgReasmPass** pass)
{
    hipStream_t s = (hipStream_t)stream;
    if (n > (1u << 30)) return ACG_ENOMEM;
    if (n > t->work_cap) {
        FLCHK(hipStreamSynchronize(s));                               // an earlier pass may still use the old buffers
        hipFree(t->work);
        t->work = nullptr;
        t->work_cap = 0;
        const size_t want = std::max<size_t>(n, 4096);
        const size_t b_ev = up256(want * sizeof(AcgReasmEv)), b_64 = up256(want * 8), b_32 = up256(want * 4);
        FLCHK(hipMalloc(&t->work, b_ev + 3 * b_64 + 3 * b_32 + up256(want)));
        unsigned char* w = (unsigned char*)t->work;
        t->p.ev = (AcgReasmEv*)w; w += b_ev;
        t->p.ka = (unsigned long long*)w; w += b_64;
        t->p.kb = (unsigned long long*)w; w += b_64;
        t->p.segs = (uint2*)w; w += b_64;
        t->p.va = (unsigned int*)w; w += b_32;
        t->p.vb = (unsigned int*)w; w += b_32;
        t->p.status = (unsigned int*)w; w += b_32;
        t->p.keep = w;
        t->work_cap = want;
    }
    // a pass of n records completes at most n messages ...
    void* dq = t->p.done;
    int rc = queue_room(&dq, &t->p.done_cap, sizeof(AcgReasmDone), &t->done_bound, &t->p.st->ndone, n, s);
    t->p.done = (AcgReasmDone*)dq;
    if (rc != ACG_OK) return rc;
    // ... whose texts hold what lay in the rows and what the pass appends (242 bytes a record), each rounded up to 16 bytes
    const unsigned long long row = t->p.max_text;
    t->in_table = std::min<unsigned long long>(t->in_table + 242ull * n, row * t->p.cap);
    const unsigned long long need = std::min<unsigned long long>(row * n, t->in_table + 16ull * n);
    if (t->text_bound + need > t->p.text_cap) {                        // as queue_room: what is really queued, before the queue grows
        unsigned long long queued = 0;
        FLCHK(hipMemcpyAsync(&queued, &t->p.st->tbytes, sizeof(queued), hipMemcpyDeviceToHost, s));
        FLCHK(hipStreamSynchronize(s));
        t->text_bound = std::min(queued, t->p.text_cap);
    }
    if (t->text_bound + need > t->p.text_cap) {
        const unsigned long long want = std::max(2 * t->p.text_cap, t->text_bound + need);
        if (want > (1ull << 40)) return ACG_ENOMEM;
        void* bigger = nullptr;
        FLCHK(hipMalloc(&bigger, (size_t)want));
        FLCHK(hipMemcpyAsync(bigger, t->p.texts, (size_t)t->text_bound, hipMemcpyDeviceToDevice, s));
        FLCHK(hipStreamSynchronize(s));
        hipFree(t->p.texts);
        t->p.texts = (unsigned char*)bigger;
        t->p.text_cap = want;
    }
    t->text_bound += need;
    t->p.chmap = chmap;
    t->p.nmap = chmap ? nmap : 0;
    t->p.pass += 1;
    *pass = &t->p;
    return ACG_OK;
}

int acg_rs_launch(AcgReasm* t, const AcgMsgRec* recs, unsigned int n, const AcgLabelFilter* f, void* stream)
{
    return acg_launch_reasm_pass(recs, n, f, &t->p, stream) == 0 ? ACG_OK : ACG_EHIP;
}

int acg_rs_fetch_status(AcgReasm* t, void* stream, unsigned int n, unsigned char* status, unsigned char* keep)
{
    hipStream_t s = (hipStream_t)stream;
    if (n > t->work_cap) return ACG_ESTATE;
    std::vector<unsigned int> w(n);
    if (n) FLCHK(hipMemcpyAsync(w.data(), t->p.status, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (n && keep) FLCHK(hipMemcpyAsync(keep, t->p.keep, n, hipMemcpyDeviceToHost, s));
    FLCHK(hipStreamSynchronize(s));
    for (unsigned int i = 0; i < n; ++i) status[i] = (unsigned char)w[i];
    return ACG_OK;
}

int acg_rs_drain(AcgReasm* t, void* stream, acg_reasm_msg* out, int max, int* n, char* text, size_t cap, size_t* nbytes, int* dropped)
{
    hipStream_t s = (hipStream_t)stream;
    AcgReasmState st{};
    FLCHK(hipMemcpyAsync(&st, t->p.st, sizeof(st), hipMemcpyDeviceToHost, s));
    FLCHK(hipStreamSynchronize(s));
    if (st.qfull || st.ndone > t->p.done_cap || st.tbytes > t->p.text_cap) return ACG_EHIP;     // (the queues are sized so that this cannot happen)
    if (dropped) *dropped = (int)st.dropped;
    if (t->pend_head == t->pending.size()) {                          // everything fetched earlier has been handed out
        t->pending.clear();
        t->pend_text.clear();
        t->pend_head = 0;
    }
    if (st.ndone) {
        std::vector<AcgReasmDone> h(st.ndone);
        const size_t t0 = t->pend_text.size();
        t->pend_text.resize(t0 + (size_t)st.tbytes);
        FLCHK(hipMemcpyAsync(h.data(), t->p.done, (size_t)st.ndone * sizeof(AcgReasmDone), hipMemcpyDeviceToHost, s));
        if (st.tbytes) FLCHK(hipMemcpyAsync(t->pend_text.data() + t0, t->p.texts, (size_t)st.tbytes, hipMemcpyDeviceToHost, s));
        FLCHK(hipMemsetAsync(&t->p.st->ndone, 0, sizeof(unsigned int), s));
        FLCHK(hipMemsetAsync(&t->p.st->tbytes, 0, sizeof(unsigned long long), s));
        FLCHK(hipStreamSynchronize(s));
        // the waves queued them in the order they got there: by (pass, time key of the final fragment) they are in the order of
        // their final fragments
        std::sort(h.begin(), h.end(), [](const AcgReasmDone& a, const AcgReasmDone& b) { return a.pass != b.pass ? a.pass < b.pass : a.tkey < b.tkey; });
        for (const AcgReasmDone& d : h) {
            acg_reasm_msg x;
            std::memcpy(&x, d.r, sizeof(x));
            if (x.text_off + x.text_len > st.tbytes) return ACG_EHIP;
            x.text_off += t0;
            t->pending.push_back(x);
        }
    }
    t->done_bound = 0;
    t->text_bound = 0;
    int k = 0;
    size_t used = 0;
    while (k < max && t->pend_head < t->pending.size() && used + t->pending[t->pend_head].text_len <= cap) {
        const acg_reasm_msg& x = t->pending[t->pend_head++];
        out[k] = x;
        out[k].text_off = used;
        if (x.text_len) std::memcpy(text + used, t->pend_text.data() + x.text_off, x.text_len);
        used += x.text_len;
        ++k;
    }
    *n = k;
    *nbytes = used;
    return t->pend_head == t->pending.size() ? ACG_OK : ACG_EAGAIN;
}
