// flights.cpp -- host side of the flight table (flight.hip): the table and its work space in device memory, grown on demand
// like the message staging of acg_api.cpp, the snapshot and the route hand-over.  Used by a context (acg_flights_enable) and,
// without one, by acg_selftest_flights.
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

void acg_fl_destroy(AcgFlights* t)
{
    if (!t) return;
    free_work(t);
    hipFree(t->p.slots); hipFree(t->p.st); hipFree(t->p.routes);
    hipFree(t->snap_key); hipFree(t->snap_val); hipFree(t->snap_out);
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

int acg_fl_prepare(AcgFlights* t, unsigned int n, void* stream, const AcgFlightPass** pass)
{
    hipStream_t s = (hipStream_t)stream;
    int rc = ensure_work(t, n, s);
    if (rc != ACG_OK) return rc;
    // a pass of n records queues at most n routes.  route_bound counts records, not routes: before the queue grows on its
    // account, ask the device how many routes it really holds (the stream is idle here: every entry point ends with a
    // synchronise), so a host that never drains pays for the routes it leaves queued, not for the records it has seen
    if (t->route_bound + n > t->p.route_cap) {
        unsigned int queued = 0;
        FLCHK(hipMemcpyAsync(&queued, &t->p.st->nroutes, sizeof(queued), hipMemcpyDeviceToHost, s));
        FLCHK(hipStreamSynchronize(s));
        t->route_bound = std::min(queued, t->p.route_cap);
    }
    if (t->route_bound + n > t->p.route_cap) {
        const size_t want = std::max<size_t>(2 * (size_t)t->p.route_cap, t->route_bound + n);
        AcgRouteRec* bigger = nullptr;
        FLCHK(hipMalloc(&bigger, want * sizeof(AcgRouteRec)));
        FLCHK(hipMemcpyAsync(bigger, t->p.routes, (size_t)t->p.route_cap * sizeof(AcgRouteRec), hipMemcpyDeviceToDevice, s));
        FLCHK(hipStreamSynchronize(s));
        hipFree(t->p.routes);
        t->p.routes = bigger;
        t->p.route_cap = (unsigned int)want;
    }
    t->route_bound += n;
    t->p.pass += 1;
    *pass = &t->p;
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
