// lab.cpp -- the self tests that need no context (label pass, flight table, sin/cos, division), the stamp build's read-out,
// the probes and the generators.
#include <chrono>

#include "acg_ctx.h"

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
