// flights.h -- the flight table's host object (flights.cpp), shared by acg_api.cpp's entry points and the self test.
// The functions are WEAK references: the host runtime (acg_api.cpp) is also linked without the device units and without
// flights.cpp (the sanitizer build of tests/test_host_logic.py, which stubs the launchers it knows); there the table is simply
// absent, acg_flights_enable says ACG_ESTATE and nothing else is reachable.  flights.cpp includes this header too, so its
// definitions are emitted weak as well: intended and harmless, there is one definition of each in the library.
#pragma once
#include "acarsdec_amd.h"
#include "acg_internal.h"

struct AcgFlights;
#define ACG_FL_WEAK __attribute__((weak))
static inline int acg_fl_config_ok(const acg_flight_config* cfg)
{
    return cfg && cfg->mdly >= 1 && cfg->max_flights >= 1 && cfg->max_flights <= (1 << 24) && cfg->t0_usec >= 0 && cfg->t0_usec <= 999999;
}
ACG_FL_WEAK int acg_fl_create(AcgFlights** out, const acg_flight_config* cfg);     // an empty table on the current device
ACG_FL_WEAK void acg_fl_destroy(AcgFlights* t);
ACG_FL_WEAK int acg_fl_reset(AcgFlights* t);                                       // empties table, counters and pending routes (synchronises)
// before a pass over n records on `stream`: grows the work space and the route queue, numbers the pass; *pass goes to
// AcgLabelPass::flights
ACG_FL_WEAK int acg_fl_prepare(AcgFlights* t, unsigned int n, void* stream, const AcgFlightPass** pass);
ACG_FL_WEAK int acg_fl_snapshot(AcgFlights* t, void* stream, acg_flight* out, int max, int* n, int* dropped);
ACG_FL_WEAK int acg_fl_drain_routes(AcgFlights* t, void* stream, acg_route* out, int max, int* n);
// ---- one table for several contexts (acg_flights_set_channels / _export / _import of the public header)
// the number recorded for local channel l: chn[nch], null = identity (the values are checked by the caller); synchronises
ACG_FL_WEAK int acg_fl_set_channels(AcgFlights* t, const int* chn, int nch);
// the context's own map (acg_set_channel_numbers): a device array the CONTEXT owns, null / 0 = identity.  The table follows it while
// acg_fl_set_channels has given it none of its own; the caller has made sure no pass is in flight
ACG_FL_WEAK void acg_fl_context_channels(AcgFlights* t, const int* d_chn, unsigned int n);
// on: acg_fl_prepare's passes end behind the extraction and queue their events for acg_fl_drain_events.  Either way the table
// and both event queues are emptied (acg_fl_reset, which keeps the switch and the channel map)
ACG_FL_WEAK int acg_fl_export(AcgFlights* t, int on);
ACG_FL_WEAK int acg_fl_exporting(const AcgFlights* t);
ACG_FL_WEAK int acg_fl_drain_events(AcgFlights* t, void* stream, acg_flight_event* out, int max, int* n);
// n checked events for the next acg_fl_prepare, whose pass then covers its n records and these (AcgFlightPass::n_import)
ACG_FL_WEAK int acg_fl_import(AcgFlights* t, const acg_flight_event* ev, int n);
ACG_FL_WEAK int acg_fl_imports_queued(const AcgFlights* t);
// the pass over the queued imports alone, on `stream`, waited for; nothing queued: nothing happens
ACG_FL_WEAK int acg_fl_commit(AcgFlights* t, void* stream);
// ---- the table's text (flight_text.hip).  cfg: nbch and the escaped station stretch (null: the renderer off and its buffers freed)
ACG_FL_WEAK int acg_fl_text_enable(AcgFlights* t, const AcgFlightTextDev* cfg);
ACG_FL_WEAK int acg_fl_text_on(const AcgFlights* t);
// all or nothing, ACG_EAGAIN with *nbytes needed; the renderer must be on
ACG_FL_WEAK int acg_fl_monitor_text(AcgFlights* t, void* stream, long long hdr_soh, char* out, size_t cap, size_t* nbytes, int* nrows, int* dropped);
ACG_FL_WEAK int acg_fl_routes_json(AcgFlights* t, void* stream, char* out, size_t cap, size_t* nbytes, int* nlines);   // ACG_ESTATE: routes pending on the host
// lab: the table's content replaced by n designed entries (in[0] the latest update; cap >= n) and nr designed routes
ACG_FL_WEAK int acg_fl_load_designed(AcgFlights* t, const acg_flight* in, int n, const acg_route* rt, int nr);

// ---- the reassembly table's host object (flights.cpp; reasm.hip), the same way: weak references, absent without flights.cpp
struct AcgReasm;
// the configuration with its defaults filled in (max_msgs 0 = 1024, max_text 0 = 3584); 0: a value out of range
static inline int acg_rs_config_ok(const acg_reasm_config* cfg, acg_reasm_config* eff)
{
    if (!cfg) return 0;
    *eff = *cfg;
    if (eff->max_msgs == 0) eff->max_msgs = 1024;
    if (eff->max_text == 0) eff->max_text = 3584;
    return eff->t0_usec >= 0 && eff->t0_usec <= 999999 && eff->max_msgs >= 1 && eff->max_msgs <= (1 << 20) && eff->max_text >= 16 &&
           eff->max_text <= 65536 && eff->max_text % 16 == 0;
}
ACG_FL_WEAK int acg_rs_create(AcgReasm** out, const acg_reasm_config* cfg);         // an empty table on the current device
ACG_FL_WEAK void acg_rs_destroy(AcgReasm* t);
ACG_FL_WEAK int acg_rs_reset(AcgReasm* t);                                           // empties table, queues and pending messages (synchronises)
// before a pass over n records on `stream`: grows the work space and the two queues, numbers the pass.  chmap / nmap: the channel
// numbers recorded (a device array the caller owns, null = the slots' own)
ACG_FL_WEAK int acg_rs_prepare(AcgReasm* t, unsigned int n, void* stream, const int* chmap, unsigned int nmap, const AcgReasmPass** pass);
// the pass itself over recs[n] (device), behind acg_rs_prepare
ACG_FL_WEAK int acg_rs_launch(AcgReasm* t, const AcgMsgRec* recs, unsigned int n, const AcgLabelFilter* f, void* stream);
// the last pass's statuses (and with `keep` the label pass's decisions: AcgReasmPass::keep) of its n records; waits for the stream
ACG_FL_WEAK int acg_rs_fetch_status(AcgReasm* t, void* stream, unsigned int n, unsigned char* status, unsigned char* keep);
ACG_FL_WEAK int acg_rs_drain(AcgReasm* t, void* stream, acg_reasm_msg* out, int max, int* n, char* text, size_t cap, size_t* nbytes, int* dropped);
