/*
 * acarsdec_amd_lab.h -- measurement and diagnostic entry points of libacarsdec_amd.so.  NOT product API: nothing here has a
 * counterpart in the reference, and a host that decodes ACARS needs none of it.  bench.py, the GPU tests and the probes under
 * profiles/probe/ use it: tuning switches for same-process A/B, timing trials, bandwidth probes, self tests of the device
 * arithmetic, device-side generators of synthetic input, and the test hooks that move the block counters next to their wrap and the
 * stream counters to where days of uptime put them.
 * Everything is exported by the product library as well (bench.py times the product), except where noted.
 */
#ifndef ACARSDEC_AMD_LAB_H
#define ACARSDEC_AMD_LAB_H

#include "acarsdec_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Measurement / layout switches (ACG_PIPE_BLOCKS, ACG_MSK_LPC, ACG_FIR_WAVES_PER_WG, ...: profiles/LEDGER.md).  A production
 * process has none and pays one atomic load per look-up.  This call sets one (value NULL removes it).  The environment is
 * read ONCE per process, at the library's first look-up, and only if ACG_ALLOW_TUNING=1 is set too (otherwise stray ACG_*
 * variables are named on stderr and ignored).  The measurement-only kernel variants and debug shapes exist only in the lab
 * build of the library (libacarsdec_amd_lab.so, which tests and probes load; it always takes the environment).
 * Not product configuration. */
int  acg_tune(const char *name, const char *value);
int  acg_is_lab_build(void);
/* Diagnostic: times a context on a sample of the caller's input.  Runs one untimed and `repeats` timed acg_process_iq_u8_dev
 * calls back to back (host clock around a device sync), reports the mean in *ms_per_call, and returns the context to its reset
 * state (acg_reset: channel state, queues).  Rounds 2-3 used it to pick the fastest of several contexts; round 4 found that
 * contexts timed for >= 0.25 s of streaming calls agree to 2 % and that what a short trial sees between them is mostly the
 * trial (profiles/LEDGER.md): a host creates ONE context per device and uses it.  The reference has no counterpart. */
int  acg_placement_trial(acg_ctx *ctx, const uint8_t *iq_dev, size_t pitch_bytes, int nblocks, int repeats,
			 void *hip_stream, double *ms_per_call);

/* the same for the acg_process_samples_dev formats (declared below) */
int  acg_placement_trial_samples(acg_ctx *ctx, int fmt, const void *dev, size_t pitch_bytes, size_t plane_bytes, int nblocks,
				 int repeats, void *hip_stream, double *ms_per_call);

/* device-side generator for large synthetic workloads: fills [nstreams] rows with seeded
 * uniform bytes */
int  acg_fill_random_u8_dev(uint8_t *dev, size_t pitch_bytes, int nrows, size_t row_bytes,
			    uint64_t seed, void *hip_stream);

/* measurement aid: a pure streaming reader (non-temporal 16-byte loads, nothing else) over `bytes` of
 * device memory, `repeats` back-to-back launches timed with HIP events on the default stream: the read
 * bandwidth this GPU delivers to a kernel that only reads.  Synchronises. */
int  acg_probe_read_dev(const void *dev, size_t bytes, int repeats, double *gb_per_s);

/* measurement aid: `repeats` synchronous host-to-device copies of `bytes` (after one for nothing), host clock: the rate
 * the *_host entry points can at best be fed at from that host memory (pinned or pageable) */
int  acg_probe_h2d(void *dev, const void *host, size_t bytes, int repeats, double *gb_per_s);

/* device-side AM up-converter: row r = scale*env[env_index[r]][n/decim] *
 * exp(j(2*pi*off_hz[r]*n/(12500*decim) + phase[r])) + N(0, noise_sigma^2), quantised like an RTL
 * dongle (u8 = clip(rint(127.37 + 127.5 x))).  All pointers are device pointers. */
int  acg_synth_iq_u8_dev(uint8_t *iq_dev, size_t pitch_bytes, int nrows, int nout, int decim,
			 const float *env_dev, size_t env_pitch_floats, const int *env_index_dev,
			 const float *off_hz_dev, const float *phase_dev, float scale, float noise_sigma,
			 uint64_t seed, void *hip_stream);
/* diagnostics: the device sin/cos used by the mixer (msk.c:90 calls cexp), evaluated on the GPU
 * for n host arguments in [0, 2*pi) -- lets a test bound its error against libm */
int  acg_selftest_sincos(const double *x_host, double *sin_host, double *cos_host, int n);
/* diagnostics: the loop's f64 divisions and square root as the device computes them (msk.c:103,110-111: shared
 * reciprocal, no exponent scaling) next to the compiler's IEEE forms, for n host triples:
 * out[8i..8i+7] = {n0/d, n1/d (shared reciprocal), n0/d, n1/d (IEEE), sqrt(x), sqrt(x) (IEEE), n0/d (single), x}
 * with x = n0^2 + n1^2 -- a test checks the pairs are bit-identical over the operand range the loop produces */
int  acg_selftest_div2(const double *n0_host, const double *n1_host, const double *d_host, double *out_host, int n);

/* diagnostics: the batch sink's filter / label-decoding / compaction pass (label.hip) on n caller-supplied records, taken as
 * acg_drain_msgs hands them out (every record counts as kept by the block repair).  keep[i] = 1 when the filter f (NULL = none)
 * keeps in[i]; oooi[i] = its decoded labels when kept, all zero when dropped.  Bytes of in[i].txt at or past txt_len (clamped to
 * 0..ACG_MSGTXTMAX) read as 0; label[2] is not read.  Returns ACG_ESTATE when the compacted records are not the kept inputs,
 * byte for byte and in order, ACG_EINVAL for a bad filter or n < 0. */
int  acg_selftest_msg_labels(const acg_msg *in, int n, const acg_msg_filter *f, unsigned char *keep, acg_oooi *oooi);

/* diagnostics: the flight table (flight.hip) on caller-supplied records, without a demodulator.  in holds sum(batch[0..nbatch))
 * records as acg_drain_msgs hands them out; batch b is taken through one pass (filter f, NULL = none; order (end_sample, chn)
 * within the batch) of a table made from cfg.  After batch b, snap_n[b] entries of the snapshot are appended to snaps (snap_cap
 * records in all); the routes of all batches go to routes (route_cap records), *nroutes of them; *dropped as acg_flight_snapshot.
 * ACG_EAGAIN: snaps or routes too small; ACG_ENODEV: no GPU. */
int  acg_selftest_flights(const acg_msg *in, const int *batch, int nbatch, const acg_flight_config *cfg, const acg_msg_filter *f,
			  acg_flight *snaps, int snap_cap, int *snap_n, acg_route *routes, int route_cap, int *nroutes, int *dropped);
/* diagnostics: the same records through nshards (1 .. 64) tables, driven as a host that shards its channels `c mod nshards` over
 * as many contexts drives them (acg_flights_set_channels / _export / _import of the product header).  in[i].chn is the GLOBAL
 * channel (0 .. 2^20 - 1): shard r = chn % nshards holds it as local channel chn / nshards under the map l -> l * nshards + r.
 * Shards 1 .. export, shard 0 owns the table.  Batch b is one ROUND: each peer's pass over its records and the drain of its events,
 * their import at the owner, then the owner's pass over its records and the imports -- the pass over the imports alone
 * (acg_flights_commit's) when the round has no record of the owner's.  snaps, snap_n, routes, *nroutes are the OWNER's, as
 * acg_selftest_flights fills them; dropped[b] (nbatch entries) is its `dropped` after round b.  pass_ms (nbatch entries, or NULL):
 * the device time of the owner's part of round b in milliseconds, HIP events around the upload of the imported events, the label
 * pass and the flight pass (the way of the owner's records to the device is outside).
 * ACG_ESTATE: a peer's table or route queue is not empty at the end, or it exported an event acg_flight_events_check refuses. */
int  acg_selftest_flights_sharded(const acg_msg *in, const int *batch, int nbatch, int nshards, const acg_flight_config *cfg,
				  const acg_msg_filter *f, acg_flight *snaps, int snap_cap, int *snap_n, acg_route *routes, int route_cap,
				  int *nroutes, int *dropped, float *pass_ms);

/* diagnostics: the reassembly table (reasm.hip) on caller-supplied records, without a demodulator: acg_selftest_flights' shape.
 * in holds sum(batch[0..nbatch)) records as acg_drain_msgs hands them out; batch b is taken through one pass (filter f, NULL =
 * none; order (end_sample, chn) within the batch) of a table made from cfg.  status[i] (ACG_REASM_*) belongs to in[i].  The
 * completed messages of all batches go to done (done_cap records) and text (text_cap bytes) as acg_drain_reassembled hands them
 * out, *ndone of them; *dropped as there.  pass_ms (nbatch entries, or NULL): the device time of batch b's pass in milliseconds,
 * HIP events around it (the records' way to the device is outside).  ACG_EAGAIN: done or text too small; ACG_ENODEV: no GPU;
 * ACG_ESTATE: the product library (the entry is compiled into the lab library only). */
int  acg_selftest_reasm(const acg_msg *in, const int *batch, int nbatch, const acg_reasm_config *cfg, const acg_msg_filter *f,
			unsigned char *status, acg_reasm_msg *done, int done_cap, char *text, size_t text_cap, int *ndone, int *dropped,
			float *pass_ms);

/* diagnostics: the flight table's text (flight_text.hip) on caller-supplied entries and routes, without traffic: a table made
 * from cfg (at least n slots) holds in[0 .. n) as its live entries, in[0] the latest update, and its queue holds rt[0 .. nr),
 * stored in a shuffled order under tags that ascend with their index; then exactly what acg_flight_monitor_text (tcfg,
 * hdr_soh_sample) and acg_drain_routes_json launch.  An entry's strings are read up to their NUL: addr 7, fid 7, sa / da / eta 4
 * bytes; chm's low 16 bits, nbm, ts_sec, ts_usec, tl_sec, tl_usec as they stand.  mon / rts: the two output buffers, each all or
 * nothing as its entry point (ACG_EAGAIN when either is too small, both byte counts say what is needed).
 * ACG_EINVAL: n or nr < 0, a bad cfg or tcfg; ACG_ENODEV: no GPU. */
int  acg_selftest_flight_text(const acg_flight *in, int n, const acg_route *rt, int nr, const acg_flight_config *cfg,
			      const acg_flight_text_config *tcfg, long long hdr_soh_sample, char *mon, size_t mon_cap, size_t *mon_nbytes,
			      int *nrows, char *rts, size_t rts_cap, size_t *rts_nbytes, int *nlines);

/* diagnostics: the JSON sink's passes (label.hip's filter and compaction, then json.hip's order / measure / scan / render) on n
 * caller-supplied records, taken as acg_drain_msgs hands them out, without a demodulator: the lines of the records the filter f
 * (NULL = none) keeps, in (chn, end_bit) order (equal keys: input order), packed into out; *nbytes, *nlines as acg_drain_json.
 *   level        this entry has no lvlsum / bitcount: "level" is "%2.1f" of in[i].lvl as it stands (the device's log10 is not run);
 *   time         tv = cfg->t0 + in[i].soh_sample / 12500 s;
 *   dropped      in[i].reserved2 != 0 marks a record the block repair dropped: it yields nothing;
 *   freq         Fr_hz[nch] (NULL = 0); ACG_EINVAL unless 0 <= in[i].chn < nch <= 2^20 and 0 <= in[i].end_bit < 2^44.
 * ACG_EAGAIN: cap < the bytes needed (*nbytes says how many; out is untouched); ACG_ENODEV: no GPU. */
int  acg_selftest_msg_json(const acg_msg *in, int n, const acg_msg_filter *f, const acg_json_config *cfg, const int *Fr_hz, int nch,
			   char *out, size_t cap, size_t *nbytes, int *nlines);
/* diagnostics: how many lines acg_drain_json / acg_collect_json have rendered since acg_json_enable whose level, as the double
 * 10 log10(lvlsum / bitcount), lay within 8 ulp of the midpoint of two floats -- the only lines whose "level" could differ from
 * a host's that narrows glibc's log10 */
int  acg_lab_json_level_guard(acg_ctx *ctx, unsigned int *near_midpoint);

/* diagnostics: the text sink's passes (label.hip's filter and compaction, then text.hip's order / measure / scan / render) on n
 * caller-supplied records, exactly as acg_selftest_msg_json takes them (level = in[i].lvl as it stands, time, dropped records,
 * Fr_hz, the ACG_EINVAL conditions): the records of the messages the filter keeps, in (chn, end_bit) order (equal keys: input
 * order), packed into out; offs (n + 1 entries of room), *nbytes, *nrecs as acg_drain_text.
 * ACG_EAGAIN: cap < the bytes needed (*nbytes says how many; out and offs are untouched); ACG_ENODEV: no GPU. */
int  acg_selftest_msg_text(const acg_msg *in, int n, const acg_msg_filter *f, const acg_text_config *cfg, const int *Fr_hz, int nch,
			   char *out, size_t cap, size_t *nbytes, unsigned int *offs, int *nrecs);
/* diagnostics: the same count as acg_lab_json_level_guard (the same rule, sink_pack.h) for the records acg_drain_text /
 * acg_collect_text have rendered since acg_text_enable (PP records show no level and are not counted) */
int  acg_lab_text_level_guard(acg_ctx *ctx, unsigned int *near_midpoint);
/* measurement: the device time of json.hip's passes and of text.hip's over the SAME n records (taken as the two self tests take
 * them, no filter), the label pass run once before; HIP events around each renderer's launches, `warmup` unrecorded rounds and
 * `reps` recorded ones, the two arms alternated within every round: ms[0 .. reps) = the JSON passes, ms[reps .. 2 reps) = the text
 * passes, milliseconds.  With the measurement switch ACG_SINK_MAP=1 (acg_tune) both renderers run under a channel map (slot l ->
 * nch - 1 - l), as behind acg_set_channel_numbers.  ACG_ENODEV: no GPU. */
int  acg_lab_time_sink_passes(const acg_msg *in, int n, const acg_json_config *jcfg, const acg_text_config *tcfg, int nch, int warmup, int reps,
			      float *ms);

/* The three entries of the outputs below are compiled into the LAB library only (libacarsdec_amd_lab.so); the product library
 * exports their names and says ACG_ESTATE.
 *
 * diagnostics: the combined outputs pass (label.hip's filter and compaction, then outs.hip's one order and every leg of cfg) on n
 * caller-supplied records, exactly as acg_selftest_msg_json / _text take them (level = in[i].lvl as it stands, time, dropped
 * records, Fr_hz, the ACG_EINVAL conditions).  bufs[cfg->nlegs] as acg_drain_outputs takes them (offs: n + 1 entries of room); a
 * JSON or text leg is what its own self test hands out, the MSGS leg the kept records in key order (equal keys: input order) with
 * lvl as given, the reserved words zero and their acg_oooi.  *nrecs: the records of every leg.
 * ACG_EAGAIN: a leg's cap < the bytes it needs (every leg's nbytes says how many; nothing is written); ACG_ENODEV: no GPU;
 * ACG_ESTATE: the entry's own check found the legs not indexing alike -- the first *nrecs sorted keys the pass left on the device
 * are real and ascending (equal keys: input order) over distinct kept records, every table starts at 0, ascends strictly and ends
 * at its leg's bytes, and record i of the MSGS leg carries key i. */
int  acg_selftest_outputs(const acg_msg *in, int n, const acg_msg_filter *f, const acg_outputs_config *cfg, const int *Fr_hz, int nch,
			  acg_out_buf *bufs, int *nrecs);
/* diagnostics: acg_lab_json_level_guard / acg_lab_text_level_guard for leg `leg` of the outputs (a JSON or text leg) of a context
 * of the lab library */
int  acg_lab_outputs_level_guard(acg_ctx *ctx, int leg, unsigned int *near_midpoint);
/* measurement: as acg_lab_time_sink_passes, two arms over the SAME n records alternated within every round, each bracketed by HIP
 * events on one stream.  cfg: exactly one JSON leg and one text leg.  Arm A, ms[0 .. reps): json.hip's passes followed by
 * text.hip's, the launchers of acg_drain_json and acg_drain_text; arm B, ms[reps .. 2 reps): the combined pass over those two
 * legs (one keys launch, one sort and two scan launches fewer).  ACG_SINK_MAP=1 (acg_tune): both arms under a channel map, as
 * there.  ACG_ESTATE: what arm B left on the device is not, leg by leg, what arm A left (counters, offset table, bytes): the
 * figures are refused.  ACG_ENODEV: no GPU. */
int  acg_lab_time_output_passes(const acg_msg *in, int n, const acg_outputs_config *cfg, int nch, int warmup, int reps, float *ms);

/* Test hook (the block ring across the wrap of its 32-bit counters): right after acg_reset, with nothing queued,
 * sets the device's block counter, the repair pass's mark and the host's consumer mark to `value`, as if that many blocks had
 * been produced and consumed already.  ACG_ESTATE if calls have been issued since the reset. */
int  acg_lab_set_block_counter(acg_ctx *ctx, unsigned int value);
/* length of the block ring (a power of two) */
unsigned int acg_lab_block_ring_size(const acg_ctx *ctx);
/* Test hook (the stream counters after days of uptime: 2^31 samples at 12.5 kHz are 47.7 hours): right after acg_reset, sets the
 * 64-bit sample and bit counters of channels ch0 .. ch0+n-1 to the given values, and their 32-bit SOH stamp to the low word of
 * nsamp_total, as if that much signal had been demodulated already.  Nothing else changes.  ACG_EINVAL for a channel range
 * outside the context or a negative value; ACG_ESTATE if calls have been issued since the reset. */
int  acg_lab_set_stream_counters(acg_ctx *ctx, int ch0, int n, long long nsamp_total, long long nbit_total);

/* diagnostics: the down-converter launch the library makes for ONE launch of `nblocks` callbacks of u8 I/Q on this context, as the
 * launcher itself decides it (the same function sizes the launch): which kernel, how the input is cut into dispensed runs, the
 * grid.  A call of acg_process_iq_u8_* is one such launch per pipeline chunk (chunk_blocks callbacks; 0 = the whole call).  Reads
 * the tuning switches as a launch at this moment would; launches nothing.  ACG_EINVAL: nblocks outside 1..max_blocks. */
typedef struct acg_lab_launch_shape {
	int kernel;			/* 0 a vector-pipe kernel (nothing below but ncu, device_cus, chunk_blocks is set),
					   1 fir_u8_mm_kernel<cpr, stages>, 2 fir_u8_mm1_kernel<cpr> */
	int stages;			/* tiles in flight per wave */
	int cpr;			/* decim / 8 */
	int ncu;			/* CUs the launch is sized for (the down-converter's side of a CU partition) */
	int device_cus;			/* CUs of the device */
	int chunk_blocks;		/* the context's pipeline chunk in callbacks, 0 = whole calls */
	unsigned int units;		/* channel groups (kernel 1) or channels (kernel 2) */
	unsigned int runs_per_unit;
	unsigned int tiles_per_run;	/* 32-window tiles per dispensed run */
	unsigned int runs;		/* units * runs_per_unit */
	unsigned int wave_slots;	/* resident waves the run length was sized for; fewer runs than this: the grid is cut */
	unsigned int workgroups;	/* the grid */
	unsigned int waves;		/* waves launched: runs beyond these are handed out by ticket */
} acg_lab_launch_shape;
int  acg_lab_fir_launch_shape(acg_ctx *ctx, int nblocks, acg_lab_launch_shape *out);

/* diagnostics: which down-converter kernel family ONE launch of `nblocks` callbacks of sample format fmt (ACG_FMT_*) takes on this
 * context, as the launchers themselves decide it, and the streaming kernel's tile geometry.  A call of acg_process_samples_dev is
 * one such launch per pipeline chunk (chunk_blocks callbacks); acg_feed_samples_host launches the windows a feed completes.
 * Reads the tuning switches as a launch at this moment would; launches nothing.  ACG_EINVAL: nblocks outside 1..max_blocks, or a
 * format the context's window length does not admit (acg_last_error names the rule, as acg_process_samples_dev would). */
#define ACG_LAB_FIR_STREAMING     1	/* wave-private streaming kernel */
#define ACG_LAB_FIR_WORKGROUP     2	/* workgroup-granular fallback */
#define ACG_LAB_FIR_MATRIX        3	/* matrix pipe: several channels per stream (ACG_FMT_CS8 at decim 160 / 192 / 200) */
#define ACG_LAB_FIR_SHARED_VECTOR 4	/* shared-stream vector kernel (ACG_FMT_CS8 at other lengths or with ACG_FIR_MM=0) */
typedef struct acg_lab_samples_launch {
	int family;			/* ACG_LAB_FIR_* */
	int tile_windows;		/* streaming kernel: windows per tile (W); matrix pipe: 32 */
	int stages;			/* matrix pipe: tiles in flight per wave */
	int waves_per_workgroup;	/* streaming kernel */
	int bodies_per_run;		/* streaming kernel: two-tile bodies per dispensed run */
	int chunk_blocks;		/* the format's pipeline chunk in callbacks */
	unsigned int runs;		/* streaming kernel, matrix pipe: dispensed runs of the launch */
	unsigned int waves;		/* ... and waves launched: runs beyond these are handed out by ticket */
} acg_lab_samples_launch;
int  acg_lab_samples_launch_shape(acg_ctx *ctx, int fmt, int nblocks, acg_lab_samples_launch *out);

/* diagnostics: ONLY the de-interleave kernel of acg_process_pcm_dev (pcm.hip) on nframes host frames of the context's nch channels:
 * dm_host, an image of nch rows of pitch_floats words, is filled with `fill`, goes to the device, the kernel writes columns
 * [0, nframes) of its rows, and the WHOLE image comes back -- every word outside those columns must still be `fill`.  The input
 * is copied to a device buffer of exactly nframes*nch elements (rounded up to 4 bytes).  ACG_EINVAL: unknown fmt, a base that is
 * not 4-byte aligned, nframes < 0, pitch_floats < nframes. */
int  acg_lab_pcm_deinterleave(acg_ctx *ctx, int fmt, const void *frames_host, int nframes, float *dm_host, size_t pitch_floats, float fill);

/* only in the stamp build (libacarsdec_amd_stamp.so, -DACG_MSK_STAMP): phase cycle sums of the LAST demodulator launch,
 * [waves][10], and the lanes per channel of the context's demodulator */
int  acg_msk_stamp_read(acg_ctx *ctx, unsigned long long *out, int nwaves);
int  acg_msk_lanes_per_channel(const acg_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* ACARSDEC_AMD_LAB_H */
