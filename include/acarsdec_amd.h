/*
 * acarsdec_amd.h -- C ABI of the MI355X-native acarsdec DSP hot path.
 *
 * This is the drop-in boundary: a plain-C shared library (libacarsdec_amd.so) that a C host
 * (the reference's acarsdec, or any FFI) binds instead of the reference's per-channel DSP
 *      rtl.c:314-361  in_callback()   u8 I/Q -> NCO mix + decimate -> |D| -> dm_buffer
 *      msk.c:67-137   demodMSK()      MSK matched filter / bit-clock PLL -> putbit()
 *      msk.c:53-63    putbit()  ->  acars.c:246-375 decodeAcars()   (framing FSM, fed back into the PLL)
 * All citations are file:line into TLeconte/acarsdec v3.7.  No torch / C++ types cross this
 * boundary: pointers, sizes, ints.  Every function returns ACG_OK (0) or a negative ACG_E* code;
 * nothing throws.  One caller thread per context (same rule as the reference: all DSP runs on the
 * SDR callback thread, rtl.c:363-364).
 *
 * Two layers:
 *   1. batched API (acg_*, this header): thousands of channels per GPU, state resident in HBM across calls;
 *   2. legacy view (compat_msk.c, built inside the reference tree; entry points: acarsdec_amd_compat.h):
 *      initMsk()/demodMSK() with the reference's own signatures (acarsdec.h:190-191) on top of (1), so
 *      acars.c/output.c link unchanged.  See INTEGRATION.md.
 * Measurement and diagnostic entry points (tuning switches, probes, self tests, generators) are NOT product API: they are
 * declared in acarsdec_amd_lab.h.  The shared library exports exactly what THIS header and acarsdec_amd_lab.h declare (a linker
 * version script made from them); what acarsdec_amd_compat.h declares lives in compat_msk.c, which is compiled into the
 * reference program, not into the library.
 */
#ifndef ACARSDEC_AMD_H
#define ACARSDEC_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACG_OK          0
#define ACG_EINVAL     -1   /* bad argument / configuration */
#define ACG_ENOMEM     -2   /* host or device allocation failed */
#define ACG_EHIP       -3   /* HIP runtime error (acg_last_error has the text) */
#define ACG_ENODEV     -4   /* no usable GPU: the library has NO CPU fallback */
#define ACG_EOVERFLOW  -5   /* results were LOST: the device lapped the block queue (the host collected too rarely), or a per-bit
                               log was longer than its buffer; what could be handed out has been.  From acg_drain_* /
                               acg_collect_* it reports the loss ONCE and may still leave blocks queued (the caller's buffer was
                               smaller than what survived): call again -- the next call returns ACG_OK or ACG_EAGAIN.
                               The rule, for every acg_drain_* / acg_collect_* (cap = the queue's length in blocks, consumed = the
                               blocks handed out or declared lost so far, live = the blocks queued by ALL process calls issued so
                               far, upto = live for a drain, the queue's length at the end of the call `lag` calls back for a
                               collect):  lost = max(0, live - cap - consumed) blocks, the oldest, are gone (their count is in
                               acg_last_error and goes to acg_stats_read's lost_blocks); then the oldest
                               min(max(0, upto - consumed), what the caller's buffer holds) blocks that remain are handed out.
                               ACG_EOVERFLOW iff lost > 0.  The loss is judged against `live` for a collect as well: the calls
                               newer than its mark write into the queue whether the host has waited for them or not */
#define ACG_ESTATE     -6   /* call sequence error */
#define ACG_EAGAIN     -7   /* drain/collect: the caller's buffer is full and more results are queued -- nothing is lost,
                               call again */

#define ACG_INTRATE     12500     /* acarsdec.h:31 */
#define ACG_BLOCK       1024      /* rtl.c:49 RTLOUTBUFSZ: outputs per reference callback */
#define ACG_MAXDECIM    320       /* rtl.c:39 RTLMULTMAX: limit of the u8 I/Q path */
#define ACG_MAXDECIM_SAMPLES 1024 /* limit of the acg_*_samples_* formats (air.c:213: 10 Msps -> 800) */
#define ACG_FLEN        11        /* msk.c:25 */
#define ACG_TXTMAX      250       /* acarsdec.h:55 */

/* acg_config.flags */
#define ACG_F_BITLOG    1u        /* keep per-bit {soft symbol, level} records of each call (8 B per bit to device memory: 2 % of the
                                   * demodulator's time at 1024 channels, 5 % at 16 384; a host that only wants messages leaves it off) */
#define ACG_F_TIMING    2u        /* bracket kernels with HIP events (acg_get_timing) */
#define ACG_F_REPAIR    4u        /* run the block thread's check/repair (acars.c:93-215) on the device:
                                     drain/collect then return what outputmsg() receives -- parity/CRC
                                     verified or repaired, parity stripped, err = parity errors found --
                                     and omit the blocks the reference drops */
#define ACG_F_EXACT_FIR 8u        /* verification mode: the u8 down-converter adds the rtlMult terms of rtl.c:349-351 one after
                                     the other, products and 127.37 per sample rounded separately -- what an IEEE (-O2) build of
                                     the reference executes -- so dm and everything after it is BIT-IDENTICAL to that build.
                                     The streaming kernels re-associate the sum (|d dm| <= 1e-5 |dm|, like the reference's own
                                     -Ofast build); this one is ~20x slower and exists to prove that nothing else differs */

#define ACG_F_PRECISE_MIXER 16u   /* verification mode: the demodulator's mixer (msk.c:86-91, cexp) evaluates sin/cos with the < 1 ulp
                                     polynomial instead of the product's table + rotation (<= 2.1 ulp).  The loop keeps only the
                                     float-rounded products in*cos, in*(-sin), which are the same for both: this flag lets a
                                     maintainer check that on his own input (every bit, state double and block must not change).
                                     ~10 % slower per bit */

typedef struct acg_ctx acg_ctx;

typedef struct {
	int device;         /* HIP device ordinal */
	int nch;            /* channels */
	int nstreams;       /* I/Q streams: nch (one stream per channel) or fewer (rtl.c shape: all
	                       channels of a dongle share one stream, rtl.c:344-354) */
	int decim;          /* M = rtlMult (rtl.c:35-37): input rate = 12500*M */
	int ntaps;          /* complex taps per channel, 1..decim.  Reference: ntaps == decim */
	int max_blocks;     /* capacity: 1024-output blocks per acg_process_* call */
	uint32_t flags;
	int max_lag;        /* most process calls acg_collect_* may stay behind (sizes the block queue: the worst case of
	                       max_lag + 1 calls, 304 B per block, rounded UP to a power of two -- so up to twice that worst
	                       case is allocated; acg_max_lag() says what the queue really holds).  0 = as many calls as fit
	                       into a power-of-two queue of at most 512 MiB, at most 6 (very wide contexts: two calls,
	                       whatever they cost); a host that collects with lag <= 1 after every call asks for 1 */
} acg_config;

/* MSK + framing fields of channel_t (acarsdec.h:76-89) */
typedef struct {
	double MskPhi, MskDf, MskLvlSum;
	float MskClk;
	int MskBitCount;
	unsigned int MskS, idx;
	float inb[2 * ACG_FLEN];      /* re,im interleaved (acarsdec.h:83) */
	int outbits, nbits, Acarsstate;
	int blk_len, blk_err;
	int soh_back;                 /* not in channel_t: 12.5 kHz samples since the SOH byte of the block being assembled completed
	                                 (where acars.c:290 stamps blk->tv; what soh_sample of that block will be measured from).
	                                 Meaningful while Acarsstate is TXT / CRC1 / CRC2, else 0.  acg_set_state() re-bases it on the
	                                 destination slot's own sample counter, so a channel moved mid-block keeps its time stamp;
	                                 a host that leaves it 0 stamps the block at the moment of the move. */
} acg_chan_state;

/* A message block as decodeAcars() queues it (msgblk_t, acarsdec.h:48-57; acars.c:350-364):
 * text still carries parity bits, no repair applied. */
typedef struct {
	int chn;
	int len;
	int err;
	float lvl;                    /* 10*log10(MskLvlSum/MskBitCount), acars.c:351 */
	unsigned char crc[2];
	unsigned char txt[ACG_TXTMAX];
	long long end_bit;            /* per-channel index of the bit that completed the block */
	long long end_sample;         /* per-channel 12.5 kHz sample index of that bit */
	long long soh_sample;         /* per-channel 12.5 kHz sample index of the bit that completed the block's SOH byte: the
	                                 moment the reference stamps blk->tv (acars.c:290 gettimeofday), which every printer and
	                                 JSON sink reports (output.c:162,227,244,361).  Epoch rule: a host that noted the wall
	                                 clock t0 of the channel's first sample since acg_reset sets
	                                     tv = t0 + soh_sample / 12500 s
	                                 (INTEGRATION.md "time stamps"); soh_sample <= end_sample, both count from acg_reset */
} acg_frame;

/* A message as outputmsg() splits it out of a processed block (acarsmsg_t, acarsdec.h:108-124; output.c:486-560,
 * 566-568,623-631 in the build without libacars): the fixed binary record every sink (printmsg, buildjson, Netout*)
 * formats from.  Strings are NUL terminated like the reference's; txt is txt_len bytes, not terminated.  The CLI's
 * filters (-A airflt, -b label_filter, -e emptymsg) apply only once a host sets them (acg_set_msg_filter). */
#define ACG_MSGTXTMAX   242
typedef struct {
	int chn;
	int err;                      /* parity errors repaired (acars.c:156) */
	float lvl;                    /* dB, acars.c:351 */
	int txt_len;
	long long end_bit, end_sample;   /* as in acg_frame */
	long long soh_sample;         /* as in acg_frame: where blk->tv is taken (acars.c:290); msg->tv = t0 + soh_sample / 12500 s */
	int reserved1;
	char reserved2;
	char mode;
	char addr[8];                 /* aircraft registration without the leading dots */
	char ack;                     /* NAK is reported as '!' (output.c:511-514) */
	char label[3];                /* a DEL second character is reported as 'd' (output.c:518-520) */
	char bid;                     /* block id; '0'..'9' = downlink (output.c:31) */
	char no[5];                   /* message number, downlinks only */
	char fid[7];                  /* flight id, downlinks only */
	char bs, be;                  /* start / end of text characters (STX or ETX / ETX or ETB) */
	char down;
	char txt[ACG_MSGTXTMAX];
	int reserved3;
} acg_msg;

/* ---- lifetime ---------------------------------------------------------------------------- */
int  acg_device_count(void);
int  acg_create(acg_ctx **out, const acg_config *cfg);
void acg_destroy(acg_ctx *ctx);
const char *acg_strerror(int code);
const char *acg_last_error(const acg_ctx *ctx);
const char *acg_version(void);

/* ---- channel set-up (host side of rtl.c:268-287) ------------------------------------------ */
/* rtl.c:131-168 chooseFc(): Fd (Hz) is sorted in place; returns Fc or 0 ("too far apart"). */
unsigned int acg_rtl_choose_fc(unsigned int *Fd, unsigned int nbch, int decim);
/* rtl.c:283-286: wf[ind] = cexpf(-j*AMFreq*ind)/rtlMult/127.5, taps_out is [decim][2]. */
int  acg_rtl_taps(int Fr_hz, unsigned int Fc_hz, int decim, float *taps_out);
/* taps: [n][ntaps][2] float for channels ch0..ch0+n-1 */
int  acg_set_taps(acg_ctx *ctx, int ch0, int n, const float *taps);
/* stream index of every channel; default: channel c reads stream c % nstreams */
int  acg_set_channel_streams(acg_ctx *ctx, const int *stream_of_channel);
/* initMsk() (msk.c:30-51) + initAcars() (acars.c:230-234) for all channels */
int  acg_reset(acg_ctx *ctx);

/* ---- the hot path ------------------------------------------------------------------------- */
/* in_callback() for every channel: iq is [nstreams] rows of interleaved u8 I,Q, row r at
 * iq + r*pitch_bytes, each nblocks*1024*decim*2 bytes (rtl.c:330).  *_dev: device pointer,
 * asynchronous: the down-converter (the only reader of iq) is enqueued on hip_stream (NULL = the
 * context's own stream) so later work on that stream may overwrite iq; the demodulator follows on
 * an internal stream.  Results are complete after acg_sync / acg_drain_frames / acg_collect_frames.
 * *_host: the librtlsdr contract (rtl.c:314-330: the buffer is the driver's again when the callback returns) -- the call
 * returns as soon as the input has LEFT iq_host; it went to one of two device staging buffers on a copy stream of its own,
 * beside the kernels of the previous call, and this call's kernels run after the return.  From pinned memory
 * (acg_host_alloc, or the caller's own buffers through acg_host_register) that copy is one DMA at the link's rate; pageable
 * memory works and is staged by the runtime. */
int  acg_process_iq_u8_dev(acg_ctx *ctx, const uint8_t *iq_dev, size_t pitch_bytes, int nblocks,
			   void *hip_stream);
int  acg_process_iq_u8_host(acg_ctx *ctx, const uint8_t *iq_host, size_t pitch_bytes, int nblocks);
/* demodMSK() for every channel straight from 12.5 kHz samples (soundfile.c:71-77, alsa.c:122):
 * dm is [nch] rows of `len` floats, row c at dm + c*pitch_floats; len <= max_blocks*1024.
 * *_dev: asynchronous like the iq entry points -- dm is consumed after what hip_stream holds so far, and
 * later work on hip_stream (refilling dm in place) is ordered behind the demodulator that reads it. */
int  acg_process_dm_dev(acg_ctx *ctx, const float *dm_dev, size_t pitch_floats, int len,
			void *hip_stream);
int  acg_process_dm_host(acg_ctx *ctx, const float *dm_host, size_t pitch_floats, int len);
/* only the down-converter (rtl.c:332-354), no demodMSK: leaves dm readable by acg_read_dm */
int  acg_fir_only_dev(acg_ctx *ctx, const uint8_t *iq_dev, size_t pitch_bytes, int nblocks,
		      void *hip_stream);
int  acg_sync(acg_ctx *ctx);

/* ---- the other front ends' sample formats ----------------------------------- */
#define ACG_FMT_CS16       1   /* interleaved int16 I,Q: soapy.c:238-241 (dm = |D| with the /32768 of soapy.c:241) */
#define ACG_FMT_S16_SPLIT  2   /* int16 I plane + int16 Q plane: sdrplay.c:219-225 (dm = |D|/4) */
#define ACG_FMT_F32_REAL   3   /* real float32 samples, complex taps: air.c:314-324 */
/* the recordings' formats: soapy.c:232-254's loop with only the sample type changed; taps as acg_soapy_taps makes them */
#define ACG_FMT_CS8        4   /* interleaved int8 I,Q (SigMF ci8, HackRF):                    dm = |D| / 128 */
#define ACG_FMT_CF32       5   /* interleaved float32 I,Q (SigMF cf32_le, .cfile, Soapy CF32): dm = |D|       */
/* soapy.c:163-166 oscillator table ([decim][2]); ch->Fr is a float in that front end */
int  acg_soapy_taps(float Fr_hz, int freq_hz, int decim, float *taps_out);
/* sdrplay.c:160-164 (fixed rate multiplier 160) */
int  acg_sdrplay_taps(float Fr_hz, unsigned int Fc_hz, float *taps_out);
/* air.c:62 centre frequency (no IF-filter branch) and air.c:278-285 taps; inrate = 12500*decim */
unsigned int acg_airspy_choose_fc(unsigned int minF_hz, unsigned int maxF_hz);
int  acg_airspy_taps(int Fr_hz, int Fc_hz, unsigned int inrate, float *taps_out);
/* Window-aligned device input: [nstreams] rows of nblocks*1024*decim samples.  Bytes per sample: 4 (ACG_FMT_CS16,
 * ACG_FMT_F32_REAL), 2 per plane (ACG_FMT_S16_SPLIT: I plane at the row start, Q plane plane_bytes further), 2 (ACG_FMT_CS8),
 * 8 (ACG_FMT_CF32); plane_bytes is 0 for every format but split planes.  decim % 4 == 0 and decim <= ACG_MAXDECIM_SAMPLES
 * (split planes: decim % 8 == 0, decim <= 208; ACG_FMT_CS8: decim % 8 == 0, decim <= ACG_MAXDECIM; ACG_FMT_CF32:
 * decim % 2 == 0); base, pitch and plane 16-byte aligned; anything else is ACG_EINVAL before a launch.  Several channels of a
 * stream (acg_set_channel_streams) each read it; ACG_FMT_CS8 at decim 160 / 192 / 200 then takes the matrix-pipe kernel of the
 * u8 path (exact integer sums, one rounding).  Same asynchronous contract and FIR/demodulator stream pipeline as
 * acg_process_iq_u8_dev. */
int  acg_process_samples_dev(acg_ctx *ctx, int fmt, const void *dev, size_t pitch_bytes, size_t plane_bytes,
			     int nblocks, void *hip_stream);
/* Host input of ANY length per call, as the SDR drivers deliver it: windows may straddle calls (the
 * reference carries D / its index across buffers: soapy.c:232-254, sdrplay.c:215-236, air.c:299-338).
 * p0 = samples (I plane for ACG_FMT_S16_SPLIT), p1 = Q plane or NULL (every other format); rows pitch_samples apart; a
 * sample is the format's bytes per sample as above (lengths and the pitch count samples, never bytes).  Same return contract
 * and the same two staging buffers as acg_process_iq_u8_host: the copy of feed i+1 runs beside the kernels of feed i. */
int  acg_feed_samples_host(acg_ctx *ctx, int fmt, const void *p0, const void *p1, size_t pitch_samples,
			   size_t nsamples);

/* ---- any input sample rate: the down-converter's windows on a rational grid ---------------- */
/* The reference's down-converter (rtl.c:344-354, soapy.c:232-254: one window per 12.5 kHz output, a per-window oscillator
 * table that restarts at index 0, |D|) with only the window grid generalised.  R = the input rate in Hz, g = gcd(R, 12500),
 * P = R / g, Q = 12500 / g.  Window k, counted per context from acg_reset, covers input samples [s_k, s_(k+1)) with
 * s_k = floor(k P / Q) in exact integer arithmetic, so its length L_k is floor(P / Q) or ceil(P / Q), and
 *     dm_c[k] = scale_fmt / L_k * | sum_{i < L_k} v[s_k + i] * t_c[i] |
 * with t_c the decim = ntaps = ceil(P / Q) taps of channel c -- the bare oscillator (acg_rate_taps): the 1 / L_k differs from
 * window to window and is the kernel's -- and scale_fmt = 1/32768 (ACG_FMT_CS16), 1/128 (ACG_FMT_CS8), 1 (ACG_FMT_CF32),
 * 1/127.5 for ACG_FMT_CU8 whose sample is (I - 127.37) + j (Q - 127.37) (rtl.c:338-339).  Q == 1 is the integer case.  The
 * outputs are 12 500 per second on average and each is displaced by less than one input sample: end_sample, soh_sample and the
 * time stamps keep their meaning.  All streams of a context share one rate. */
#define ACG_FMT_CU8        6   /* interleaved u8 I,Q (rtl_sdr files, SigMF cu8): on the acg_*_rate_* entry points only */
/* ceil(rate / 12500) = what acg_config.decim (== ntaps) must be, or ACG_EINVAL outside 25 000 <= rate_hz <= 12500 * ACG_MAXDECIM */
int  acg_rate_decim(unsigned int rate_hz);
/* s_k0 .. s_(k0 + n): n + 1 values of the grid above */
int  acg_rate_window_starts(unsigned int rate_hz, unsigned long long k0, int n, unsigned long long *starts);
/* [n][2]: (float)cos, (float)-sin of 2 pi frac(offset_hz * i / rate_hz), i = 0 .. n - 1, evaluated in double */
int  acg_rate_taps(unsigned int rate_hz, double offset_hz, int n, float *taps_out);
/* The context's input rate; 0 = integer windows again (the default).  ACG_EINVAL unless cfg.decim == cfg.ntaps ==
 * acg_rate_decim(rate_hz); ACG_ESTATE while either host feed carries samples.  Sets the window counter to 0, as acg_reset
 * does.  While a rate is set the window-aligned entry points (acg_process_iq_u8_*, acg_fir_only_dev, acg_process_samples_dev,
 * acg_feed_samples_host) return ACG_ESTATE and launch nothing; acg_process_dm_* and the PCM entry points do not care. */
int  acg_set_input_rate(acg_ctx *ctx, unsigned int rate_hz);
/* Device input at the rate set: each of the [nstreams] rows holds nsamples samples (ACG_FMT_CU8, _CS8, _CS16 or _CF32; 2, 2, 4,
 * 8 bytes each) that begin at the context's current window start.  Base and pitch 16-byte aligned, pitch_bytes >= nsamples *
 * bytes per sample rounded up to 16 (a 16-byte read that covers a row's last sample stays inside the row's pitch).  Runs the
 * whole windows that fit, at most max_blocks * 1024 of them, and the demodulator on them, under the asynchronous contract of
 * acg_process_samples_dev; reports *nwin and *consumed = s_(k0 + nwin) - s_k0 and advances the context by that much: the
 * caller presents the rest again at the head of the next call.  ACG_ESTATE while acg_feed_rate_host carries samples or no
 * rate is set; split planes and real f32 belong to front ends that fix their own rates: ACG_EINVAL. */
int  acg_process_rate_dev(acg_ctx *ctx, int fmt, const void *dev, size_t pitch_bytes, size_t nsamples,
			  void *hip_stream, int *nwin, size_t *consumed);
/* Host input of ANY length at the rate set: acg_feed_samples_host's scheme with variable windows -- the incomplete window's
 * samples wait at the head of the other staging row (always a window start), the copy of feed i+1 runs beside the kernels of
 * feed i.  Rows pitch_samples apart. */
int  acg_feed_rate_host(acg_ctx *ctx, int fmt, const void *samples, size_t pitch_samples, size_t nsamples);

/* ---- channel filters: taps over several windows (overlapped FIR) ---------------------------- */
/* The definition above is a boxcar of one output period: a sinc with side lobes at -13 dB, -18 dB, ... that folds every
 * neighbour into the 12.5 kHz output.  On a wide-band recording, where the neighbours are not on the 12.5 kHz raster, a
 * context whose rate is a multiple of 12 500 Hz (Q == 1, M = decim = rate / 12500, window k = samples [k M, (k + 1) M)) can
 * be given a filter of J = nseg windows, 2 <= J <= ACG_MAXSEG, with J M complex taps t_c[n] per channel:
 *     dm_c[k] = scale_fmt * | sum_{n < J M} v[(k - J + 1) M + n] * t_c[n] |
 * v[i] = 0 before the context's first sample since acg_reset / acg_set_input_rate / acg_set_channel_filter; k counts windows
 * as the rate path does; scale_fmt is the rate path's and there is no 1 / L: the taps carry the gain (DC gain 1 reproduces the
 * boxcar's level).  The ACG_FMT_CU8 sample is ((float)I - 127.37f) + j ((float)Q - 127.37f), each rounded once; the constant
 * is not folded out of the sum.  Output k exists as soon as window k is complete: acg_process_rate_dev and acg_feed_rate_host
 * deliver the same nwin and consumed as without a filter, in any split of the input the same bits, and every record field
 * keeps its meaning.  The filter's centre lies (J - 1) / 2 output samples earlier than the boxcar's: a host that cares
 * subtracts (J - 1) / 25000 s from its t0.  The down-converter's history (the J - 1 windows before the next call) belongs to
 * the context, not to a channel: acg_get_state / acg_set_state do not carry it, a channel moved between contexts starts with
 * J - 1 windows of zeros. */
#define ACG_MAXSEG 4
/* taps: [nch][nseg * decim][2], index 0 multiplies the OLDEST sample.  nseg == 0 or taps == NULL: off, the rate path is
 * bit for bit what it was.  ACG_ESTATE unless a rate is set, ACG_EINVAL when that rate is no multiple of 12 500 Hz or nseg
 * is outside 2 .. ACG_MAXSEG, ACG_ESTATE while acg_feed_rate_host carries samples.  Zeroes the window counter and the
 * history, as acg_set_input_rate does; acg_set_input_rate (any value) switches the filter off; acg_reset keeps the filter
 * and empties the history, and so does a change of sample format between calls; acg_set_taps keeps setting the one-window
 * table, which is unused while a filter is on. */
int  acg_set_channel_filter(acg_ctx *ctx, int nseg, const float *taps);
/* Kaiser-windowed sinc of nseg * decim taps (decim = rate_hz / 12500), -6 dB at cutoff_hz, DC gain 1, times the oscillator
 * exp(-j 2 pi frac(offset_hz n / rate_hz)); everything evaluated in double, rounded once to float.  [nseg * decim][2].
 * ACG_EINVAL unless rate_hz is a multiple of 12 500 that acg_rate_decim takes, 2 <= nseg <= ACG_MAXSEG,
 * 0 < cutoff_hz < rate_hz / 2 and beta >= 0. */
int  acg_channel_filter_taps(unsigned int rate_hz, double offset_hz, int nseg, double cutoff_hz, double beta, float *taps_out);

/* ---- the 12.5 kHz front ends' own shape: interleaved PCM frames (soundfile.c, alsa.c) ------- */
#define ACG_PCM_S16 1   /* interleaved int16 frames, x/32768: what sf_read_float makes of a PCM16 file (soundfile.c:65) */
#define ACG_PCM_F32 2   /* interleaved float32 frames: sf_read_float's own output, alsa.c:66,114 */
/* demodMSK() for every channel from frames as a sound file, a sound card or a recorder delivers them: [nframes][nch], frame i
 * at frames + i*nch elements, 4-byte aligned base.  A device kernel de-interleaves (and scales: exact) into the context's dm
 * image; the results are those of acg_process_dm_host on the de-interleaved floats.
 * frames_dev: on the device, nframes <= max_blocks*1024; asynchronous, the contract of acg_process_dm_dev -- except that later
 * work on hip_stream is ordered behind the de-interleave kernel (the only reader of frames_dev), not behind the demodulator. */
int  acg_process_pcm_dev(acg_ctx *ctx, int fmt, const void *frames_dev, int nframes, void *hip_stream);
/* frames in host memory, ANY nframes (chunks of max_blocks*1024 frames, one contiguous copy each into the two staging buffers
 * of the *_host entry points, the copy of a chunk beside the kernels of the chunk before); returns when the input has left the
 * caller's buffer (the contract of acg_process_iq_u8_host / acg_feed_samples_host).  ACG_ESTATE while acg_feed_samples_host
 * carries a partial window in those buffers.  The bit log (ACG_F_BITLOG: acg_read_bits*, acg_replay_bits) holds the bits of the
 * call's LAST chunk only (every chunk is a call of its own): a host that replays bits feeds at most max_blocks*1024 frames per call. */
int  acg_feed_pcm_host(acg_ctx *ctx, int fmt, const void *frames, size_t nframes);

/* pinned host memory for the *_host entry points (hipHostMalloc / hipHostRegister behind a C face, so that a C host needs
 * no HIP headers): acg_host_alloc returns NULL on failure */
void *acg_host_alloc(size_t bytes);
void acg_host_free(void *p);
int  acg_host_register(void *p, size_t bytes);
int  acg_host_unregister(void *p);

/* ---- results ------------------------------------------------------------------------------ */
/* Blocks completed since the last drain/collect, ordered by (chn, end_bit) within the call.  Waits for ALL
 * enqueued work of the context.  If more blocks are queued than max_frames, the oldest max_frames are handed out, the
 * rest STAY queued and the call returns ACG_EAGAIN (call again: across calls the order is completion order). */
int  acg_drain_frames(acg_ctx *ctx, acg_frame *out, int max_frames, int *nframes);
/* Streaming variant: hands over the blocks of every process call except the `lag` most recent
 * ones and waits only for those older calls, so that the newest call(s) keep the GPU busy
 * (lag = 1: classic double buffering; lag = 0: wait for the last call only).  0 <= lag <= acg_max_lag().
 * With fewer than lag + 1 calls issued it hands out nothing.  A host that collects after every call is never lapped and
 * never waits for a newer call.  One that fell behind -- it skipped collects, or left a remainder through a small buffer,
 * so that what it has not consumed plus the worst case of the `lag` newer calls no longer fits the queue -- gets the rule
 * of ACG_EOVERFLOW applied to the queue as it stands once every issued call has finished: such a collect (and only such a
 * one) waits for the newest call too, reports what was overwritten, and hands out what is left up to its own mark. */
int  acg_collect_frames(acg_ctx *ctx, int lag, acg_frame *out, int max_frames, int *nframes);
/* Largest lag this context accepts: its block queue is sized for the worst case (a 56-bit block every 291 samples on
 * every channel) of acg_max_lag() + 1 calls, so a host that collects after every call cannot be lapped.
 * At least acg_config.max_lag if that was given (the power-of-two queue may hold more), else 6 unless that would take
 * more than 512 MiB (then fewer, at least 1). */
int  acg_max_lag(const acg_ctx *ctx);
/* SURVEY 8f.4, the batch sink: like acg_drain_frames / acg_collect_frames, but every block is taken through
 * outputmsg()'s field split on the device and handed over as a fixed binary record.  Needs ACG_F_REPAIR (outputmsg()
 * receives repaired, parity-stripped blocks); blocks the repair drops are omitted.  Ordered by (chn, end_bit) within the
 * call.  A call looks at the oldest max_msgs queued blocks only (splits, copies and consumes exactly those); if more are
 * queued they STAY queued and the call returns ACG_EAGAIN ("call again"; across calls the order is completion order).
 * Every byte of a record is defined (unused text bytes are 0). */
int  acg_drain_msgs(acg_ctx *ctx, acg_msg *out, int max_msgs, int *nmsgs);
int  acg_collect_msgs(acg_ctx *ctx, int lag, acg_msg *out, int max_msgs, int *nmsgs);

/* ---- the batch sink's filters and label decoding (output.c:537-540,650; label.c) ---------- */
/* The CLI's three message filters, in the order outputmsg() applies them to a repaired block:
 *   ACG_MSGF_DOWNLINK_ONLY  -A: drop uplinks (msg->down == 0)
 *   label list              -b: keep only labels (as the C string the split reports: DEL second char -> 'd') equal to one of the
 *                           tokens; a label whose first byte is NUL matches nothing; nlabels == 0 = no label filter
 *   ACG_MSGF_SKIP_EMPTY     -e: drop when txt[0] == 0 -- NOT txt_len == 0: a text that starts with a NUL byte goes too
 * A token slot holds up to 3 chars + NUL.  Labels have at most 2, so a longer token (stored as its first 3 chars) never matches
 * but still switches the label filter on, as in the reference. */
#define ACG_MSGF_DOWNLINK_ONLY  1u
#define ACG_MSGF_SKIP_EMPTY     2u
#define ACG_MSGF_MAXLABELS      64
typedef struct {
	uint32_t flags;               /* ACG_MSGF_* */
	int nlabels;                  /* 0 .. ACG_MSGF_MAXLABELS tokens in use */
	char labels[ACG_MSGF_MAXLABELS][4];   /* NUL terminated, non-empty */
} acg_msg_filter;

/* label.c build_label_filter(): splits a -b argument on ':' the way strtok does (empty tokens skipped: "::H1:" = {H1}).
 * NULL or "" (or only separators) leaves the label list empty.  Only f->nlabels and f->labels are written (flags are the
 * caller's).  ACG_EINVAL: f is NULL, or more than ACG_MSGF_MAXLABELS tokens. */
int  acg_parse_label_filter(const char *arg, acg_msg_filter *f);
/* Sets the filters of every message entry point (acg_drain_msgs, acg_collect_msgs and the _oooi pair below) from the next call
 * on; NULL = no filter (the default).  A block a filter drops is consumed and yields nothing.  acg_drain_frames /
 * acg_collect_frames are never filtered (they sit before outputmsg()).  With no filter set, acg_drain_msgs / acg_collect_msgs do
 * exactly what they did before: no extra pass, nothing extra copied.  ACG_EINVAL: unknown flag bits, nlabels outside
 * 0..ACG_MSGF_MAXLABELS, an empty or unterminated token. */
int  acg_set_msg_filter(acg_ctx *ctx, const acg_msg_filter *f);

/* label.c DecodeLabel() (run by printmsg, buildjson and the flight monitor: output.c:206-215,280-295,391-399) as a fixed record:
 * oooi_t (acarsdec.h:94-102) field for field, then its return value.  Fields are 4 chars + NUL, copied from the text at fixed
 * offsets; the JSON keys are depa = sa, dsta = da, eta, gtout = gout, gtin = gin, wloff = woff, wlin = won, each present when
 * decoded != 0 and the field's first byte is not NUL.  When decoded == 0 every field is zero (the reference discards a partial
 * fill); every byte of the record is defined.
 * Bytes at or past txt_len read as 0.  The reference reads its calloc(txt_len + 1) copy of the text there and, where an
 * extractor reaches beyond txt_len + 1, heap memory (a Q1 downlink with an empty text prints "dsta":"U" or whatever lies there),
 * so this record equals the reference's output wherever the label's extractor stays within the text and its NUL. */
typedef struct {
	char da[5], sa[5], eta[5], gout[5], gin[5], woff[5], won[5];
	char decoded;                 /* DecodeLabel()'s return value: 1 = the label's checks passed */
	char reserved[4];             /* 0 */
} acg_oooi;

/* acg_drain_msgs / acg_collect_msgs with each message's label decoded on the device: oooi[i] belongs to out[i].  Same contract:
 * the oldest max_msgs queued blocks are looked at and consumed, results in (chn, end_bit) order, ACG_EAGAIN / ACG_EOVERFLOW as
 * there; the filters of acg_set_msg_filter apply.  One extra device pass (filter, decode, compaction) per call; only the records
 * kept cross to the host. */
int  acg_drain_msgs_oooi(acg_ctx *ctx, acg_msg *out, acg_oooi *oooi, int max_msgs, int *nmsgs);
int  acg_collect_msgs_oooi(acg_ctx *ctx, int lag, acg_msg *out, acg_oooi *oooi, int max_msgs, int *nmsgs);
/* ---- the flight table: addFlight() / routejson() (output.c:361-456), what -o 3 and -o 5 print from ---------------------------
 * Off by default; with it off every entry point launches, copies and returns exactly what it does without this section.
 * When enabled, every message entry point (acg_drain_msgs, acg_collect_msgs and the _oooi pair) takes the blocks it consumes
 * through addFlight() on the device, before the -e filter drops anything, in the same host round trip as the label pass; the
 * records those calls hand out are byte-identical with and without the table.
 *   which messages   those that passed -A / -b and are downlinks with bs != 0x03 (output.c:545-567,647).  -e is tested AFTER
 *                    addFlight(), as in the reference; a message that skips addFlight() never emits a route (the reference
 *                    reads an uninitialised pointer there).
 *   time             tv = t0 + soh_sample / 12500 s (the epoch rule of acg_frame), in integer arithmetic.
 *   ORDER            within one drain / collect call the messages are applied in ascending (end_sample, chn); across calls,
 *                    call order holds.  Every channel of a context advances by the same samples per process call, so this is
 *                    global real-time order as long as no call returns ACG_EAGAIN.  A call that does return ACG_EAGAIN has
 *                    consumed an arbitrary oldest part of the block queue: the rule then still holds per call, not globally.
 *   expiry           an entry whose last message is more than mdly seconds older than the newest message second seen so far
 *                    is gone (output.c:407-423; the CLI's -t, default 600); its aircraft starts anew with its next message.
 * One table per context.  A host that spreads its channels over several devices keeps one table at one of them and moves the
 * other contexts' EVENTS there (acg_flights_export / acg_flights_import below): that is exact, merging snapshots is not. */
typedef struct {
	long long t0_sec;             /* wall clock of the channels' first sample since acg_reset */
	int t0_usec;                  /* 0 .. 999999 */
	int mdly;                     /* -t: seconds without a message after which a flight is forgotten, >= 1 */
	int max_flights;              /* capacity, >= 1 (rounded up to a power of two) */
} acg_flight_config;

/* One entry of the table (flight_t, output.c:345-358).  Every byte is defined (strings are NUL padded). */
typedef struct {
	char addr[8];
	char fid[7];                  /* of the latest message; may be empty */
	char rt;                      /* 1 = this entry has emitted its route record */
	int nbm;                      /* messages */
	int first_chn, last_chn;      /* channel of the first and of the latest message */
	int reserved1;                /* 0 */
	unsigned long long chm;       /* bit (chn % 64) set for every channel heard on: the reference's mask for its <= 16 channels */
	long long ts_sample, tl_sample;   /* soh_sample of the first and of the latest message */
	long long ts_sec, tl_sec;     /* ... and as wall clock, from t0 */
	int ts_usec, tl_usec;
	char da[5], sa[5], eta[5], gout[5], gin[5], woff[5], won[5];   /* as in acg_oooi: per field the last non-empty value */
	char reserved2[5];            /* 0 */
} acg_flight;

/* One route record (routejson(), output.c:428-456): emitted by the first message of an entry that passed -e as well and has a
 * flight id while departure and destination are known; once per entry.  Every byte is defined. */
typedef struct {
	long long soh_sample;         /* of the triggering message */
	long long sec;                /* its tv */
	int usec;
	int chn;
	char fid[7];
	char sa[5];                   /* "depa" */
	char da[5];                   /* "dsta" */
	char addr[8];
	char reserved[7];             /* 0 */
} acg_route;

/* Switches the table on (cfg) or off and frees it (NULL).  Enabling an enabled table replaces it by an empty one.
 * ACG_EINVAL: mdly < 1, max_flights < 1, t0_usec outside 0..999999; ACG_ESTATE: context without ACG_F_REPAIR.
 * acg_reset() empties the table, the pending routes and the event queues of export and import (the sample clock restarts
 * there); switching the table off does too. */
int  acg_flights_enable(acg_ctx *ctx, const acg_flight_config *cfg);
/* The live entries in printmonitor()'s order (output.c:467-481): latest update first (the order is total).  ACG_EAGAIN: max is
 * too small, *n is the number needed.  *dropped (may be NULL) counts, since enable / reset, every (call, aircraft) pair in which an
 * aircraft that is not in the table had messages and found no slot -- an aircraft that stays unplaced over three calls counts
 * three times.  Its messages are still delivered, only the table update is skipped.  A slot is free when it was never used or its
 * entry has expired; an aircraft looks for one within 128 slots of its place, so a table filled to the last slots can drop an
 * aircraft before it is completely full (size max_flights with room to spare), and when a call brings more new aircraft than
 * there are free slots, which of them get the slots is not specified.  Waits for the passes issued so far; consumes nothing. */
int  acg_flight_snapshot(acg_ctx *ctx, acg_flight *out, int max, int *n, int *dropped);
/* The route records emitted so far, in the order of their triggering messages.  ACG_EAGAIN: more are queued than fit, call again.
 * Routes stay queued until they are drained or the table is reset or switched off: a host that enables the table for the monitor
 * alone still drains them now and then, or the queue grows by one record per route emitted. */
int  acg_drain_routes(acg_ctx *ctx, acg_route *out, int max, int *n);

/* ---- one flight table for the channels of several contexts: export and import of flight EVENTS --------------------------
 * A host that shards its channels over several contexts (devices) keeps ONE table, at an OWNER context.  Tables cannot be merged
 * exactly from snapshots (the per-field "last non-empty value" and the "first message that ..." route rule are gone there); the
 * stream of events can: every message that reaches addFlight() is one event with the order key (end_sample, chn), and the rest
 * of the pass is defined by that order alone.  So the other contexts (the PEERS) hand their events out instead of applying them,
 * the owner takes them in and runs its ordinary pass over its own and the imported events together.
 * Nothing here is used by default: with these entry points unused every other one launches, copies and returns what it did.
 *
 * THE ROUND that makes it exact.  One process call on every context over the same sample span; then one message entry point on
 * every peer, followed by acg_drain_flight_events; then the owner imports all of them and makes its own message entry point
 * call.  As long as no call of a round returns ACG_EAGAIN, the owner's table, routes and `dropped` are those of one context
 * that holds all channels and makes the same calls.  (Merging once per shard instead of once per round is NOT the same: the
 * running "newest second seen" and the restart of expired entries depend on the order of all messages.)
 *
 * One event.  88 bytes, every byte defined. */
typedef struct {
	long long end_sample;         /* with chn: the order key of the pass */
	long long soh_sample;
	long long sec;                /* tv of the message, already t0 + soh_sample / 12500 s of the exporting context */
	int usec;                     /* 0 .. 999999 */
	int chn;                      /* the channel number the table records (see acg_flights_set_channels) */
	char addr[8];                 /* NUL padded, never empty */
	char fid[7];                  /* NUL padded, may be empty */
	char e_ok;                    /* 1: the message also passed -e */
	acg_oooi oooi;                /* all zero when the label did not decode */
} acg_flight_event;

/* The number recorded for each local channel in events and therefore in first_chn, last_chn, chm, acg_route.chn and the order
 * key: chn[nch], or NULL for the identity.  It applies to the context's own table and to what it exports; for `c mod N` sharding
 * on rank r local channel l gets l * N + r.  ACG_EINVAL: a value outside 0 .. 2^20 - 1 (the key holds 20 bits); ACG_ESTATE: the
 * table is off.  acg_reset keeps the map; acg_flights_enable drops it with the table.
 * A host that numbers everything it hands out calls acg_set_channel_numbers (below, "sharded hosts") instead: the table follows the
 * context's map while it has none of its own.  A map given HERE keeps precedence, for the table only. */
int  acg_flights_set_channels(acg_ctx *ctx, const int *chn);
/* on != 0: this context is a peer.  Its flight pass stops behind the extraction (after -A / -b, before -e, as ever): the events
 * of the blocks a message entry point consumes go to an export queue on the device, channel numbers applied, and the table stays
 * empty.  The queue grows until it is drained, like the route queue.  The message, JSON and text records handed out are the same
 * bytes with export on and off.  A message whose address is empty (seven dots on the air) is no event of an export: acg_flight_event
 * has no room for "no address", a single context gives it a row.  Turning export on or off empties the table and both queues;
 * acg_reset empties them too and keeps the switch.  ACG_ESTATE: the table is off. */
int  acg_flights_export(acg_ctx *ctx, int on);
/* The events exported so far, in any order; their (end_sample, chn) pairs are distinct.  ACG_EAGAIN: more are queued than fit,
 * nothing is lost, call again.  Waits only for the passes issued so far.  ACG_ESTATE: the table or export is off. */
int  acg_drain_flight_events(acg_ctx *ctx, acg_flight_event *out, int max, int *n);
/* ACG_OK when every one of the n events is one acg_flights_import takes, else ACG_EINVAL: usec outside 0 .. 999999, addr[0] == 0,
 * chn outside 0 .. 2^20 - 1, end_sample negative or >= 2^43, e_ok not 0 or 1.  Host arithmetic only, no context. */
int  acg_flight_events_check(const acg_flight_event *ev, int n);
/* Queues events of other contexts at the owner (table on, export off).  They are applied by the owner's NEXT message entry
 * point, in the same pass as the events of the blocks that call consumes, in ascending (end_sample, chn) over both; a call that
 * consumes no blocks still runs the pass over the imports alone.  Checked on the host first (acg_flight_events_check):
 * ACG_EINVAL queues nothing.  sec / usec are used as they come, so a peer may have its own t0.  end_sample is the caller's
 * business: contexts that were reset together and fed in lock step share it as it is, otherwise the host rebases the field
 * before the import.  ACG_ESTATE: the table is off, or this context exports. */
int  acg_flights_import(acg_ctx *ctx, const acg_flight_event *ev, int n);
/* A pass over the queued imports alone: for an owner with no channels of its own, or the end of a run.  Nothing queued: no-op. */
int  acg_flights_commit(acg_ctx *ctx);

/* ---- the flight table's text: the monitor screen (-o 3) and the route line (-o 5), rendered on the device -------------------
 * Off by default; with it off every entry point launches, copies and returns exactly what it does without this section, and
 * with it on the message entry points, acg_flight_snapshot and acg_drain_routes still hand out the same bytes.  The two entry
 * points below hand out TEXT, byte for byte what the reference built without libacars writes:
 *   acg_flight_monitor_text   one frame of printmonitor() (output.c:458-484): the 7 bytes of cls() ("\x1b[H\x1b[2J",
 *                             ACG_MONITOR_CLS_LEN: a host that writes to a file skips them), "             Acarsdec monitor ",
 *                             printtime(tv), the column header line (ACG_MONITOR_HDR_LEN bytes so far), then one row per live
 *                             entry in acg_flight_snapshot's order:
 *                               " %-8s %-7s %3d " addr fid nbm, nbch mask columns ('x' / '.': bit i of chm) padded with spaces
 *                               to 16, " ", printtime(ts), " %4s " or six spaces for each of sa, da, eta, "\n".
 *   acg_drain_routes_json     the queued route records as routejson()'s lines (output.c:428-456,677-683, cJSON fmt = 0):
 *                               {"timestamp":T[,"station_id":".."],"flight":"..","depa":"..","dsta":".."} and '\n',
 *                             in the order of their triggering messages (the tag is sorted on the device), packed back to back.
 * printtime() is "%02d:%02d:%02d.%03ld" of gmtime_r(tv_sec) and tv_usec / 1000 in integer arithmetic (the text sink's date rule:
 * exact from 1970 to the year 9999).  "%-8s", "%-7s", "%4s" and "%3d" pad and never cut.  T is the JSON sink's "timestamp"
 * (print_number's text, exact for 10^9 <= tv_sec < 9999999998), strings are escaped as the JSON sink escapes them.
 *
 * ACG_MONITOR_ROW_MAX, the longest row, token by token:
 *   " " 1 + "%-8s" 8 (an addr has at most 7 characters) + " " 1 + "%-7s" 7 + " " 1 + "%3d" 11 ("-2147483648"; 3 while
 *   0 <= nbm <= 999, 10 for 2^31 - 1) + " " 1 + the mask 16 + " " 1 + printtime 12 + 3 x 6 + "\n" 1
 * = 78; a row is 70 bytes while nbm <= 999.  A frame is at most ACG_MONITOR_HDR_LEN + rows * ACG_MONITOR_ROW_MAX bytes.
 * ACG_ROUTE_LINE_MAX, the longest line, every string byte a control character that costs 6 ("\u00xx"), key by key:
 *   {"timestamp":        13 + 18   ten integer digits, the point, seven fraction digits ("%1.17g")
 *   ,"station_id":".."   15 + 32 * 6 + 1 = 208
 *   ,"flight":".."       11 + 7 * 6 + 1 = 54   (acg_route's fid[7] read as at most 7 bytes; a message's flight id has 6: 48)
 *   ,"depa":".."          9 + 4 * 6 + 1 = 34     ,"dsta":".."   34
 *   }  1,   '\n'  1
 * = 363 (357 for anything traffic can produce). */
#define ACG_MONITOR_CLS_LEN  7
#define ACG_MONITOR_HDR_LEN  110  /* 7 + 30 + 12 + 61 ("\n Aircraft Flight   Nb Channels     First    DEP   ARR   ETA\n") */
#define ACG_MONITOR_ROW_MAX  78
#define ACG_ROUTE_LINE_MAX   363
typedef struct {
	int nbch;                     /* 0 .. 16: the mask columns printmonitor() shows (the reference's nbch, padded to MAXNBCHANNELS = 16) */
	char station_id[33];          /* idstation (-i) for the route line; "" = the key is absent (output.c:444) */
} acg_flight_text_config;
/* Switches the renderer on (cfg) or off (NULL).  The station is escaped once, like the JSON sink's.  ACG_EINVAL: nbch outside
 * 0..16, an unterminated station_id; ACG_ESTATE: the flight table is not enabled.  acg_reset keeps the configuration; switching
 * the table off -- or on again: acg_flights_enable replaces it -- switches the renderer off too. */
int  acg_flight_text_enable(acg_ctx *ctx, const acg_flight_text_config *cfg);
/* One frame.  The header's time is the time of the message the frame is printed for -- the reference prints a frame per kept
 * message with that message's tv, also for messages that never reach addFlight() (an uplink without -A) -- so the caller names
 * it: tv = t0 + hdr_soh_sample / 12500 s in integers (acg_msg's soh_sample; t0 from acg_flight_config).  hdr_soh_sample < 0: the
 * newest live entry's tl, or t0 when the table is empty.  *nbytes bytes, *nrows rows, *dropped (may be NULL) as
 * acg_flight_snapshot; out is not NUL terminated.  ALL OR NOTHING: cap too small returns ACG_EAGAIN with *nbytes = the bytes
 * needed and leaves out untouched.  Waits for the passes issued so far and consumes nothing, like the snapshot.
 * ACG_ESTATE: the table or the renderer is off. */
int  acg_flight_monitor_text(acg_ctx *ctx, long long hdr_soh_sample, char *out, size_t cap, size_t *nbytes, int *nrows, int *dropped);
/* The queued routes as lines.  ALL OR NOTHING: cap too small returns ACG_EAGAIN with *nbytes = the bytes needed and nothing is
 * consumed; otherwise the queue is emptied.  It is the queue of acg_drain_routes: each entry point consumes what it hands out.
 * ACG_ESTATE: the table or the renderer is off, or an earlier acg_drain_routes returned ACG_EAGAIN and left records pending on
 * the host -- a host uses one of the two, or switches only behind an ACG_OK. */
int  acg_drain_routes_json(acg_ctx *ctx, char *out, size_t cap, size_t *nbytes, int *nlines);

/* ---- reassembly of multi-block messages: the reference's call site of la_reasm_fragment_add() (output.c:33-101,579-626) ------
 * An ACARS message longer than about 220 characters travels as a chain of blocks, every block but the last ending in ETB; the
 * reference built with libacars reports per block "assstat" and hands the complete text on.  Off by default; with it off every
 * entry point launches, allocates, copies and returns exactly what it does without this section.  When enabled, every message
 * entry point, the sinks and the outputs take the blocks they consume through ONE table on the device, resident across calls like
 * the flight table, and by the flight table's three rules:
 *   which messages   those that passed -A / -b, downlinks and uplinks alike, BEFORE -e (output.c:537-540,650);
 *   time             tv_us = t0_us + 80 * soh_sample, in integers;
 *   ORDER            within one drain / collect call ascending (end_sample, chn); across calls, call order.
 * The table's rule, for a message m (tests/reasm_model.py is this text as a plain dict walk; it follows libacars' documented
 * behaviour from the reference's call site outward and HAS NOT BEEN RUN AGAINST libacars):
 *   bs == ETX or bid == 0 (a squitter)                SKIPPED, the table is not touched
 *   key    (addr, label, msn) as C strings; msn = no[0..2] of a downlink ('0' <= bid <= '9'), "" of an uplink
 *   seq    (signed char)no[3] - 'A' of a downlink, whose first fragment has 0; bid - 'A' of an uplink, which has no first and
 *          wraps (after 'Z' in mode '2', after 'W' otherwise, comes 'A')
 *   an entry whose FIRST fragment is more than its time-out older than m (strictly; VGT4 = 660 s for a chain begun by a
 *   downlink, VAT4 = 90 s by an uplink) is gone.  Then, without an entry: a downlink with seq != 0 is OUT_OF_SEQUENCE, a block
 *   that does not end in ETB is SKIPPED (a single-block message), anything else begins an entry.  With one: seq == the previous
 *   is a DUPLICATE (entry untouched); seq != previous + 1 is OUT_OF_SEQUENCE and the entry is gone; a text that would pass
 *   max_text bytes is an OVERFLOW and the entry is gone; otherwise m.txt (txt_len bytes) is appended, and the entry is
 *   IN_PROGRESS while m ends in ETB, else COMPLETE, handed to acg_drain_reassembled and gone.
 * The fragment data is acg_msg.txt: the H1 sublabel / MFI prefix that libacars strips per fragment is NOT stripped.
 * "assstat" and the complete text are not spliced into the JSON / text sinks' rendered bytes: a host does that by (chn, end_bit). */
#define ACG_REASM_UNKNOWN          0   /* a chain's first block found no slot in the table (counted in `dropped`) */
#define ACG_REASM_COMPLETE         1
#define ACG_REASM_IN_PROGRESS      2
#define ACG_REASM_SKIPPED          3
#define ACG_REASM_DUPLICATE        4
#define ACG_REASM_OUT_OF_SEQUENCE  5
#define ACG_REASM_ARGS_INVALID     6   /* libacars' value; never produced */
#define ACG_REASM_OVERFLOW         7   /* ours: the one bound a fixed table needs */
typedef struct {
	long long t0_sec;             /* wall clock of the channels' first sample since acg_reset */
	int t0_usec;                  /* 0 .. 999999 */
	int max_msgs;                 /* chains in progress the table holds, >= 1 (rounded up to a power of two), <= 2^20; 0 = 1024 */
	int max_text;                 /* bytes of a complete text: a multiple of 16, 16 .. 65536; 0 = 3584 (16 blocks of 224) */
} acg_reasm_config;

/* One completed message.  Every byte is defined (strings are NUL padded). */
typedef struct {
	int chn;                      /* of the FINAL fragment, as chn, end_bit, end_sample, soh_sample: they name the handed-out */
	int nfrag;                    /* message (or sink line) this text replaces.  nfrag: fragments appended */
	long long end_bit, end_sample, soh_sample;
	long long first_soh_sample;   /* soh_sample of the chain's first fragment */
	unsigned long long text_off;  /* the text: text_len bytes at text + text_off of the same acg_drain_reassembled call */
	unsigned int text_len;
	char down;                    /* the final fragment is a downlink */
	char addr[8];
	char label[3];
	char msn[4];                  /* "" for an uplink */
	char reserved[12];            /* 0 */
} acg_reasm_msg;

/* Switches the table on (cfg) or off and frees it (NULL).  Enabling an enabled table replaces it by an empty one.  ACG_EINVAL: a
 * value outside the ranges above; ACG_ESTATE: context without ACG_F_REPAIR.  acg_reset() empties the table and the completed
 * messages not yet drained. */
int  acg_reasm_enable(acg_ctx *ctx, const acg_reasm_config *cfg);
/* acg_drain_msgs_oooi / acg_collect_msgs_oooi plus the reassembly status: status[i] (ACG_REASM_*) belongs to out[i]; oooi may be
 * NULL here.  The records are byte-identical to the plain pair's.  ACG_ESTATE: the table is off. */
int  acg_drain_msgs_reasm(acg_ctx *ctx, acg_msg *out, acg_oooi *oooi, unsigned char *status, int max_msgs, int *nmsgs);
int  acg_collect_msgs_reasm(acg_ctx *ctx, int lag, acg_msg *out, acg_oooi *oooi, unsigned char *status, int max_msgs, int *nmsgs);
/* The completed messages in the order of their final fragments, texts packed back to back into text (cap bytes, *nbytes used).
 * Whole records only: ACG_EAGAIN when more are queued than max or cap take, the rest stay queued (a text longer than cap never
 * fits: cap >= max_text always makes progress).  *dropped (may be NULL) counts, since enable / reset, every (call, key) pair in
 * which a key that could begin an entry found no slot within 128 of its place (see acg_flight_snapshot); its creating blocks
 * carry ACG_REASM_UNKNOWN.  Waits for the passes issued so far.  ACG_ESTATE: the table is off. */
int  acg_drain_reassembled(acg_ctx *ctx, acg_reasm_msg *out, int max, int *n, char *text, size_t cap, size_t *nbytes, int *dropped);
/* "unknown", "complete", "in progress", "skipped", "duplicate", "out of sequence", "invalid args", "overflow": libacars' names in
 * libacars' order, for a host that prints assstat; anything else: "unknown". */
const char *acg_reasm_status_name(int status);

/* ---- the JSON sink: buildjson() (output.c:227-324), what -o 4 prints, -j sends and the MQTT sink publishes ------------------
 * Off by default; with it off every entry point launches, copies and returns exactly what it does without this section.
 * acg_drain_json / acg_collect_json are message entry points like acg_drain_msgs / acg_collect_msgs (ACG_F_REPAIR, the filters
 * of acg_set_msg_filter, the flight table when it is on, blocks the repair dropped yield nothing), but what they hand out is
 * TEXT rendered on the device: one JSON object per kept message, each ended by '\n', packed back to back in `out`, in
 * (chn, end_bit) order within the call -- byte for byte what the reference built without libacars prints through
 * cJSON_PrintPreallocated(.., fmt = 0), time stamps included.  *nbytes bytes, *nlines lines; out is not NUL terminated.
 * A call looks at the oldest cap / ACG_JSON_LINE_MAX queued blocks only and consumes exactly those; more queued: ACG_EAGAIN
 * (call again, nothing is lost).  ACG_EINVAL: cap < ACG_JSON_LINE_MAX; ACG_ESTATE: no ACG_F_REPAIR, or acg_json_enable has
 * not been called.
 *
 * ACG_JSON_LINE_MAX, the longest line, every string byte a control character that costs 6 ("\u00xx"), key by key:
 *   {"timestamp":            13 + 18   ten integer digits, the point, seven fraction digits ("%1.17g")
 *   ,"station_id":".."       15 + 32 * 6 + 1 = 208
 *   ,"channel":              11 + 11   (an int)
 *   ,"freq":                  8 + 7    ,"level":  9 + 7    (both cut to 7 characters by the reference's 8-byte buffer)
 *   ,"error":                 9 + 11
 *   ,"mode":".."              9 + 6 + 1       ,"label":".."   10 + 2 * 6 + 1    ,"block_id":".."  13 + 6 + 1
 *   ,"ack":".."               8 + 6 + 1       ,"tail":".."     9 + 7 * 6 + 1
 *   ,"flight":".."           11 + 6 * 6 + 1   ,"msgno":".."   10 + 4 * 6 + 1
 *   ,"text":".."              9 + 242 * 6 + 1 = 1462
 *   ,"end":true              11
 *   ,"depa":".." ,"dsta":".." ,"eta":".." ,"gtout":".." ,"gtin":".." ,"wloff":".." ,"wlin":".."     64 + 7 * (4 * 6 + 1) = 239
 *   ,"app":{"name":"..","ver":".."}}    16 + 16 * 6 + 9 + 16 * 6 + 3 = 220,    '\n'  1
 * = 2454, rounded up to a multiple of 64. */
#define ACG_JSON_LINE_MAX  2496
typedef struct {
	long long t0_sec;             /* the epoch rule of acg_frame: tv = t0 + soh_sample / 12500 s, in integers */
	int t0_usec;                  /* 0 .. 999999 */
	char station_id[33];          /* idstation (-i); "" = the key is absent (output.c:246) */
	char app_name[17], app_ver[17];   /* "app":{"name":..,"ver":..}: the reference's are "acarsdec" and its ACARSDEC_VERSION */
} acg_json_config;
/* Switches the JSON sink on (cfg) or off and frees it (NULL).  Fr_hz: the channels' frequencies in Hz ([nch]; NULL = all 0, what
 * a reference built without an SDR front end prints): "freq" is snprintf(8 bytes, "%3.3f", (float)(Fr / 1000000.0)), rendered
 * here once per channel (output.c:232,248).  The three strings are escaped once, like every string of a line.
 * "timestamp" is print_number's text (cJSON.c:475-506: "%1.15g", or "%1.17g" when that does not parse back) of
 * (double)tv_sec + (double)tv_usec / 1e6, exact for 10^9 <= tv_sec < 9999999998 (September 2001 .. the year 2286); outside, the
 * token is the integer second (well formed, not the reference's digits).  ACG_EINVAL: t0_sec outside [10^9, 4 * 10^9), t0_usec
 * outside 0..999999, an unterminated string; ACG_ESTATE: context without ACG_F_REPAIR.  acg_reset keeps the configuration. */
int  acg_json_enable(acg_ctx *ctx, const acg_json_config *cfg, const int *Fr_hz);
int  acg_drain_json(acg_ctx *ctx, char *out, size_t cap, size_t *nbytes, int *nlines);
int  acg_collect_json(acg_ctx *ctx, int lag, char *out, size_t cap, size_t *nbytes, int *nlines);

/* ---- the text sink: the reference's other per-message formats, rendered on the device like the JSON sink's lines ------------
 * Off by default; with it off every entry point launches, copies and returns exactly what it does without this section.
 *   ACG_TEXT_ONELINE  printoneline() (output.c:327-346): what -o 1 prints, one '\n'-ended line per message;
 *   ACG_TEXT_STD      printmsg() (output.c:162-224) of the build without libacars: what -o 2 prints, and acarsdec without -o;
 *                     a record begins with the "\n[#" of its header line;
 *   ACG_TEXT_PP       the packet Netoutpp() formats for -N (netout.c:101-120), no trailing newline;
 *   ACG_TEXT_SV       the packet Netoutsv() formats for -n (netout.c:122-140), likewise.
 * acg_drain_text / acg_collect_text are message entry points like acg_drain_json / acg_collect_json (ACG_F_REPAIR, the filters of
 * acg_set_msg_filter, the flight table when it is on, blocks the repair dropped yield nothing, (chn, end_bit) order within the
 * call).  Record i is out[offs[i] .. offs[i + 1]); offs gets *nrecs + 1 entries (offs[*nrecs] == *nbytes), records are packed
 * back to back, out is not NUL terminated.  A record holds its bytes exactly as the reference's printf writes them, a NUL
 * ("%1c" of a NUL mode), a '\n' or any other byte included: hence a table and no line count.  (PP, SV: the reference sends
 * strlen() of its packet, so a datagram ends before the first NUL; a host that wants exactly that sends strnlen(record, length).)
 * A call looks at the oldest min(max_recs, cap / ACG_TEXT_REC_MAX) queued blocks only and consumes exactly those; more queued:
 * ACG_EAGAIN (call again, nothing is lost).  ACG_EINVAL: cap < ACG_TEXT_REC_MAX or max_recs < 1; ACG_ESTATE: no ACG_F_REPAIR, or
 * the sink is not enabled.  The JSON sink may be enabled too; each entry point consumes the blocks it hands out.
 *
 * The bytes: "%Ns" right-justifies a C string (it ends at its first NUL) to at least N and never cuts it; "%1c" writes the byte.
 * printoneline shows the first 59 bytes of the text up to its NUL, '\n' and '\r' as a space; Netoutpp the whole text with the same
 * substitution and `bid ? bid : '.'`; Netoutsv the text as it is and "%03d" of (int)lvl, toward zero (-7.9: "-07"; a level that
 * is not finite: the x86 conversion's -2147483648).  "L:%+5.1f" is the float's exact value rounded half-even to one decimal,
 * sign forced, space padded to 5 ("+inf", "-inf", "+nan", "-nan" as glibc); the level's float has the JSON sink's residual
 * (the device's log10 against glibc's; acarsdec_amd_lab.h counts the candidates).  The date is printdate()'s
 * "%02d/%02d/%04d %02d:%02d:%02d.%03ld" of gmtime_r(tv), tv = t0 + soh_sample / 12500 s in integers (SV: without ".%03ld"),
 * exact from 1970 to the year 9999 (2100 is no leap year); printdate() prints nothing when tv_sec + tv_usec == 0, which
 * t0_sec >= 10^9 excludes.
 *
 * ACG_TEXT_REC_MAX, the longest record of any format -- printmsg()'s, token by token:
 *   "\n[#" 3 + chn 11 + " (" 2 + "F:%3.3f " 12 ("F:-2147.484 ") + "L:" 2 + level 21 (sign, 18 digits, ".d") + " E:" 3 + err 11 + ") " 2 = 67
 *   date 23, " " + 32 x '-' + "\n" 34
 *   "Mode : %1c " 9     "Label : %2s " 11    "Id : %1c " 7      "Ack : %1c\n" 8
 *   "Aircraft reg: %s " 14 + 7 + 1 = 22      "Flight id: %s\n" 11 + 6 + 1 = 18       "No: %4s" 8       "\n" 1
 *   the text and "\n" 242 + 1 = 243          "ETB\n" 4          26 x '#' + "\n" 27
 *   "Destination Airport : %s\n" 22 + 4 + 1 = 27       "Departure Airport : %s\n" 25     "Estimation Time of Arrival : %s\n" 34
 *   "Gate out Time : %s\n" 21    "Gate in Time : %s\n" 20     "Wheels off Tme : %s\n" 22     "Wheels on Time : %s\n" 22
 * = 653, rounded up to a multiple of 64.  (Netoutsv's: 32 + 11 + 19 + 11 + 11 + the fields + 242 + 17 separators < 400.) */
#define ACG_TEXT_ONELINE  1   /* -o 1  printoneline()  output.c:327-346 */
#define ACG_TEXT_STD      2   /* -o 2  printmsg()      output.c:162-224, the build without libacars */
#define ACG_TEXT_PP       3   /* -N    Netoutpp()      netout.c:101-120: one datagram per record, no trailing newline */
#define ACG_TEXT_SV       4   /* -n    Netoutsv()      netout.c:122-140: likewise */
#define ACG_TEXT_F_DATE   1u  /* printdate() is printed (the reference: inmode != 2); ONELINE and STD only */
#define ACG_TEXT_F_FREQ   2u  /* the "F:%3.3f " token of printmsg() (the reference: inmode >= 3); STD only */
#define ACG_TEXT_REC_MAX  704
typedef struct {
	int format;                   /* ACG_TEXT_* */
	unsigned int flags;           /* ACG_TEXT_F_* the format takes */
	long long t0_sec;             /* the epoch rule of acg_frame: tv = t0 + soh_sample / 12500 s, in integers */
	int t0_usec;                  /* 0 .. 999999 */
	char station_id[33];          /* idstation (-i): SV's "%8s" */
} acg_text_config;
/* Switches the text sink on (cfg) or off and frees it (NULL).  Fr_hz: the channels' frequencies in Hz ([nch]; NULL = all 0):
 * "F:%3.3f " is snprintf of the DOUBLE Fr / 1000000.0 (output.c:168-169; not the JSON line's float), rendered here once per
 * channel, as is SV's padded station.  ACG_EINVAL: an unknown format, a flag the format does not take, t0_sec outside
 * [10^9, 4 * 10^9), t0_usec outside 0..999999, an unterminated station_id; ACG_ESTATE: context without ACG_F_REPAIR.
 * acg_reset keeps the configuration. */
int  acg_text_enable(acg_ctx *ctx, const acg_text_config *cfg, const int *Fr_hz);
int  acg_drain_text(acg_ctx *ctx, char *out, size_t cap, size_t *nbytes, unsigned int *offs, int max_recs, int *nrecs);
int  acg_collect_text(acg_ctx *ctx, int lag, char *out, size_t cap, size_t *nbytes, unsigned int *offs, int max_recs, int *nrecs);

/* ---- the outputs: every output of a message from ONE consumption ---------------------------------------------------------------
 * The reference's outputmsg() prints the format -o selects AND sends the packet -n / -N / -j selects, both from the same msg
 * (output.c:665-701).  The entry points above each consume the blocks they hand out, so a block rendered as a JSON line is gone
 * before the text sink sees it.  acg_drain_outputs / acg_collect_outputs consume a take of blocks ONCE and hand out up to
 * ACG_OUT_LEGS_MAX "legs" rendered from the same kept records in the same order: record i of every leg is the same message.
 * Off by default; with it off nothing is allocated or launched and every entry point above hands out the bytes it hands out
 * without this section.
 *   Legs.    1 <= nlegs <= ACG_OUT_LEGS_MAX, the kinds pairwise distinct: at most one ACG_OUT_MSGS leg and one ACG_OUT_JSON leg,
 *            and two or three different text formats are allowed (-o 1 beside -n: ONELINE and SV).  -o 4 -j is ONE JSON leg, which
 *            the host writes and sends, like the reference's one jsonbuf.  A text leg's kind is its ACG_TEXT_* format and its
 *            flags are the ACG_TEXT_F_* that format takes; the other kinds take no flag.
 *   Errors.  acg_outputs_config_check (host arithmetic only, no context) and acg_outputs_enable say ACG_EINVAL for nlegs out of
 *            range, an unknown kind, a flag the kind does not take, duplicate kinds, t0_sec outside [10^9, 4 * 10^9), t0_usec
 *            outside 0..999999, an unterminated string: the conditions of acg_json_enable and acg_text_enable, through the same
 *            checks.  ACG_ESTATE: context without ACG_F_REPAIR.  cfg == NULL: off, everything freed.  acg_reset keeps the
 *            configuration, acg_destroy frees it.  Fr_hz as for acg_json_enable / acg_text_enable, one table for all legs.
 *   Take.    A call looks at the oldest min(max_recs, min over legs of cap / recmax) queued blocks (recmax: ACG_JSON_LINE_MAX,
 *            ACG_TEXT_REC_MAX, sizeof(acg_msg)) and consumes exactly those, ONCE, for all legs.  More queued: ACG_EAGAIN -- call
 *            again, nothing is lost and nothing is rendered twice.  ACG_EINVAL: a leg's cap below its recmax, a missing buffer or
 *            table, max_recs < 1.  ACG_ESTATE: no ACG_F_REPAIR, or the outputs are not enabled.
 *   Order.   Every leg hands out *nrecs records in ascending key order -- the (chn, end_bit) order of every other entry point,
 *            numbered by acg_set_channel_numbers' map when one is set.  JSON and text legs hand out offs[0 .. *nrecs] (the JSON
 *            leg too, so that all legs index alike); acg_sink_keys(.., ACG_SINK_OUTPUTS, ..) hands out ONE key list for all legs.
 *   Bytes.   Each leg is byte for byte what its own entry point hands out for the same blocks: acg_drain_json; acg_drain_text
 *            with that format and those flags; acg_drain_msgs_oooi (lvl, soh_sample, the reserved words zero, the number handed
 *            out in chn).
 *   Once.    The filters, the flight table's pass, the statistics pass and (in a call that consumes nothing) the commit of imported
 *            flight events happen once per take, whatever the number of legs.  -o 3 / -o 5 stay acg_flight_monitor_text /
 *            acg_drain_routes_json, called after the outputs call: that call has updated the table.
 * The individually enabled JSON and text sinks are separate states and keep working beside the outputs; each entry point consumes
 * the blocks it hands out. */
#define ACG_OUT_MSGS      0x10   /* acg_msg + acg_oooi records, as acg_drain_msgs_oooi hands them out */
#define ACG_OUT_JSON      0x20   /* buildjson()'s line, as acg_drain_json */
/* text legs use ACG_TEXT_ONELINE / _STD / _PP / _SV as their kind */
#define ACG_OUT_LEGS_MAX  4
typedef struct {
	int kind;                     /* ACG_OUT_MSGS, ACG_OUT_JSON or an ACG_TEXT_* format */
	unsigned int flags;           /* the ACG_TEXT_F_* the kind takes, else 0 */
} acg_out_leg;
typedef struct {
	int nlegs;
	acg_out_leg leg[ACG_OUT_LEGS_MAX];
	long long t0_sec;             /* one epoch for all legs: tv = t0 + soh_sample / 12500 s, in integers */
	int t0_usec;                  /* 0 .. 999999 */
	char station_id[33], app_name[17], app_ver[17];   /* as acg_json_config's; station_id also SV's "%8s" */
} acg_outputs_config;
typedef struct {
	void *out;                    /* JSON and text legs: the packed records; MSGS leg: an acg_msg array */
	size_t cap;                   /* bytes of out (MSGS leg too) */
	unsigned int *offs;           /* JSON and text legs: max_recs + 1 entries of room; MSGS leg: NULL */
	acg_oooi *oooi;               /* MSGS leg only: cap / sizeof(acg_msg) entries; else NULL */
	size_t nbytes;                /* out: bytes written to this leg */
} acg_out_buf;
int  acg_outputs_config_check(const acg_outputs_config *cfg);
int  acg_outputs_enable(acg_ctx *ctx, const acg_outputs_config *cfg, const int *Fr_hz);
/* bufs[nlegs], in the order of the configuration's legs */
int  acg_drain_outputs(acg_ctx *ctx, acg_out_buf *bufs, int max_recs, int *nrecs);
int  acg_collect_outputs(acg_ctx *ctx, int lag, acg_out_buf *bufs, int max_recs, int *nrecs);

/* ---- sharded hosts: global channel numbers in everything handed out, and the keys to merge by ---------------------------------
 * A host that spreads its channels over N contexts (`c mod N`: slot l of rank r is channel l * N + r) gives every context the
 * numbers of its slots once; from then on N contexts behind one host hand out exactly what ONE context over all channels hands
 * out, byte for byte and -- merged by the keys below -- in its order.  Unused, nothing changes: no launch, no copy, no byte.
 *
 * acg_channel_numbers_check: ACG_OK when every one of the n values lies in 0 .. 2^20 - 1 (the sinks' order key holds 20 bits of
 * channel) and the values are pairwise distinct (two slots under one number would make the order ambiguous), else ACG_EINVAL.
 * n == 0 is ACG_OK.  Host arithmetic only, no context. */
int  acg_channel_numbers_check(const int *chn, int n);
/* chn[nch]: the number handed out for each local channel (slot); NULL = the identity, the default.  Checked with the function
 * above: on ACG_EINVAL the map in force stays in force.  It takes effect with the NEXT entry point call, and blocks already queued
 * are numbered by the map in force when they are HANDED OUT, not when they were decoded.  acg_reset keeps the map.
 *   the number is used  in acg_frame.chn and acg_msg.chn, the JSON line's "channel", the channel tokens of the text formats
 *                       (number + 1, as the reference prints chn + 1), in the order of every entry point -- "(chn, end_bit) order
 *                       within the call" means the number handed out -- and in the sinks' order key (acg_sink_keys);
 *                       by the flight table (events, first_chn, last_chn, chm, acg_route.chn, its order key) unless
 *                       acg_flights_set_channels has given the table a map of its own;
 *   the slot stays      the index of everything that is a table per slot: the Fr_hz of acg_json_enable / acg_text_enable (a line
 *                       carries the number handed out and the frequency of its slot), acg_stats_read, acg_get_state /
 *                       acg_set_state, acg_set_taps, acg_set_channel_streams, acg_read_bits. */
int  acg_set_channel_numbers(acg_ctx *ctx, const int *chn);
/* The order keys, (number handed out) << 44 | end_bit, of the records the most recent acg_drain_json / acg_collect_json call
 * (sink == ACG_SINK_JSON) or acg_drain_text / acg_collect_text call (ACG_SINK_TEXT) handed out, in the order of its records:
 * strictly ascending.  *n is their count: the call's *nlines / *nrecs, 0 before any call and after a call that handed out nothing.
 * ACG_EAGAIN: max is too small, *n is the number needed.  Nothing is consumed either way; one copy of *n x 8 bytes, no kernel.
 * ACG_ESTATE: that sink is off.
 * THE MERGE.  Keys of different contexts are distinct when their channel numbers are, and each context's are ascending: after one
 * sink call on every context over the same sample span, a k-way merge of (keys, records) by key is the one stream a single context
 * would have handed out in that call.  JSON lines need no offset table for it (a line holds no raw '\n': cJSON escapes it), the
 * text sink hands out its offsets.  As with the flight table's round, a call that returns ACG_EAGAIN has consumed an arbitrary
 * oldest part of the queue: the merge then holds per call, so a host sizes its buffers for a round.
 * ACG_SINK_OUTPUTS: the keys of the most recent acg_drain_outputs / acg_collect_outputs call, ONE list for all its legs (the merge
 * is applied per leg with it); ACG_ESTATE: the outputs are off. */
#define ACG_SINK_JSON  1
#define ACG_SINK_TEXT  2
#define ACG_SINK_OUTPUTS  4      /* (3 stays what it was: ACG_EINVAL) */
int  acg_sink_keys(acg_ctx *ctx, int sink, unsigned long long *keys, int max, int *n);

/* ---- per-channel reception statistics: what the reference says under -v, counted on the device --------------------------------
 * One record per channel, resident on the device across calls and updated in the round trips the entry points above already make
 * (csrc/stats.hip: one launch behind the split / label pass of a message entry point, one of its own in the frame entry points).
 * Every counter is the number of times the reference prints the line named beside it (acars.c, output.c); blocks the repair drops
 * and blocks a filter drops never cross to the host, so this table is the only place they can be told apart.
 *
 * Counting rules.  A block is counted when, and only when, an entry point consumes it: a call that returns ACG_EAGAIN has counted
 * what it handed out or dropped and nothing else, a call that consumes nothing counts nothing, no block is counted twice.  The frame
 * entry points move the block-level fields and `delivered`; the three filter fields move in the message entry points (acg_*_msgs*,
 * acg_*_json, acg_*_text) only.  Blocks lost to a lapped queue (ACG_EOVERFLOW) belong to no channel: they go to `lost_blocks`.
 * After every call  blocks == too_short + parity_many + unfixable + parity_problem + kept, and on a channel consumed through message
 * entry points only  kept == uplink_dropped + label_dropped + empty_dropped + delivered.
 * The counters are 32-bit and WRAP: at ten blocks per second a channel fills one in 13 years.  Every accumulator is an integer add
 * or an integer minimum / maximum, so a snapshot does not depend on the order the device took the blocks in.
 * Not counted: the two resets only the framing sees ("too many parity errors" without a count, acars.c:313, and "too long", :336);
 * they queue no block, and counting them inside the demodulator was not free (profiles/LEDGER.md, "Per-channel reception statistics"). */
typedef struct {
    unsigned int blocks;            /* blocks taken off the queue                          "get message #n"            acars.c:121 */
    unsigned int too_short;         /* dropped: fewer than 13 bytes                        "too short"                 :126 */
    unsigned int parity_many;       /* dropped                                             "too many parity errors: k" :148 */
    unsigned int parity_blocks;     /* "parity error(s): k" lines ...                                                   :154 */
    unsigned int parity_errs;       /* ... and the sum of their k */
    unsigned int crc_errors;        /*                                                     "crc error"                 :167 */
    unsigned int unfixable;         /* dropped                                             "not able to fix errors"    :173, :185 */
    unsigned int fixed;             /* (with parity errors also when the CRC was clean)    "errors fixed"              :178, :190 */
    unsigned int parity_problem;    /* dropped                                             "parity check problem"      :203 */
    unsigned int kept;              /* blocks that reach outputmsg()                                                    :209 */
    unsigned int miss_txt_end;      /* blocks queued by the DEL rule, whatever became of them  "miss txt end"           :326 */
    unsigned int uplink_dropped;    /* dropped by -A, -b, -e: a block is charged to the FIRST filter that drops it, in the */
    unsigned int label_dropped;     /* reference's order (output.c:537, 539, 650)  */
    unsigned int empty_dropped;
    unsigned int delivered;         /* handed to the caller */
    unsigned int reserved;
    double lvl_min, lvl_max;        /* least and greatest MskLvlSum / MskBitCount over kept blocks (acg_host_level_db turns a ratio
                                     * into the dB of acars.c:351); blocks with MskBitCount <= 0 are skipped; 0 and 0 while none */
    long long last_end_sample;      /* end_sample of the newest kept block, -1 while none */
} acg_chan_stats;
/* on = 1: allocates and zeroes the table and starts counting (already on: zeroes); on = 0: stops and frees -- every entry point
 * then issues exactly what it issues without this section.  acg_reset zeroes the table and keeps the switch.  A slot's statistics
 * stay with the slot: acg_set_state does not move them.  ACG_ESTATE: context without ACG_F_REPAIR. */
int  acg_stats_enable(acg_ctx *ctx, int on);
/* Waits for everything issued (like a drain) and copies the records of channels ch0 .. ch0 + n - 1; *lost_blocks (may be null):
 * blocks lost to a lapped queue since the table was zeroed.  ACG_ESTATE while off, ACG_EINVAL: a range outside the context. */
int  acg_stats_read(acg_ctx *ctx, int ch0, int n, acg_chan_stats *out, unsigned long long *lost_blocks);

/* Per-bit records of the LAST process call for one channel (needs ACG_F_BITLOG):
 * vo = the value putbit() receives (msk.c:122-126), lvl = cabsf(v) (msk.c:110). */
int  acg_read_bits(acg_ctx *ctx, int ch, float *vo, float *lvl, int max_bits, int *nbits);
/* all channels at once: counts[nch], vo/lvl [nch][cap] with cap = acg_bit_capacity() */
int  acg_read_bits_all(acg_ctx *ctx, int *counts, float *vo, float *lvl);
int  acg_bit_capacity(const acg_ctx *ctx);
/* dm_buffer of the last call (rtl.c:353), n floats of channel ch */
int  acg_read_dm(acg_ctx *ctx, int ch, float *dm, int n);
int  acg_get_state(acg_ctx *ctx, int ch, acg_chan_state *st);
int  acg_set_state(acg_ctx *ctx, int ch, const acg_chan_state *st);     /* ACG_EINVAL: idx >= 11, blk_len outside 0..241 */
/* the same for channels ch0 .. ch0+n-1 in ONE transfer each way (the legacy view moves all of a dongle's channels per
 * callback: rtl.c:344-360), and dm_buffer of the last call for n channels: row i at dm + i*pitch_floats, nfloats each */
int  acg_get_state_n(acg_ctx *ctx, int ch0, int n, acg_chan_state *st);
int  acg_set_state_n(acg_ctx *ctx, int ch0, int n, const acg_chan_state *st);
int  acg_read_dm_n(acg_ctx *ctx, int ch0, int n, float *dm, size_t pitch_floats, int nfloats);
/* blk->txt of the block channel ch is assembling (acars.c:304 appends to it; blk_len bytes of it are meaningful): the part of
 * channel_t's state that is not a scalar.  A host that moves a channel between slots or contexts in the middle of a block takes
 * it along with acg_get_state / acg_set_state (the legacy view does not need it: there the text lives in the caller's ch->blk).
 * txt: ACG_TXTMAX bytes. */
int  acg_get_block_text(acg_ctx *ctx, int ch, unsigned char *txt);
int  acg_set_block_text(acg_ctx *ctx, int ch, const unsigned char *txt);

/* Replays the bit records of the last call through a putbit()-shaped sink, channel by channel
 * in channel order: for every bit sink(user, ch, vo, lvl).  The legacy shim's sink performs
 * msk.c:112-113 + putbit() on the caller's channel_t, i.e. calls the UNCHANGED decodeAcars(). */
typedef void (*acg_bit_sink)(void *user, int ch, float vo, float lvl);
int  acg_replay_bits(acg_ctx *ctx, acg_bit_sink sink, void *user);

/* ---- timing ------------------------------------------------------------------------------- */
/* Sums of HIP-event-bracketed kernel time since the last call (ACG_F_TIMING), in ms, and the
 * number of launches they cover.  Synchronises. */
int  acg_get_timing(acg_ctx *ctx, double *fir_ms, int *fir_launches, double *msk_ms, int *msk_launches);
/* 0 = no events, 1 = both stages (what ACG_F_TIMING starts with), 2 = down-converter launches only:
 * event records on the demodulator stream sit on its serial launch chain (~10 us per launch). */
int  acg_set_timing(acg_ctx *ctx, int mode);

#ifdef __cplusplus
}
#endif
#endif /* ACARSDEC_AMD_H */
