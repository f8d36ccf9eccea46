"""Host-side mirror of the reference's per-channel interface on top of the C ABI.

Names follow the reference: a Decoder owns `nch` channels (channel_t, acarsdec.h:59-92);
`init_rtl` is initRtl's tap set-up (rtl.c:243-287), `in_callback` is rtl.c:314-361 for all
channels, `demod_msk` is demodMSK (msk.c:67-137) fed from 12.5 kHz samples, frames are the
msgblk_t blocks decodeAcars queues (acars.c:350-364).  Everything numerical happens in
libacarsdec_amd.so on the GPU; this file only marshals pointers.
"""
import ctypes as C

import numpy as np

from . import _capi as K


def _chk(ctx, rc, allow=(), lib=None):
    """lib = the library that owns ctx (a lab-build context must not be handed to the product library's acg_last_error)"""
    if rc != K.OK and rc not in allow:
        msg = (lib or K.load()).acg_last_error(ctx).decode() if ctx else ""
        raise K.AcgError(rc, msg)
    return rc


def rtl_taps(Fr_hz, Fc_hz, decim):
    """wf[] of rtl.c:283-286 as float32 [decim, 2]."""
    out = np.zeros((decim, 2), dtype=np.float32)
    _chk(None, K.load().acg_rtl_taps(int(Fr_hz), int(Fc_hz), int(decim), out.ctypes.data))
    return out


def choose_fc(freqs_hz, decim):
    """chooseFc of rtl.c:131-168. Returns (Fc, sorted freqs)."""
    fd = np.array(freqs_hz, dtype=np.uint32)
    fc = K.load().acg_rtl_choose_fc(fd.ctypes.data, len(fd), int(decim))
    return int(fc), fd


def soapy_taps(Fr_hz, freq_hz, decim):
    """oscillator[] of soapy.c:163-166 as float32 [decim, 2]."""
    out = np.zeros((decim, 2), dtype=np.float32)
    _chk(None, K.load().acg_soapy_taps(float(Fr_hz), int(freq_hz), int(decim), out.ctypes.data))
    return out


def sdrplay_taps(Fr_hz, Fc_hz):
    out = np.zeros((160, 2), dtype=np.float32)
    _chk(None, K.load().acg_sdrplay_taps(float(Fr_hz), int(Fc_hz), out.ctypes.data))
    return out


def airspy_taps(Fr_hz, Fc_hz, inrate):
    out = np.zeros((inrate // K.INTRATE, 2), dtype=np.float32)
    _chk(None, K.load().acg_airspy_taps(int(Fr_hz), int(Fc_hz), int(inrate), out.ctypes.data))
    return out


def airspy_choose_fc(freqs_hz):
    return int(K.load().acg_airspy_choose_fc(int(min(freqs_hz)), int(max(freqs_hz))))


def rate_decim(rate_hz):
    """ceil(rate / 12500): the decim (== ntaps) of a Decoder that takes input at rate_hz (acg_rate_decim)"""
    m = K.load().acg_rate_decim(int(rate_hz))
    if m < 0:
        raise K.AcgError(m, "acg_rate_decim(%d)" % int(rate_hz))
    return m


def rate_taps(rate_hz, offset_hz, n=None):
    """The bare oscillator of a channel offset_hz above the centre at input rate rate_hz, float32 [n, 2] (n: rate_decim):
    (cos, -sin) of 2 pi frac(offset_hz i / rate_hz).  The rate kernel divides by the window's own length."""
    n = rate_decim(rate_hz) if n is None else int(n)
    out = np.zeros((n, 2), dtype=np.float32)
    _chk(None, K.load().acg_rate_taps(int(rate_hz), float(offset_hz), n, out.ctypes.data))
    return out


def channel_filter_taps(rate_hz, offset_hz, nseg, cutoff_hz=6250.0, beta=7.0):
    """A channel filter over nseg windows for Decoder.set_channel_filter, float32 [nseg * decim, 2]: a Kaiser-windowed sinc (-6 dB
    at cutoff_hz, DC gain 1) times the oscillator of a channel offset_hz above the centre; rate_hz a multiple of 12 500
    (acg_channel_filter_taps)."""
    if int(rate_hz) % K.INTRATE:
        raise K.AcgError(K.EINVAL, "channel_filter_taps: the rate must be a multiple of 12 500 Hz")
    out = np.zeros((max(int(nseg), 0) * (int(rate_hz) // K.INTRATE), 2), dtype=np.float32)
    _chk(None, K.load().acg_channel_filter_taps(int(rate_hz), float(offset_hz), int(nseg), float(cutoff_hz), float(beta), out.ctypes.data))
    return out


def rate_window_starts(rate_hz, k0, n):
    """s_k0 .. s_(k0 + n) of the window grid s_k = floor(k P / Q), P / Q = rate_hz / 12500: uint64 [n + 1]"""
    out = np.zeros(int(n) + 1, dtype=np.uint64)
    _chk(None, K.load().acg_rate_window_starts(int(rate_hz), int(k0), int(n), out.ctypes.data))
    return out


def parse_freq_mhz(s):
    """rtl.c:245-247: command-line MHz string -> Hz rounded to the 12.5 kHz raster."""
    return (int(1000000 * float(s) + K.INTRATE / 2) // K.INTRATE) * K.INTRATE


class Decoder:
    def __init__(self, nch, decim=160, ntaps=None, nstreams=None, max_blocks=1, device=0,
                 bitlog=True, timing=False, repair=False, exact_fir=False, max_lag=0, lab=False, precise_mixer=False):
        self.L = K.load(lab)          # lab=True: the lab build of the library (measurement variants; tests and probes only)
        self.nch, self.decim = int(nch), int(decim)
        self.ntaps = int(ntaps if ntaps is not None else decim)
        self.nstreams = int(nstreams if nstreams is not None else nch)
        self.max_blocks = int(max_blocks)
        cfg = K.Config(device, self.nch, self.nstreams, self.decim, self.ntaps, self.max_blocks,
                       (K.F_BITLOG if bitlog else 0) | (K.F_TIMING if timing else 0) | (K.F_REPAIR if repair else 0) |
                       (K.F_EXACT_FIR if exact_fir else 0) | (K.F_PRECISE_MIXER if precise_mixer else 0), int(max_lag))
        self.ctx = C.c_void_p()
        rc = self.L.acg_create(C.byref(self.ctx), C.byref(cfg))
        if rc != K.OK:
            raise K.AcgError(rc, "acg_create")
        self.timing_flag = bool(timing)
        self.bit_cap = self.L.acg_bit_capacity(self.ctx)
        self.max_lag = self.L.acg_max_lag(self.ctx)
        self.Fc = None

    def _chk(self, rc, allow=()):
        return _chk(self.ctx, rc, allow, self.L)

    def close(self):
        if self.ctx:
            self.L.acg_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- set-up -------------------------------------------------------------------------
    def reset(self):
        self._chk(self.L.acg_reset(self.ctx))

    def set_taps(self, taps, ch0=0):
        taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1, self.ntaps, 2)
        self._chk(self.L.acg_set_taps(self.ctx, ch0, taps.shape[0], taps.ctypes.data))

    def set_channel_streams(self, stream_of):
        a = np.ascontiguousarray(stream_of, dtype=np.int32)
        assert a.size == self.nch
        self._chk(self.L.acg_set_channel_streams(self.ctx, a.ctypes.data))

    def init_rtl(self, freqs_mhz):
        """One dongle, nch channels sharing its stream: rtl.c:243-287.  Returns Fc."""
        assert len(freqs_mhz) == self.nch
        fr = [parse_freq_mhz(f) for f in freqs_mhz]
        fc, _ = choose_fc(fr, self.decim)
        if fc == 0:
            raise ValueError("Frequencies too far apart")          # rtl.c:150
        self.set_taps(np.stack([rtl_taps(f, fc, self.decim) for f in fr]))
        self.Fc = fc
        return fc

    # ---- hot path -----------------------------------------------------------------------
    @staticmethod
    def _ptr(x):
        """(pointer, is_device) of a numpy array or a torch tensor."""
        if hasattr(x, "data_ptr"):
            return x.data_ptr(), bool(x.is_cuda)
        return x.ctypes.data, False

    def in_callback(self, iq, nblocks=None, pitch=None, stream=None):
        """in_callback() for all channels.  iq: uint8, [nstreams, nblocks*1024*decim*2] (numpy = host,
        torch cuda tensor = device, asynchronous on `stream`)."""
        row = K.BLOCK * self.decim * 2
        if hasattr(iq, "data_ptr"):
            nbytes_row = iq.shape[-1] if iq.dim() > 1 else iq.numel() // self.nstreams
            pitch = pitch or (iq.stride(0) if iq.dim() > 1 else nbytes_row)
        else:
            iq = np.ascontiguousarray(iq, dtype=np.uint8).reshape(self.nstreams, -1)
            nbytes_row = iq.shape[1]
            pitch = pitch or nbytes_row
        nblocks = nblocks or nbytes_row // row
        p, dev = self._ptr(iq)
        if dev:
            self._chk(self.L.acg_process_iq_u8_dev(self.ctx, p, pitch, nblocks, stream))
        else:
            self._chk(self.L.acg_process_iq_u8_host(self.ctx, p, pitch, nblocks))

    def feed(self, fmt, samples, q_plane=None):
        """Host samples of any length (the SDR drivers' shape): [nstreams, n] int16 pairs / planes / float32; the recordings'
        formats: int8 pairs (FMT_CS8), float32 pairs or complex64 (FMT_CF32)."""
        if fmt == K.FMT_CS8:
            a = np.ascontiguousarray(samples, dtype=np.int8).reshape(self.nstreams, -1)
            n, pitch = a.shape[1] // 2, a.shape[1] // 2
        elif fmt == K.FMT_CF32:
            a = np.asarray(samples)
            a = np.ascontiguousarray(a, dtype=np.complex64 if np.iscomplexobj(a) else np.float32).reshape(self.nstreams, -1)
            a = a.view(np.float32)
            n, pitch = a.shape[1] // 2, a.shape[1] // 2
        elif fmt == K.FMT_CS16:
            a = np.ascontiguousarray(samples, dtype=np.int16).reshape(self.nstreams, -1)
            n, pitch = a.shape[1] // 2, a.shape[1] // 2
        elif fmt == K.FMT_S16_SPLIT:
            a = np.ascontiguousarray(samples, dtype=np.int16).reshape(self.nstreams, -1)
            q_plane = np.ascontiguousarray(q_plane, dtype=np.int16).reshape(self.nstreams, -1)
            n, pitch = a.shape[1], a.shape[1]
        else:
            a = np.ascontiguousarray(samples, dtype=np.float32).reshape(self.nstreams, -1)
            n, pitch = a.shape[1], a.shape[1]
        self._chk(self.L.acg_feed_samples_host(self.ctx, fmt, a.ctypes.data,
                                                     q_plane.ctypes.data if q_plane is not None else None, pitch, n))

    # ---- any input rate (acg_set_input_rate, acg_process_rate_dev, acg_feed_rate_host) ------------------------------------
    _RATE_DTYPES = {K.FMT_CU8: np.uint8, K.FMT_CS8: np.int8, K.FMT_CS16: np.int16, K.FMT_CF32: np.float32}

    def set_input_rate(self, rate_hz):
        """Input at rate_hz from now on, windows on the grid s_k = floor(k rate / 12500) (needs decim == ntaps ==
        rate_decim(rate_hz) and taps as rate_taps makes them); 0: whole windows of decim samples again.  Restarts the grid."""
        self._chk(self.L.acg_set_input_rate(self.ctx, int(rate_hz)))

    def set_channel_filter(self, taps):
        """A channel filter over several windows on the rate path (rate a multiple of 12 500 Hz): float32 [nch, nseg * decim, 2] as
        channel_filter_taps makes them, index 0 for the oldest sample, nseg = 2 .. 4 from the shape; None: off.  Restarts the
        grid and empties the history.  The filter's centre lies (nseg - 1) / 2 output samples earlier than the boxcar's."""
        if taps is None:
            self._chk(self.L.acg_set_channel_filter(self.ctx, 0, None))
            return
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        assert taps.ndim == 3 and taps.shape[0] == self.nch and taps.shape[2] == 2 and taps.shape[1] % self.decim == 0, taps.shape
        self._chk(self.L.acg_set_channel_filter(self.ctx, taps.shape[1] // self.decim, taps.ctypes.data))

    def process_rate(self, fmt, dev_tensor, nsamples, pitch, stream=None):
        """Device rows of nsamples samples that begin at the current window start; pitch in bytes.  Returns (nwin, consumed): the
        whole windows run and the samples they covered -- present the rest again at the head of the next call."""
        nwin, used = C.c_int(0), C.c_size_t(0)
        self._chk(self.L.acg_process_rate_dev(self.ctx, int(fmt), dev_tensor.data_ptr(), int(pitch), int(nsamples), stream,
                                              C.byref(nwin), C.byref(used)))
        return nwin.value, used.value

    def feed_rate(self, fmt, samples):
        """Host samples of any length at the rate set: [nstreams, n] pairs of uint8 (FMT_CU8), int8, int16, float32 (or
        complex64 for FMT_CF32)."""
        a = np.asarray(samples)
        dt = np.complex64 if (fmt == K.FMT_CF32 and np.iscomplexobj(a)) else self._RATE_DTYPES[fmt]
        a = np.ascontiguousarray(a, dtype=dt).reshape(self.nstreams, -1)
        n = a.shape[1] if dt is np.complex64 else a.shape[1] // 2
        self._chk(self.L.acg_feed_rate_host(self.ctx, int(fmt), a.ctypes.data, n, n))

    def process_samples(self, fmt, dev_tensor, nblocks, pitch, plane=0, stream=None):
        self._chk(self.L.acg_process_samples_dev(self.ctx, fmt, dev_tensor.data_ptr(), pitch, plane, nblocks, stream))

    def fir_only(self, iq_dev, nblocks, pitch, stream=None):
        self._chk(self.L.acg_fir_only_dev(self.ctx, iq_dev.data_ptr(), pitch, nblocks, stream))

    def placement_trial(self, iq_dev, nblocks, pitch, repeats=2, stream=None):
        """ms per in_callback-sized call on this decoder's placement (acg_placement_trial); the decoder comes back reset."""
        ms = C.c_double(0)
        self._chk(self.L.acg_placement_trial(self.ctx, iq_dev.data_ptr(), pitch, nblocks, repeats, stream, C.byref(ms)))
        return ms.value

    def placement_trial_samples(self, fmt, dev_tensor, nblocks, pitch, plane=0, repeats=2, stream=None):
        """the same for a sample-format input (acg_placement_trial_samples)"""
        ms = C.c_double(0)
        self._chk(self.L.acg_placement_trial_samples(self.ctx, fmt, dev_tensor.data_ptr(), pitch, plane, nblocks, repeats, stream, C.byref(ms)))
        return ms.value

    def launch_shape(self, nblocks):
        """The down-converter launch the library makes for one launch of nblocks callbacks (acg_lab_fir_launch_shape), as a
        K.LaunchShape: kernel (0 vector pipe, 1 fir_u8_mm_kernel, 2 fir_u8_mm1_kernel), stages, runs, tiles_per_run, waves ..."""
        s = K.LaunchShape()
        self._chk(self.L.acg_lab_fir_launch_shape(self.ctx, int(nblocks), C.byref(s)))
        return s

    def samples_launch(self, fmt, nblocks):
        """The kernel family one launch of nblocks callbacks of sample format fmt takes (acg_lab_samples_launch_shape), as a
        K.SamplesLaunch: family (K.FIR_STREAMING / FIR_WORKGROUP / FIR_MATRIX / FIR_SHARED_VECTOR), tile_windows, runs, waves ..."""
        s = K.SamplesLaunch()
        self._chk(self.L.acg_lab_samples_launch_shape(self.ctx, int(fmt), int(nblocks), C.byref(s)))
        return s

    def set_stream_counters(self, nsamp_total, nbit_total, ch0=0, n=None):
        """Test hook (acg_lab_set_stream_counters): right after reset, channels ch0 .. ch0+n-1 (default: all from ch0) count their
        samples and bits from these values on, as after days of uptime."""
        n = self.nch - ch0 if n is None else n
        self._chk(self.L.acg_lab_set_stream_counters(self.ctx, int(ch0), int(n), int(nsamp_total), int(nbit_total)))

    def demod_msk(self, dm):
        """demodMSK() for all channels from 12.5 kHz samples: dm float32 [nch, len]."""
        dm = np.ascontiguousarray(dm, dtype=np.float32)
        dm = dm.reshape(self.nch, dm.size // self.nch)
        self._chk(self.L.acg_process_dm_host(self.ctx, dm.ctypes.data, dm.shape[1], dm.shape[1]))

    def feed_pcm(self, frames):
        """demodMSK() for all channels from interleaved frames as a sound file or a sound card delivers them: numpy [nframes, nch],
        int16 (PCM16, scaled by 1/32768 on the device) or float32, C-contiguous, any nframes (acg_feed_pcm_host)."""
        if not isinstance(frames, np.ndarray) or frames.dtype not in (np.int16, np.float32):
            raise TypeError("frames: a numpy array of int16 or float32")
        if frames.ndim != 2 or frames.shape[1] != self.nch or not frames.flags["C_CONTIGUOUS"]:
            raise ValueError("frames: C-contiguous [nframes, %d]" % self.nch)
        fmt = K.PCM_S16 if frames.dtype == np.int16 else K.PCM_F32
        self._chk(self.L.acg_feed_pcm_host(self.ctx, fmt, frames.ctypes.data, frames.shape[0]))

    def process_pcm(self, dev_tensor, fmt, nframes, stream=None):
        """The same from a device tensor of nframes * nch interleaved elements (K.PCM_S16 / K.PCM_F32), nframes <= max_blocks * 1024,
        asynchronous on `stream` (acg_process_pcm_dev)."""
        self._chk(self.L.acg_process_pcm_dev(self.ctx, int(fmt), dev_tensor.data_ptr(), int(nframes), stream))

    def sync(self):
        self._chk(self.L.acg_sync(self.ctx))

    # ---- results ------------------------------------------------------------------------
    def drain_frames(self, max_frames=4096):
        """Blocks completed since the last drain as a list of ctypes Frame objects (loops while the C side says ACG_EAGAIN)."""
        out = []
        while True:
            n, buf, more = self._frames_call(self.L.acg_drain_frames, max_frames)
            out += [K.Frame.from_buffer_copy(buf[i]) for i in range(n)]      # copies: the array is reused
            if not more:
                return out

    def _frames_call(self, fn, max_frames, *lead):
        max_frames = max(1, int(max_frames))          # (a zero-length buffer would make every EAGAIN loop spin without progress)
        if getattr(self, "_fbuf_cap", 0) < max_frames:
            self._fbuf = (K.Frame * max_frames)()
            self._fbuf_cap = max_frames
        n = C.c_int(0)
        rc = self._chk(fn(self.ctx, *lead, self._fbuf, self._fbuf_cap, C.byref(n)), allow=(K.EAGAIN,))
        return n.value, self._fbuf, rc == K.EAGAIN

    def drain_frames_raw(self, max_frames=4096):
        """(count, ctypes array): no per-block Python objects; the array is reused by the next call.  Blocks beyond
        max_frames stay queued (the next drain / collect hands them out)."""
        n, buf, _ = self._frames_call(self.L.acg_drain_frames, max_frames)
        return n, buf

    def collect_frames_raw(self, lag=1, max_frames=4096):
        """Streaming drain: blocks of all calls but the `lag` newest; waits only for those calls."""
        n, buf, _ = self._frames_call(self.L.acg_collect_frames, max_frames, lag)
        return n, buf

    def _msg_buf(self, max_msgs):
        if getattr(self, "_mbuf_cap", 0) < max_msgs:
            self._mbuf = (K.Msg * max_msgs)()
            self._mbuf_cap = max_msgs
        return self._mbuf

    def drain_msgs(self, max_msgs=4096, oooi=False, reasm=False):
        """outputmsg()'s field split of every block completed since the last drain (needs repair=True): K.Msg records.
        The C side hands out the oldest messages that fit and says ACG_EAGAIN ("call again, nothing lost") while more are
        queued: this wrapper calls again until the queue is empty, so the list is complete whatever max_msgs is (per call the
        records are ordered by (chn, end_bit); across calls the order is completion order).
        oooi=True: (K.Msg, K.Oooi) pairs from acg_drain_msgs_oooi (the labels decoded on the device).
        reasm=True (after reasm_enable): (K.Msg, status) pairs from acg_drain_msgs_reasm, status one of K.REASM_*; with oooi=True
        (K.Msg, K.Oooi, status) triples."""
        if reasm:
            return self._msgs_reasm(self.L.acg_drain_msgs_reasm, max_msgs, oooi)
        if oooi:
            return self._msgs_oooi(self.L.acg_drain_msgs_oooi, max_msgs)
        buf = self._msg_buf(max(1, max_msgs))
        out = []
        while True:
            n = C.c_int(0)
            rc = self._chk(self.L.acg_drain_msgs(self.ctx, buf, self._mbuf_cap, C.byref(n)), allow=(K.EAGAIN,))
            out += [K.Msg.from_buffer_copy(buf[i]) for i in range(n.value)]
            if rc == K.OK:
                return out

    def drain_msgs_raw(self, max_msgs=4096):
        """(count, ctypes array, more): one acg_drain_msgs call, no per-message Python objects"""
        buf = self._msg_buf(max(1, max_msgs))
        n = C.c_int(0)
        rc = self._chk(self.L.acg_drain_msgs(self.ctx, buf, self._mbuf_cap, C.byref(n)), allow=(K.EAGAIN,))
        return n.value, buf, rc == K.EAGAIN

    def collect_msgs_raw(self, lag=1, max_msgs=4096):
        """Streaming variant (acg_collect_msgs): (count, ctypes array, more) -- messages of all calls but the `lag` newest; `more`
        is True when the buffer was too small and the rest stays queued for the next collect (nothing is lost)."""
        buf = self._msg_buf(max(1, max_msgs))
        n = C.c_int(0)
        rc = self._chk(self.L.acg_collect_msgs(self.ctx, lag, buf, self._mbuf_cap, C.byref(n)), allow=(K.EAGAIN,))
        return n.value, buf, rc == K.EAGAIN

    def collect_msgs(self, lag=1, max_msgs=4096, oooi=False, reasm=False):
        """list of K.Msg of all calls but the `lag` newest (loops while the C side says "call again"); oooi=True: (K.Msg, K.Oooi)
        pairs from acg_collect_msgs_oooi; reasm=True: as drain_msgs, from acg_collect_msgs_reasm"""
        if reasm:
            return self._msgs_reasm(self.L.acg_collect_msgs_reasm, max_msgs, oooi, lag)
        if oooi:
            return self._msgs_oooi(self.L.acg_collect_msgs_oooi, max_msgs, lag)
        out = []
        while True:
            n, buf, more = self.collect_msgs_raw(lag, max_msgs)
            out += [K.Msg.from_buffer_copy(buf[i]) for i in range(n)]
            if not more:
                return out

    # ---- the sink's filters and label decoding (acg_set_msg_filter, acg_*_msgs_oooi) -------------------------------------
    def set_msg_filter(self, downlink_only=False, skip_empty=False, labels=None):
        """The CLI's -A (downlink_only), -e (skip_empty) and -b (labels: a list of labels or a -b string "H1:Q1") for every
        message entry point from now on.  All defaults = no filter (what a new context has)."""
        if not downlink_only and not skip_empty and labels is None:
            self._chk(self.L.acg_set_msg_filter(self.ctx, None))
            return
        f = make_msg_filter(downlink_only, skip_empty, labels, self.L)
        self._chk(self.L.acg_set_msg_filter(self.ctx, C.byref(f)))

    def _msgs_oooi(self, fn, max_msgs, *lead):
        max_msgs = max(1, int(max_msgs))
        if getattr(self, "_obuf_cap", 0) < max_msgs:
            self._obuf = (K.Oooi * max_msgs)()
            self._obuf_cap = max_msgs
        buf = self._msg_buf(max_msgs)
        cap = min(self._mbuf_cap, self._obuf_cap)
        out = []
        while True:
            n = C.c_int(0)
            rc = self._chk(fn(self.ctx, *lead, buf, self._obuf, cap, C.byref(n)), allow=(K.EAGAIN,))
            out += [(K.Msg.from_buffer_copy(buf[i]), K.Oooi.from_buffer_copy(self._obuf[i])) for i in range(n.value)]
            if rc == K.OK:
                return out

    # ---- per-channel reception statistics (acg_stats_enable, acg_stats_read) ----------------------------------------------
    def enable_stats(self):
        """Starts (or zeroes) the per-channel statistics: the events the reference reports under -v, counted on the device over
        the blocks every entry point consumes from now on (needs repair=True)."""
        self._chk(self.L.acg_stats_enable(self.ctx, 1))

    def disable_stats(self):
        self._chk(self.L.acg_stats_enable(self.ctx, 0))

    def stats(self, ch0=0, n=None):
        """(table, lost_blocks): the records of channels ch0 .. ch0 + n - 1 (default: all from ch0) as a numpy structured array
        of K.CHAN_STATS_DTYPE, and the blocks lost to a lapped queue.  Waits for everything issued, like a drain."""
        n = self.nch - int(ch0) if n is None else int(n)
        out = np.zeros(max(n, 0), dtype=K.CHAN_STATS_DTYPE)
        lost = C.c_ulonglong(0)
        self._chk(self.L.acg_stats_read(self.ctx, int(ch0), n, out.ctypes.data, C.byref(lost)))
        return out, int(lost.value)

    # ---- the flight table (acg_flights_enable, acg_flight_snapshot, acg_drain_routes) --------------------------------------
    def enable_flights(self, t0=0.0, mdly=600, max_flights=4096):
        """addFlight() / routejson() (output.c:361-456) on the device for every message entry point from now on.  t0: wall clock
        of the first sample since reset, seconds (a float) or (sec, usec); mdly: the CLI's -t; max_flights: capacity (rounded up
        to a power of two).  The table starts empty."""
        sec, usec = t0 if isinstance(t0, tuple) else (int(t0 // 1), int(round((t0 - t0 // 1) * 1e6)))
        if usec >= 1000000:
            sec, usec = sec + 1, usec - 1000000
        cfg = K.FlightConfig(int(sec), int(usec), int(mdly), int(max_flights))
        self._chk(self.L.acg_flights_enable(self.ctx, C.byref(cfg)))
        self.flights_dropped = 0

    def disable_flights(self):
        self._chk(self.L.acg_flights_enable(self.ctx, None))

    def flights(self):
        """The live entries as a list of K.Flight, latest update first (printmonitor()'s order); self.flights_dropped = new
        aircraft that found no slot since enable / reset."""
        cap = getattr(self, "_flbuf_cap", 0) or 256
        while True:
            if getattr(self, "_flbuf_cap", 0) < cap:
                self._flbuf = (K.Flight * cap)()
                self._flbuf_cap = cap
            n, dropped = C.c_int(0), C.c_int(0)
            rc = self._chk(self.L.acg_flight_snapshot(self.ctx, self._flbuf, self._flbuf_cap, C.byref(n), C.byref(dropped)), allow=(K.EAGAIN,))
            if rc == K.OK:
                self.flights_dropped = dropped.value
                return [K.Flight.from_buffer_copy(self._flbuf[i]) for i in range(n.value)]
            cap = max(n.value, 2 * cap)

    def drain_routes(self, max_routes=1024):
        """The route records emitted so far (K.Route), in the order of their triggering messages."""
        buf = (K.Route * max(1, int(max_routes)))()
        out = []
        while True:
            n = C.c_int(0)
            rc = self._chk(self.L.acg_drain_routes(self.ctx, buf, len(buf), C.byref(n)), allow=(K.EAGAIN,))
            out += [K.Route.from_buffer_copy(buf[i]) for i in range(n.value)]
            if rc == K.OK:
                return out

    # ---- reassembly of multi-block messages (acg_reasm_enable, acg_*_msgs_reasm, acg_drain_reassembled) ----------------------
    def reasm_enable(self, t0=0.0, max_msgs=0, max_text=0):
        """The reassembly table (ETB chains, libacars' assstat) on the device for every message entry point from now on.  t0 as
        in enable_flights; max_msgs: chains in progress the table holds (0: 1024); max_text: bytes of a complete text, a multiple of
        16 (0: 3584).  The table starts empty."""
        sec, usec = t0 if isinstance(t0, tuple) else (int(t0 // 1), int(round((t0 - t0 // 1) * 1e6)))
        if usec >= 1000000:
            sec, usec = sec + 1, usec - 1000000
        cfg = K.ReasmConfig(int(sec), int(usec), int(max_msgs), int(max_text))
        self._chk(self.L.acg_reasm_enable(self.ctx, C.byref(cfg)))
        self._reasm_text = int(max_text) or 3584
        self.reasm_dropped = 0

    def reasm_disable(self):
        self._chk(self.L.acg_reasm_enable(self.ctx, None))

    def _msgs_reasm(self, fn, max_msgs, oooi, *lead):
        max_msgs = max(1, int(max_msgs))
        buf = self._msg_buf(max_msgs)
        cap = self._mbuf_cap
        obuf = (K.Oooi * cap)() if oooi else None
        st = (C.c_ubyte * cap)()
        out = []
        while True:
            n = C.c_int(0)
            rc = self._chk(fn(self.ctx, *lead, buf, obuf, st, cap, C.byref(n)), allow=(K.EAGAIN,))
            for i in range(n.value):
                m = K.Msg.from_buffer_copy(buf[i])
                out.append((m, K.Oooi.from_buffer_copy(obuf[i]), int(st[i])) if oooi else (m, int(st[i])))
            if rc == K.OK:
                return out

    def drain_reassembled(self, max_msgs=1024, cap=None):
        """The completed messages so far, in the order of their final fragments: a list of (K.ReasmMsg, text bytes);
        self.reasm_dropped = chains that found no slot since enable / reset.  cap: bytes of text taken per call of the C side
        (default max_msgs texts of the longest kind; at least one always fits)."""
        max_msgs = max(1, int(max_msgs))
        cap = max(int(cap) if cap is not None else max_msgs * self._reasm_text, self._reasm_text)
        buf = (K.ReasmMsg * max_msgs)()
        text = C.create_string_buffer(cap)
        out = []
        while True:
            n, dropped, nbytes = C.c_int(0), C.c_int(0), C.c_size_t(0)
            rc = self._chk(self.L.acg_drain_reassembled(self.ctx, buf, max_msgs, C.byref(n), text, cap, C.byref(nbytes), C.byref(dropped)), allow=(K.EAGAIN,))
            self.reasm_dropped = dropped.value
            for i in range(n.value):
                r = K.ReasmMsg.from_buffer_copy(buf[i])
                out.append((r, text.raw[r.text_off:r.text_off + r.text_len]))
            if rc == K.OK:
                return out

    def reasm_status_name(self, status):
        """libacars' name of a K.REASM_* value ("in progress", "complete", ...), what the reference prints as assstat"""
        return self.L.acg_reasm_status_name(int(status)).decode()

    # ---- one flight table for the channels of several decoders (acg_flights_set_channels / _export / _import / _commit) -----
    def set_flight_channels(self, chn=None):
        """The channel number the table records for each local channel (None: the local index).  For `c mod N` sharding:
        shard.flight_channel_map(nch, rank, world)."""
        if chn is None:
            return self._chk(self.L.acg_flights_set_channels(self.ctx, None))
        arr = np.ascontiguousarray(np.asarray(chn, dtype=np.int32))
        if arr.shape != (self.nch,):
            raise ValueError("one channel number per local channel")
        self._chk(self.L.acg_flights_set_channels(self.ctx, arr.ctypes.data))

    def export_flights(self, on=True):
        """A peer of a shared table: the message entry points queue this decoder's flight events instead of applying them."""
        self._chk(self.L.acg_flights_export(self.ctx, 1 if on else 0))

    def drain_flight_events(self, max_events=4096):
        """The events exported so far, a numpy structured array of K.FLIGHT_EVENT_DTYPE (88 bytes a record), in any order."""
        buf = np.zeros(max(1, int(max_events)), dtype=K.FLIGHT_EVENT_DTYPE)
        parts = []
        while True:
            n = C.c_int(0)
            rc = self._chk(self.L.acg_drain_flight_events(self.ctx, buf.ctypes.data, len(buf), C.byref(n)), allow=(K.EAGAIN,))
            parts.append(buf[:n.value].copy())
            if rc == K.OK:
                return np.concatenate(parts)

    def import_flight_events(self, events):
        """The owner of a shared table: events of other decoders (arrays as drain_flight_events / shard.gather_flight_events hand
        them out), applied by the next message entry point together with this decoder's own."""
        ev = np.ascontiguousarray(np.asarray(events, dtype=K.FLIGHT_EVENT_DTYPE))
        self._chk(self.L.acg_flights_import(self.ctx, ev.ctypes.data if len(ev) else None, len(ev)))

    def commit_flights(self):
        """A pass over the imported events alone (an owner without channels of its own, the end of a run)."""
        self._chk(self.L.acg_flights_commit(self.ctx))

    # ---- the flight table's text (acg_flight_text_enable, acg_flight_monitor_text, acg_drain_routes_json) -------------------
    def enable_flight_text(self, nbch, station_id=""):
        """printmonitor()'s screen and routejson()'s lines (output.c:428-484) rendered on the device from the flight table, which
        must be on.  nbch: the mask columns (0..16, the reference's nbch); station_id: the CLI's -i ("" = no key in a route line)."""
        sid = station_id if isinstance(station_id, bytes) else str(station_id).encode("latin1")
        self._chk(self.L.acg_flight_text_enable(self.ctx, C.byref(K.FlightTextConfig(int(nbch), sid))))

    def disable_flight_text(self):
        self._chk(self.L.acg_flight_text_enable(self.ctx, None))

    def _all_or_nothing(self, call, cap):
        """bytes of an entry point that says ACG_EAGAIN and the bytes needed when its buffer is too small; (bytes, records)"""
        while True:
            if getattr(self, "_ftbuf_cap", 0) < cap:
                self._ftbuf = C.create_string_buffer(cap)
                self._ftbuf_cap = cap
            nb, n = C.c_size_t(0), C.c_int(0)
            rc = self._chk(call(self._ftbuf, self._ftbuf_cap, C.byref(nb), C.byref(n)), allow=(K.EAGAIN,))
            if rc == K.OK:
                return self._ftbuf.raw[:nb.value], n.value
            cap = max(nb.value, cap + 1)

    def monitor_text(self, soh_sample=-1):
        """One monitor frame (bytes), as the reference prints it for a message whose soh_sample is given (-1: the newest live
        entry's last time); self.monitor_rows_n = its rows, self.flights_dropped as flights()."""
        dropped = C.c_int(0)
        call = lambda buf, cap, nb, n: self.L.acg_flight_monitor_text(self.ctx, int(soh_sample), buf, cap, nb, n, C.byref(dropped))
        out, self.monitor_rows_n = self._all_or_nothing(call, K.MONITOR_HDR_LEN + 64 * K.MONITOR_ROW_MAX)
        self.flights_dropped = dropped.value
        return out

    def drain_routes_json(self):
        """The route lines queued so far (bytes, each ended by a newline), in the order of their triggering messages; the queue is
        emptied.  self.route_lines_n = how many."""
        call = lambda buf, cap, nb, n: self.L.acg_drain_routes_json(self.ctx, buf, cap, nb, n)
        out, self.route_lines_n = self._all_or_nothing(call, 64 * K.ROUTE_LINE_MAX)
        return out

    # ---- sharded hosts: global channel numbers and the sinks' order keys (acg_set_channel_numbers, acg_sink_keys) ----------
    def set_channel_numbers(self, chn=None):
        """The number handed out for each local channel (slot) in frames, messages, JSON lines, text records, their order and
        (unless set_flight_channels gave it a map of its own) the flight table; None: the slot's own, the default.  Distinct
        values in 0 .. 2^20 - 1.  For `c mod N` sharding: shard.channel_numbers(nch, rank, world).  Per-slot tables (freqs_hz,
        stats, state, taps) stay indexed by the slot.  Blocks already queued are numbered by the map in force when they are
        handed out."""
        if chn is None:
            return self._chk(self.L.acg_set_channel_numbers(self.ctx, None))
        arr = np.ascontiguousarray(np.asarray(chn, dtype=np.int32))
        if arr.shape != (self.nch,):
            raise ValueError("one channel number per local channel")
        self._chk(self.L.acg_set_channel_numbers(self.ctx, arr.ctypes.data))

    def _c_sink_keys(self, sink):
        """acg_sink_keys: the keys of the records the sink's most recent C call handed out, a uint64 array"""
        n = C.c_int(0)
        buf = np.zeros(max(1, getattr(self, "_kbuf_n", 0)), dtype=np.uint64)
        rc = self._chk(self.L.acg_sink_keys(self.ctx, sink, buf.ctypes.data, len(buf), C.byref(n)), allow=(K.EAGAIN,))
        if rc == K.EAGAIN:
            self._kbuf_n = n.value
            buf = np.zeros(n.value, dtype=np.uint64)
            self._chk(self.L.acg_sink_keys(self.ctx, sink, buf.ctypes.data, len(buf), C.byref(n)))
        return buf[:n.value].copy()

    def _keep_keys(self, kind, parts):
        """a drain / collect that looped over several C calls keeps the keys of the earlier ones: sink_keys then covers them all"""
        if not hasattr(self, "_keys_kept"):
            self._keys_kept = {}
        self._keys_kept[kind] = np.concatenate(parts + [self._c_sink_keys(SINK_KINDS[kind])]) if parts else None

    def sink_keys(self, kind):
        """The order keys (numpy uint64: channel number handed out << 44 | end_bit) of the records the most recent drain_json /
        collect_json (kind "json"), drain_text / collect_text ("text") or drain_outputs / collect_outputs ("outputs": one list
        for all legs) returned, one per record in their order.  Ascending within a C call; several decoders' (keys, records) go
        to shard.merge_keyed.  Empty before any such call."""
        if kind not in SINK_KINDS:
            raise ValueError("kind is 'json', 'text' or 'outputs'")
        kept = getattr(self, "_keys_kept", {}).get(kind)
        return kept if kept is not None else self._c_sink_keys(SINK_KINDS[kind])

    # ---- the JSON sink (acg_json_enable, acg_drain_json, acg_collect_json) -------------------------------------------------
    def enable_json(self, t0, station_id="", app_name="acarsdec", app_ver="", freqs_hz=None):
        """buildjson()'s lines (output.c:227-324, what -o 4 prints) rendered on the device from now on.  t0: wall clock of the
        first sample since reset, (sec, usec) or seconds as a float, 10^9 <= sec < 4 * 10^9; station_id: the CLI's -i ("" = no
        key); app_name / app_ver: the "app" object; freqs_hz: the channels' frequencies in Hz (None = 0, "0.000")."""
        cfg = json_config(t0, station_id, app_name, app_ver)
        fr = None
        if freqs_hz is not None:
            fr = np.ascontiguousarray(freqs_hz, dtype=np.int32)
            assert fr.size == self.nch
        self._chk(self.L.acg_json_enable(self.ctx, C.byref(cfg), fr.ctypes.data if fr is not None else None))

    def disable_json(self):
        self._chk(self.L.acg_json_enable(self.ctx, None, None))

    def _json_call(self, fn, max_lines, *lead):
        cap = max(1, int(max_lines)) * K.JSON_LINE_MAX
        if getattr(self, "_jbuf_cap", 0) < cap:
            self._jbuf = C.create_string_buffer(cap)
            self._jbuf_cap = cap
        out = []
        keys = []                                    # of the C calls that said "call again" (sink_keys)
        while True:
            nb, nl = C.c_size_t(0), C.c_int(0)
            rc = self._chk(fn(self.ctx, *lead, self._jbuf, self._jbuf_cap, C.byref(nb), C.byref(nl)), allow=(K.EAGAIN,))
            out.append(C.string_at(self._jbuf, nb.value))
            if rc == K.OK:
                self._keep_keys("json", keys)
                return b"".join(out)
            keys.append(self._c_sink_keys(K.SINK_JSON))

    def drain_json(self, max_lines=4096):
        """The JSON lines of every block completed since the last drain (needs repair=True and enable_json), as bytes: one object
        per kept message, each ended by a newline, in (chn, end_bit) order per C call; loops while the C side says ACG_EAGAIN."""
        return self._json_call(self.L.acg_drain_json, max_lines)

    def collect_json(self, lag=1, max_lines=4096):
        """Streaming variant (acg_collect_json): the lines of all calls but the `lag` newest"""
        return self._json_call(self.L.acg_collect_json, max_lines, lag)

    def json_level_guard(self):
        """lines rendered since enable_json whose level lay within 8 ulp of a float rounding boundary (acg_lab_json_level_guard)"""
        n = C.c_uint(0)
        self._chk(self.L.acg_lab_json_level_guard(self.ctx, C.byref(n)))
        return n.value

    # ---- the text sink (acg_text_enable, acg_drain_text, acg_collect_text) -------------------------------------------------
    def enable_text(self, fmt, t0, date=False, freq=False, station_id="", freqs_hz=None):
        """The reference's text formats rendered on the device from now on.  fmt: "oneline" (-o 1, printoneline), "std" (-o 2,
        printmsg), "pp" (-N, Netoutpp) or "sv" (-n, Netoutsv), or K.TEXT_*; date: printdate() is printed (oneline, std); freq:
        printmsg's "F:" token (std); t0 as for enable_json; station_id: sv's "%8s"; freqs_hz: the channels' frequencies in Hz."""
        cfg = text_config(fmt, t0, date, freq, station_id)
        fr = None
        if freqs_hz is not None:
            fr = np.ascontiguousarray(freqs_hz, dtype=np.int32)
            assert fr.size == self.nch
        self._chk(self.L.acg_text_enable(self.ctx, C.byref(cfg), fr.ctypes.data if fr is not None else None))

    def disable_text(self):
        self._chk(self.L.acg_text_enable(self.ctx, None, None))

    def _text_call(self, fn, max_recs, *lead):
        n = max(1, int(max_recs))
        cap = n * K.TEXT_REC_MAX
        if getattr(self, "_tbuf_cap", 0) < cap:
            self._tbuf = C.create_string_buffer(cap)
            self._toffs = (C.c_uint * (n + 1))()
            self._tbuf_cap = cap
        out = []
        keys = []                                    # as _json_call
        while True:
            nb, nr = C.c_size_t(0), C.c_int(0)
            rc = self._chk(fn(self.ctx, *lead, self._tbuf, self._tbuf_cap, C.byref(nb), self._toffs, n, C.byref(nr)), allow=(K.EAGAIN,))
            blob, offs = C.string_at(self._tbuf, nb.value), self._toffs[:nr.value + 1]
            out += [blob[offs[i]:offs[i + 1]] for i in range(nr.value)]
            if rc == K.OK:
                self._keep_keys("text", keys)
                return out
            keys.append(self._c_sink_keys(K.SINK_TEXT))

    def drain_text(self, max_recs=4096):
        """The text records of every block completed since the last drain (needs repair=True and enable_text): a list of bytes, one
        per kept message, in (chn, end_bit) order per C call; loops while the C side says ACG_EAGAIN."""
        return self._text_call(self.L.acg_drain_text, max_recs)

    def collect_text(self, lag=1, max_recs=4096):
        """Streaming variant (acg_collect_text): the records of all calls but the `lag` newest"""
        return self._text_call(self.L.acg_collect_text, max_recs, lag)

    def text_level_guard(self):
        """records rendered since enable_text whose level lay within 8 ulp of a float rounding boundary (acg_lab_text_level_guard)"""
        n = C.c_uint(0)
        self._chk(self.L.acg_lab_text_level_guard(self.ctx, C.byref(n)))
        return n.value

    # ---- the outputs: every output of a message from one consumption (acg_outputs_enable, acg_drain_outputs) ----------------
    def enable_outputs(self, legs, t0, station_id="", app_name="acarsdec", app_ver="", freqs_hz=None):
        """Up to four legs rendered from the same kept records of one take, record i of every leg the same message: what the
        reference's outputmsg() prints (-o) and sends (-n, -N, -j) from one msg.  legs: see outputs_config ("msgs", "json",
        "oneline", "std", "pp", "sv", or (format, dict(date=.., freq=..))); t0, station_id, app_name, app_ver, freqs_hz as for
        enable_json / enable_text, one of each for all legs."""
        cfg = outputs_config(legs, t0, station_id, app_name, app_ver)
        fr = None
        if freqs_hz is not None:
            fr = np.ascontiguousarray(freqs_hz, dtype=np.int32)
            assert fr.size == self.nch
        self._chk(self.L.acg_outputs_enable(self.ctx, C.byref(cfg), fr.ctypes.data if fr is not None else None))
        self._out_kinds = [cfg.leg[l].kind for l in range(cfg.nlegs)]

    def disable_outputs(self):
        self._chk(self.L.acg_outputs_enable(self.ctx, None, None))
        self._out_kinds = []

    def _outputs_once(self, fn, max_recs, caps, *lead):
        """one C call: (rc, nrecs, one list per leg).  caps: records of room per leg (None: max_recs for every leg)"""
        kinds = getattr(self, "_out_kinds", [])
        n = max(1, int(max_recs))
        caps = [n] * len(kinds) if caps is None else [int(c) for c in caps]
        bufs = (K.OutBuf * max(1, len(kinds)))()
        keep = []
        for l, kind in enumerate(kinds):
            if kind == K.OUT_MSGS:
                out, extra = (K.Msg * max(1, caps[l]))(), (K.Oooi * max(1, caps[l]))()
                bufs[l].cap, bufs[l].oooi = caps[l] * C.sizeof(K.Msg), C.addressof(extra)
            else:
                rec_max = K.JSON_LINE_MAX if kind == K.OUT_JSON else K.TEXT_REC_MAX
                out, extra = C.create_string_buffer(max(1, caps[l] * rec_max)), (C.c_uint * (n + 1))()
                bufs[l].cap, bufs[l].offs = caps[l] * rec_max, C.addressof(extra)
            bufs[l].out = C.addressof(out)
            keep.append((out, extra))
        nr = C.c_int(0)
        rc = self._chk(fn(self.ctx, *lead, bufs, n, C.byref(nr)), allow=(K.EAGAIN,))
        legs = []
        for l, kind in enumerate(kinds):
            out, extra = keep[l]
            if kind == K.OUT_MSGS:
                assert bufs[l].nbytes == nr.value * C.sizeof(K.Msg)
                legs.append([(K.Msg.from_buffer_copy(out[i]), K.Oooi.from_buffer_copy(extra[i])) for i in range(nr.value)])
            else:
                blob, offs = C.string_at(out, bufs[l].nbytes), extra[:nr.value + 1]
                assert offs[0] == 0 and offs[nr.value] == bufs[l].nbytes
                legs.append([blob[offs[i]:offs[i + 1]] for i in range(nr.value)])
        return rc, nr.value, legs

    def _outputs_call(self, fn, max_recs, caps, *lead):
        out = [[] for _ in getattr(self, "_out_kinds", [])]
        keys = []                                    # as _json_call
        while True:
            rc, _, legs = self._outputs_once(fn, max_recs, caps, *lead)
            for acc, leg in zip(out, legs):
                acc += leg
            if rc == K.OK:
                self._keep_keys("outputs", keys)
                return out
            keys.append(self._c_sink_keys(K.SINK_OUTPUTS))

    def drain_outputs(self, max_recs=4096, caps=None):
        """Every leg of every block completed since the last drain (needs repair=True and enable_outputs), consumed once: one
        list per leg in the order of enable_outputs' legs -- bytes records (JSON, text) or (K.Msg, K.Oooi) pairs (msgs) -- all
        of one length, record i of each the same message, in (chn, end_bit) order per C call; loops while the C side says
        ACG_EAGAIN.  caps (a test aid: the binding bound of a take) gives each leg's buffer room for that many records instead of
        max_recs."""
        return self._outputs_call(self.L.acg_drain_outputs, max_recs, caps)

    def drain_outputs_once(self, max_recs=4096, caps=None):
        """A test aid, not part of the interface: (more, nrecs, legs) of ONE acg_drain_outputs call; more: the C side said
        ACG_EAGAIN"""
        rc, n, legs = self._outputs_once(self.L.acg_drain_outputs, max_recs, caps)
        self._keep_keys("outputs", [])               # sink_keys("outputs"): this call's
        return rc == K.EAGAIN, n, legs

    def collect_outputs(self, lag=1, max_recs=4096, caps=None):
        """Streaming variant (acg_collect_outputs): the legs of all calls but the `lag` newest"""
        return self._outputs_call(self.L.acg_collect_outputs, max_recs, caps, lag)

    def bits(self, ch):
        vo = np.zeros(self.bit_cap, dtype=np.float32)
        lvl = np.zeros(self.bit_cap, dtype=np.float32)
        n = C.c_int(0)
        self._chk(self.L.acg_read_bits(self.ctx, ch, vo.ctypes.data, lvl.ctypes.data, self.bit_cap, C.byref(n)))
        return vo[: n.value].copy(), lvl[: n.value].copy()

    def bits_all(self):
        counts = np.zeros(self.nch, dtype=np.int32)
        vo = np.zeros((self.nch, self.bit_cap), dtype=np.float32)
        lvl = np.zeros((self.nch, self.bit_cap), dtype=np.float32)
        self._chk(self.L.acg_read_bits_all(self.ctx, counts.ctypes.data, vo.ctypes.data, lvl.ctypes.data))
        return counts, vo, lvl

    def dm(self, ch, n):
        out = np.zeros(n, dtype=np.float32)
        self._chk(self.L.acg_read_dm(self.ctx, ch, out.ctypes.data, n))
        return out

    def state(self, ch):
        s = K.ChanState()
        self._chk(self.L.acg_get_state(self.ctx, ch, C.byref(s)))
        return dict(MskPhi=s.MskPhi, MskDf=s.MskDf, MskClk=s.MskClk, MskLvlSum=s.MskLvlSum,
                    MskBitCount=s.MskBitCount, MskS=s.MskS, idx=s.idx,
                    inb=np.array(s.inb[:], dtype=np.float32), outbits=s.outbits, nbits=s.nbits,
                    Acarsstate=s.Acarsstate, blk_len=s.blk_len, blk_err=s.blk_err)

    def set_timing(self, mode):
        """0 = off, 1 = both stages, 2 = down-converter launches only."""
        self._chk(self.L.acg_set_timing(self.ctx, int(mode)))

    def timing(self):
        f, m = C.c_double(0), C.c_double(0)
        nf, nm = C.c_int(0), C.c_int(0)
        self._chk(self.L.acg_get_timing(self.ctx, C.byref(f), C.byref(nf), C.byref(m), C.byref(nm)))
        return dict(fir_ms=f.value, fir_launches=nf.value, msk_ms=m.value, msk_launches=nm.value)


def make_msg_filter(downlink_only=False, skip_empty=False, labels=None, lib=None):
    """K.MsgFilter for acg_set_msg_filter / acg_selftest_msg_labels.  labels: None (no label filter), a -b string (split by
    acg_parse_label_filter exactly as label.c does) or a list of labels."""
    f = K.MsgFilter()
    f.flags = (K.MSGF_DOWNLINK_ONLY if downlink_only else 0) | (K.MSGF_SKIP_EMPTY if skip_empty else 0)
    if isinstance(labels, (str, bytes)):
        arg = labels.encode("latin1") if isinstance(labels, str) else labels
        _chk(None, (lib or K.load()).acg_parse_label_filter(arg, C.byref(f)))
    elif labels is not None:
        labels = [l.encode("latin1") if isinstance(l, str) else bytes(l) for l in labels]
        if len(labels) > K.MSGF_MAXLABELS or not all(labels):
            raise ValueError("at most %d non-empty labels" % K.MSGF_MAXLABELS)
        f.nlabels = len(labels)
        for i, l in enumerate(labels):
            f.labels[i].value = l[:3]
    return f


def json_config(t0, station_id="", app_name="acarsdec", app_ver=""):
    """K.JsonConfig for acg_json_enable / acg_selftest_msg_json; t0 = (sec, usec) or seconds as a float"""
    sec, usec = t0 if isinstance(t0, tuple) else (int(t0 // 1), int(round((t0 - t0 // 1) * 1e6)))
    if usec >= 1000000:
        sec, usec = sec + 1, usec - 1000000
    enc = lambda v: v.encode("latin1") if isinstance(v, str) else bytes(v)
    station_id, app_name, app_ver = enc(station_id), enc(app_name), enc(app_ver)
    if len(station_id) > 32 or len(app_name) > 16 or len(app_ver) > 16:
        raise ValueError("station_id holds 32 characters, app_name and app_ver 16")
    return K.JsonConfig(int(sec), int(usec), station_id, app_name, app_ver)


TEXT_FORMATS = {"oneline": K.TEXT_ONELINE, "std": K.TEXT_STD, "pp": K.TEXT_PP, "sv": K.TEXT_SV}


def text_config(fmt, t0, date=False, freq=False, station_id=""):
    """K.TextConfig for acg_text_enable / acg_selftest_msg_text; fmt: a name of TEXT_FORMATS or K.TEXT_*; t0 as json_config"""
    sec, usec = t0 if isinstance(t0, tuple) else (int(t0 // 1), int(round((t0 - t0 // 1) * 1e6)))
    if usec >= 1000000:
        sec, usec = sec + 1, usec - 1000000
    station_id = station_id.encode("latin1") if isinstance(station_id, str) else bytes(station_id)
    if len(station_id) > 32:
        raise ValueError("station_id holds 32 characters")
    flags = (K.TEXT_F_DATE if date else 0) | (K.TEXT_F_FREQ if freq else 0)
    return K.TextConfig(TEXT_FORMATS.get(fmt, fmt), flags, int(sec), int(usec), station_id)


SINK_KINDS = {"json": K.SINK_JSON, "text": K.SINK_TEXT, "outputs": K.SINK_OUTPUTS}      # Decoder.sink_keys
OUT_KINDS = dict(TEXT_FORMATS, msgs=K.OUT_MSGS, json=K.OUT_JSON)


def outputs_config(legs, t0, station_id="", app_name="acarsdec", app_ver=""):
    """K.OutputsConfig for acg_outputs_enable / acg_selftest_outputs.  legs: one entry per leg -- a name of OUT_KINDS ("msgs",
    "json", "oneline", "std", "pp", "sv"), a (name, dict(date=.., freq=..)) pair for a text format with flags, or a (kind, flags)
    pair of integers as the C side takes them; t0 and the strings as json_config"""
    j = json_config(t0, station_id, app_name, app_ver)
    legs = list(legs)
    if len(legs) > K.OUT_LEGS_MAX:
        raise ValueError("at most %d legs" % K.OUT_LEGS_MAX)
    cfg = K.OutputsConfig()
    cfg.nlegs = len(legs)
    for l, leg in enumerate(legs):
        kind, flags = leg if isinstance(leg, tuple) else (leg, 0)
        if isinstance(flags, dict):
            flags = (K.TEXT_F_DATE if flags.get("date") else 0) | (K.TEXT_F_FREQ if flags.get("freq") else 0)
        cfg.leg[l].kind, cfg.leg[l].flags = OUT_KINDS.get(kind, kind), int(flags)
    cfg.t0_sec, cfg.t0_usec, cfg.station_id, cfg.app_name, cfg.app_ver = j.t0_sec, j.t0_usec, j.station_id, j.app_name, j.app_ver
    return cfg


# oooi_t field -> the reference JSON's key (output.c:280-295, in the order buildjson adds them)
OOOI_JSON_KEYS = (("sa", "depa"), ("da", "dsta"), ("eta", "eta"), ("gout", "gtout"), ("gin", "gtin"), ("woff", "wloff"), ("won", "wlin"))


def oooi_json(msg, oooi):
    """The OOOI keys buildjson adds for (msg, oooi) (output.c:280-295): a key only when the label was decoded and the field's
    first byte is not NUL; its value is the field as a C string.  msg is the K.Msg the record belongs to (kept for symmetry
    with the other JSON keys a host builds from it)."""
    out = {}
    if oooi.decoded in (b"\x00", 0):
        return out
    for field, key in OOOI_JSON_KEYS:
        v = getattr(oooi, field)                      # (ctypes c_char arrays read up to the first NUL)
        if v:
            out[key] = v.decode("latin1")
    return out


def monitor_rows(flights, nbch):
    """printmonitor()'s rows (output.c:471-478) for a snapshot, without the clock column: the text before the time of the first
    message and the text after it, joined by one blank.  nbch: the channels the mask shows (the reference's nbch <= 16)."""
    rows = []
    for f in flights:
        s = " %-8s %-7s %3d " % (f.addr.decode("latin1"), f.fid.decode("latin1"), f.nbm)
        s += "".join("x" if (f.chm >> i) & 1 else "." for i in range(nbch)) + " " * max(0, 16 - nbch)
        s += " "
        for v in (f.sa, f.da, f.eta):
            s += (" %4s " % v.decode("latin1")) if v else "      "
        rows.append(s)
    return rows


def route_json(route, station=None):
    """routejson()'s object (output.c:442-447) for a K.Route, keys in the reference's order"""
    out = {"timestamp": route.sec + route.usec / 1e6}
    if station:
        out["station_id"] = station
    out["flight"] = route.fid.decode("latin1")
    out["depa"] = route.sa.decode("latin1")
    out["dsta"] = route.da.decode("latin1")
    return out


def stats_level_db(stats):
    """(lvl_min_db, lvl_max_db) as float32 arrays: the table's two level ratios through acars.c:351's arithmetic, 10 * log10 in
    double narrowed to float (what acg_frame.lvl and acg_msg.lvl hold); -inf for a ratio of 0 (no kept block yet)"""
    import math

    def db(v):
        return np.array([10 * math.log10(x) if x > 0 else -math.inf for x in v.tolist()], dtype=np.float64).astype(np.float32)
    return db(stats["lvl_min"]), db(stats["lvl_max"])


def scan_report(stats, freqs_hz):
    """scan.sh's last line for a whole table: rows (freq, delivered, kept, blocks), one per channel, busiest first (by
    delivered, then kept, then blocks; ties in channel order)"""
    assert len(freqs_hz) == len(stats)
    rows = [(freqs_hz[i], int(stats["delivered"][i]), int(stats["kept"][i]), int(stats["blocks"][i])) for i in range(len(stats))]
    order = sorted(range(len(rows)), key=lambda i: (-rows[i][1], -rows[i][2], -rows[i][3], i))
    return [rows[i] for i in order]


def frame_tuple(f):
    """(chn, len, err, crc, txt) -- the bit-exact part of a block."""
    return (int(f.chn), int(f.len), int(f.err), bytes(f.crc), bytes(f.txt[: max(0, f.len)]))


def best_placed(factory, n, iq_dev, nblocks, pitch, repeats=2, stream=None, fmt=0, plane=0, keep="best"):
    """Creates `n` decoders with factory() -- all alive during the trials, so that their buffers lie in different places --
    runs the same call on each once for nothing, then times it (Decoder.placement_trial) and keeps the fastest (keep="best")
    or the first (keep="first": the trial is then a diagnostic of how much the contexts of a process differ).  Returns
    (decoder, [ms per call], index); best_placed.last_fir_ms holds the down-converter tie-break figures where it was used."""
    decs = [factory() for _ in range(max(1, n))]
    if len(decs) == 1:
        return decs[0], [], 0
    def trial(d):
        return (d.placement_trial(iq_dev, nblocks, pitch, repeats, stream) if fmt == 0 else
                d.placement_trial_samples(fmt, iq_dev, nblocks, pitch, plane, repeats, stream))
    for d in decs:                      # a round for nothing: the first context timed is otherwise timed on a cold device (clocks,
        trial(d)                        # first touch of its buffers) and loses by 10-15 % to that alone (round 3, queue_probe.sh)
    ms = [trial(d) for d in decs]
    best = min(range(len(decs)), key=lambda i: ms[i])
    # Up to 2048 channels (CU partition) the demodulator sets the call, so the calls of all contexts are nearly alike while their
    # down-converters differ by a few per cent: among the contexts within 1 % of the fastest call keep the one whose
    # down-converter launches (event-timed) are the shortest.
    best_placed.last_fir_ms = None
    if fmt == 0 and all(getattr(d, "timing_flag", False) and d.nch <= 2048 for d in decs):
        fir = []
        for d in decs:
            d.set_timing(2)
            d.timing()
            for _ in range(3):
                d.in_callback(iq_dev, nblocks=nblocks, pitch=pitch, stream=stream)
            t = d.timing()
            fir.append(t["fir_ms"] / max(1, t["fir_launches"]))
            d.reset()
            d.set_timing(1)
        near = [i for i in range(len(decs)) if ms[i] <= 1.01 * min(ms)]
        best = min(near, key=lambda i: fir[i])
        best_placed.last_fir_ms = fir
    if keep == "first":
        best = 0
    for i, d in enumerate(decs):
        if i != best:
            d.close()
    return decs[best], ms, best
