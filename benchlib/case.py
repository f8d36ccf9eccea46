"""One case of bench.py: input synthesis, the parity gate on the first pass, the timed region, the result record."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")          # the entry point the child processes of a run re-enter

from .cases import CARRIER, COPY_CEILING_GBS, DEPTH, HBM_PEAK_GBS, SCALE, SNR_DB, make_taps
from .dump import last_step_outputs
from .probes import _probe_ab, _probe_decoders
from .telemetry import gpu_clock_mhz, gpu_telemetry
from .traffic import lookup_traffic


def run_case(J, name, case, args, steps, warmup, headline):
    """Builds the input of one workload in J.iq, checks the first pass against the oracle (--full), times `steps`
    steps.  Returns the dict that goes into the JSON line (rank 0) or None."""
    import ctypes as C
    import numpy as np
    import torch
    from acarsdec_amd import decoder as D, synth as S, _capi as K, shard
    L, dist, world, rank, dev, cdev = J.L, J.dist, J.world, J.rank, J.dev, J.cdev
    nch, M, ntaps, nblk, content = case["channels"], case["decim"], case["ntaps"], case["blocks"], case["content"]
    fmt_name = case.get("format") or (args.format if headline else "u8")
    fmt = {"u8": 0, "cs16": K.FMT_CS16, "split16": K.FMT_S16_SPLIT, "f32": K.FMT_F32_REAL}[fmt_name]
    bps = 2 if fmt == 0 else 4
    share = int(case.get("share") or (max(1, args.share) if headline else 1))
    if share > 1:
        assert fmt == 0 and nch % share == 0, "--share needs the u8 format and a channel count divisible by it"
        content = "shared+acars"
    if fmt != 0 and content != "format+acars":
        content = "format"
    nstreams = nch // share
    nout = nblk * 1024
    row = nout * M * bps
    assert nstreams * row <= J.iq_all.numel(), "input buffer too small for this case"
    iq = J.iq_all[: nstreams * row].view(nstreams, row)

    # ---- per-channel configuration: made on rank 0 for ALL channels of the job, scattered over RCCL
    # (the only data that ever crosses xGMI: 32 B per channel; inputs are generated where they are used)
    nch_total = nch * world
    cfg_rows = None
    if rank == 0:
        r0 = np.random.default_rng(0xACA25)
        off = r0.integers(-48, 49, size=nch_total) * 25000.0           # multiples of 12.5 kHz within +-1.2 MHz
        off[np.abs(off) < 25000] = 50000.0                              # >= 25 kHz from DC like chooseFc enforces
        if share > 1:
            # channels of one dongle: distinct carriers 150 kHz apart (75 kHz with more than 8), the whole comb shifted per dongle;
            # all multiples of 12.5 kHz (rtl.c:245-247), within +-0.6 MHz
            c_ = np.arange(nch_total)
            off = (2 * (c_ % share) - share + 1) * (75000.0 if share <= 8 else 37500.0) + ((c_ // share) % 5 - 2) * 12500.0
        cfg_rows = np.stack([off, r0.uniform(0, 2 * np.pi, nch_total), np.zeros(nch_total),
                             np.arange(nch_total, dtype=np.float64)], axis=1)
    mine = shard.scatter_channel_config(cfg_rows, world, rank, J.coll, device=cdev, force=J.coll is not None)
    own = shard.owned_channels(nch_total, rank, world)
    assert mine.shape[0] == nch and np.array_equal(mine[:, 3].astype(np.int64), own)
    offs, phases = mine[:, 0], mine[:, 1]
    taps = make_taps(D, fmt_name, offs, M, ntaps)

    # ---- input, resident in HBM: distinct content per channel, working set >> 256 MiB Infinity Cache
    sigma = SCALE * CARRIER * (M / (2.0 * 10 ** (SNR_DB / 10.0))) ** 0.5

    def synth_acars(n_first):
        """channels [0, n_first) of this rank: ACARS/MSK traffic, seeded 0xACA25 + global channel
        id: random printable frames of 20-220 characters every 0.25-1 s, AM depth 0.5, own carrier offset and phase, AWGN at
        20 dB SNR in the 12.5 kHz channel; modulated on the host (numpy), up-converted and quantised on the device."""
        trk = torch.empty((n_first, nout), dtype=torch.float32, device=dev)
        GEN = 512
        for c0 in range(0, n_first, GEN):
            n = min(GEN, n_first - c0)
            buf = np.empty((n, nout), dtype=np.float32)
            for i in range(n):
                a, _ = S.channel_audio(np.random.default_rng(0xACA25 + int(own[c0 + i])), nout, gap=(3125, 12500), text_len=(20, 220))
                buf[i] = CARRIER * (1.0 + DEPTH * a)
            trk[c0:c0 + n] = torch.from_numpy(buf).to(dev)
        d_idx = torch.arange(n_first, dtype=torch.int32, device=dev)
        d_off = torch.from_numpy(offs[:n_first].astype(np.float32)).to(dev)
        d_ph = torch.from_numpy(phases[:n_first].astype(np.float32)).to(dev)
        rc = L.acg_synth_iq_u8_dev(iq.data_ptr(), row, n_first, nout, M, trk.data_ptr(), nout, d_idx.data_ptr(),
                                   d_off.data_ptr(), d_ph.data_ptr(), SCALE, sigma, 0xACA25 + rank, None)
        assert rc == 0, rc
        torch.cuda.synchronize()

    if content == "acars":
        synth_acars(nch)
        data_desc = ("ACARS/MSK traffic on every channel, content seeded 0xACA25 + channel id (frames of 20-220 characters every "
                     "0.25-1 s), AM depth %.1f, carrier offset and phase per channel, AWGN at %.0f dB SNR in the 12.5 kHz channel "
                     "(sigma %.4f per I/Q sample); MSK modulator on the host, up-converter + u8 quantiser on the device" % (DEPTH, SNR_DB, sigma))
    elif content == "random+acars":
        assert L.acg_fill_random_u8_dev(iq.data_ptr(), row, nstreams, row, 0xACA25 + rank, None) == 0
        nacars = min(nch, max(64, args.check_channels))
        synth_acars(nacars)
        data_desc = ("uniform random bytes, seeded per stream (SURVEY 8d config 5: the value distribution is irrelevant to bandwidth); "
                     "the first %d channels (the ones the parity gate looks at) carry ACARS/MSK traffic as in the other cases, so "
                     "that the gate compares decoded blocks and not only magnitudes" % nacars)
    elif content == "shared+acars":
        # every dongle stream: uniform random bytes; the dongles of the gate's channels: the sum of their K channels' ACARS/MSK
        # carriers (SURVEY App. C.1 with K carriers), AWGN at 20 dB SNR per channel, generated on the device
        assert L.acg_fill_random_u8_dev(iq.data_ptr(), row, nstreams, row, 0xACA25 + rank, None) == 0
        ngate = (min(nch, max(64, args.check_channels)) + share - 1) // share
        sc_ = SCALE * 2.0 / share                                        # K carriers share the u8 range
        sg_ = sc_ * CARRIER * (M / (2.0 * 10 ** (SNR_DB / 10.0))) ** 0.5
        tt = torch.arange(nout * M, dtype=torch.float64, device=dev) * (2.0 * np.pi / (12500.0 * M))
        gen = torch.Generator(device=dev)
        gen.manual_seed(0xACA25 + rank)
        for s_ in range(ngate):
            xi = sg_ * torch.randn(nout * M, device=dev, generator=gen)
            xq = sg_ * torch.randn(nout * M, device=dev, generator=gen)
            for k_ in range(share):
                c = s_ * share + k_
                a, _ = S.channel_audio(np.random.default_rng(0xACA25 + int(own[c])), nout, gap=(3125, 12500), text_len=(20, 220))
                env = torch.from_numpy((sc_ * CARRIER * (1.0 + DEPTH * a)).astype(np.float32)).to(dev).repeat_interleave(M)
                ph = torch.remainder(tt * float(offs[c]) + float(phases[c]), 2.0 * np.pi).to(torch.float32)
                xi += env * torch.cos(ph)
                xq += env * torch.sin(ph)
            iq[s_, 0::2] = torch.round(127.37 + 127.5 * xi).clamp_(0, 255).to(torch.uint8)
            iq[s_, 1::2] = torch.round(127.37 + 127.5 * xq).clamp_(0, 255).to(torch.uint8)
        del tt, env, ph, xi, xq
        data_desc = ("uniform random bytes, seeded per dongle stream; the first %d dongles (the ones the parity gate looks at) carry the sum of "
                     "their %d channels' ACARS/MSK carriers (150 kHz apart, AM depth %.1f, %.0f dB SNR per channel), generated on the device"
                     % (ngate, share, DEPTH, SNR_DB))
    elif content == "format+acars":
        assert fmt in (K.FMT_CS16, K.FMT_F32_REAL, K.FMT_S16_SPLIT)
        if fmt in (K.FMT_CS16, K.FMT_S16_SPLIT):
            assert L.acg_fill_random_u8_dev(iq.data_ptr(), row, nstreams, row, 0xACA25 + rank, None) == 0
            iq.view(torch.int16).bitwise_and_(0x0FFF)
        else:
            iq.view(torch.float32).normal_(0.0, 0.1)
        nacars = min(nch, max(64, args.check_channels))
        # the gate's channels: ACARS/MSK traffic as in the u8 cases, up-converted with torch on the device, a few channels at a time:
        # CS16 = complex baseband quantised to int16 (rint(32767 * 0.9 x), synth.iq_s16_from_envelopes); real f32 = 2 x env x cos
        # at the channel's offset from 0 Hz of the real spectrum (synth.real_f32_from_envelopes)
        tt = torch.arange(nout * M, dtype=torch.float64, device=dev) * (2.0 * np.pi / (12500.0 * M))
        gen = torch.Generator(device=dev)
        gen.manual_seed(0xACA25 + rank)
        v16 = iq.view(torch.int16).view(nstreams, -1)
        v32 = iq.view(torch.float32).view(nstreams, -1)
        for c in range(nacars):
            a, _ = S.channel_audio(np.random.default_rng(0xACA25 + int(own[c])), nout, gap=(3125, 12500), text_len=(20, 220))
            env = torch.from_numpy((SCALE * CARRIER * (1.0 + DEPTH * a)).astype(np.float32)).to(dev).repeat_interleave(M)
            # (real f32: air.c mixes with Fc - Fr + rate / 4, air.c:278, i.e. the channel sits at its offset + a quarter of the rate)
            f_c = float(offs[c]) + (12500.0 * M / 4.0 if fmt == K.FMT_F32_REAL else 0.0)
            ph = torch.remainder(tt * f_c + float(phases[c]), 2.0 * np.pi).to(torch.float32)
            if fmt == K.FMT_CS16:
                xi = env * torch.cos(ph) + sigma * torch.randn(nout * M, device=dev, generator=gen)
                xq = env * torch.sin(ph) + sigma * torch.randn(nout * M, device=dev, generator=gen)
                v16[c, 0::2] = torch.round(32767.0 * 0.9 * xi).clamp_(-32768, 32767).to(torch.int16)
                v16[c, 1::2] = torch.round(32767.0 * 0.9 * xq).clamp_(-32768, 32767).to(torch.int16)
            elif fmt == K.FMT_S16_SPLIT:        # the 12-bit ADC range of the RSP in an I plane followed by a Q plane (sdrplay.c:215-220)
                xi = env * torch.cos(ph) + sigma * torch.randn(nout * M, device=dev, generator=gen)
                xq = env * torch.sin(ph) + sigma * torch.randn(nout * M, device=dev, generator=gen)
                v16[c, : nout * M] = torch.round(2047.0 * 0.9 * xi).clamp_(-2048, 2047).to(torch.int16)
                v16[c, nout * M:] = torch.round(2047.0 * 0.9 * xq).clamp_(-2048, 2047).to(torch.int16)
            else:
                v32[c] = 2.0 * env * torch.cos(ph) + sigma * torch.randn(nout * M, device=dev, generator=gen)
        del tt, env, ph
        data_desc = ("%s; the first %d channels (the ones the parity gate looks at) carry ACARS/MSK traffic "
                     "as in the u8 cases (AM depth %.1f, %.0f dB SNR in the channel), generated on the device"
                     % ("gaussian float32 samples" if fmt == K.FMT_F32_REAL else "uniform random 12-bit int16 samples", nacars, DEPTH, SNR_DB))
    elif content == "random":
        assert L.acg_fill_random_u8_dev(iq.data_ptr(), row, nstreams, row, 0xACA25 + rank, None) == 0
        data_desc = "uniform random bytes, seeded per stream (SURVEY 8d config 5: the value distribution is irrelevant to bandwidth)"
    else:
        if fmt == K.FMT_F32_REAL:
            iq.view(torch.float32).normal_(0.0, 0.1)
            data_desc = "gaussian float32 samples (format throughput run; blocks of this format are covered by tests/)"
        else:
            assert L.acg_fill_random_u8_dev(iq.data_ptr(), row, nstreams, row, 0xACA25 + rank, None) == 0
            iq.view(torch.int16).bitwise_and_(0x0FFF)
            data_desc = "uniform random 12-bit int16 samples (format throughput run; blocks of this format are covered by tests/)"
    torch.cuda.synchronize()

    # The batch is streamed through the library in calls of `cb` callbacks (the reference hands over ONE callback at a
    # time, rtl.c:314; 8 keeps the 12.5 kHz intermediate of a call inside the Infinity Cache at 1024 channels).
    cb = min(args.call_blocks, nblk)
    while nblk % cb:
        cb -= 1
    ncall = nblk // cb
    if fmt == K.FMT_S16_SPLIT:
        cb, ncall = nblk, 1                                # (plane layout: one call)
    repair = not args.raw_blocks
    def make_decoder():
        # max_lag = --collect-lag: this host collects that many calls behind, and the block queue holds that many + 1 calls' worth
        d_ = D.Decoder(nch, decim=M, ntaps=ntaps, nstreams=nstreams, max_blocks=cb, device=J.local, bitlog=bool(args.bitlog), timing=True,
                       repair=repair, max_lag=max(1, args.collect_lag))
        d_.set_taps(taps)
        if share > 1:
            d_.set_channel_streams(np.arange(nch) // share)
        return d_
    stream = torch.cuda.current_stream().cuda_stream
    # The context a host gets from acg_create is the one that is timed (--placements 1, the default).  --placements N is a
    # DIAGNOSTIC: N contexts alive at once, acg_placement_trial on each, their times reported under config.placement; the
    # FIRST is still the one timed unless --placement-keep best (rounds 2-3 kept the fastest of four: selection).
    ntrial = args.placements if share == 1 else 1
    dec, trial_ms, trial_best = D.best_placed(make_decoder, ntrial, iq, cb, row, repeats=8 if nch > 2048 else 24, stream=stream, fmt=fmt,
                                              plane=row // 2 if fmt == K.FMT_S16_SPLIT else 0, keep=args.placement_keep)
    dec0 = dec
    maxfr = max(8192, int(nch * (cb / 3.0 + 2)))
    cb_bytes = cb * 1024 * M * bps
    passes = [0]                                    # passes of dec0 since its last reset (the gate resets it once)

    def step(lag=None, sink=None, dec=None, dm_sink=None, frames=False, raw=None):
        """one pass of the hot path over the batch; the results (acg_msg records; blocks with frames=True or --raw-blocks) are
        delivered to the host --collect-lag calls behind (default 2: the host then never waits for the block repair of the call
        before the newest one before it may hand over the next -- with a lag of 1 that wait sat between every two calls)"""
        lag = args.collect_lag if lag is None else lag
        n = 0
        if dec is None:
            passes[0] += 1
        dec = dec or dec0
        for k in range(ncall):
            part = iq[:, k * cb_bytes:(k + 1) * cb_bytes]
            if fmt == 0:
                dec.in_callback(part, nblocks=cb, pitch=row, stream=stream)
            else:
                dec.process_samples(fmt, part, cb, pitch=row, plane=row // 2 if fmt == K.FMT_S16_SPLIT else 0, stream=stream)
            if repair and not frames:
                # the delivered path: repaired blocks through outputmsg()'s field split, as acg_msg records
                m = 0
                while True:
                    mm, fb, more = dec.collect_msgs_raw(lag, maxfr)
                    if sink is not None:
                        sink += [K.Msg.from_buffer_copy(fb[i]) for i in range(mm)]
                    keep_raw(raw, fb, mm)
                    m += mm
                    if not more:
                        break
            else:
                m, fb = dec.collect_frames_raw(lag, maxfr)
                if sink is not None:
                    sink += [K.Frame.from_buffer_copy(fb[i]) for i in range(m)]
                keep_raw(raw, fb, m)
            if dm_sink is not None:                     # (gate only) the 12.5 kHz samples this call's demodulator consumed
                for c in dm_sink:
                    dm_sink[c].append(dec.dm(c, cb * 1024))
            n += m
        return n

    def keep_raw(raw, fb, m):
        """(--dump-outputs) the first m records of the library's reused result array, as bytes: one copy, parsed after the timed region"""
        if raw is not None and m:
            raw.append(C.string_at(C.addressof(fb), m * C.sizeof(fb._type_)))

    def drain(dec=None, raw=None):
        """everything still queued, through the delivered path; returns the count"""
        dec = dec or dec0
        if not repair:
            m, fb = dec.drain_frames_raw(maxfr)
            keep_raw(raw, fb, m)
            return m
        m = 0
        while True:
            mm, fb, more = dec.drain_msgs_raw(maxfr)
            keep_raw(raw, fb, mm)
            m += mm
            if not more:
                return m

    def barrier():
        torch.cuda.synchronize()
        if J.coll is not None:
            dist.barrier(device_ids=[J.local]) if J.backend == "nccl" else dist.barrier()
        torch.cuda.synchronize()

    # ---- correctness gate on the first pass (state starts from reset): benchlib/gate.py.  A comparison with the CPU checkers, so
    # --full only: a plain run goes from set-up straight to warm-up (tests/ hold the parity of every kernel)
    parity = None
    gate_passes = 0
    if args.full:
        from types import SimpleNamespace
        from . import gate
        # channels the gate looks at: --check-channels (64), more where a case says so (wide: 8 callbacks = 0.66 s of signal per
        # channel is half a block per channel -- VERDICT r05 weak 1: "also.wide gates on 32 blocks")
        check = case.get("check_channels", args.check_channels) if args.check_channels == 64 else args.check_channels
        parity = gate.first_pass(SimpleNamespace(check=check, args=args, J=J, name=name, rank=rank, nch=nch, share=share, fmt=fmt, M=M, taps=taps, ntaps=ntaps, iq=iq, row=row,
                                                 nout=nout, cb=cb, ncall=ncall, cb_bytes=cb_bytes, stream=stream, maxfr=maxfr, repair=repair, dec=dec, step=step))
        gate_passes = 2 if repair else 1                # (in the demodulator's warm-up event sums below)
        passes[0] = 1                                   # the gate's last pass runs from a reset (repair) or from creation

    # ---- timing.  A "pass" = the hot path once over the resident batch (the step of rounds 1-2).  `burst`: `steps` single
    # passes, timed as before (about half a second at the headline case: too short to be seen by an outside observer, and
    # inside the window in which the shader clock has not settled).  The reported `value` is SUSTAINED: a step is `reps`
    # passes, reps chosen from the burst rate so that `steps` steps take >= --sustain seconds; per-step times (host clock at
    # the step boundaries, no extra synchronisation: the host runs at most one call ahead of the device) give min / median /
    # max, the shader clock is read from sysfs while the device is still busy.
    # the HBM-saturating cases are reported at >= --sustain-hbm seconds (their rate sinks with the shader clock at the power cap);
    # the cases whose step the demodulator sets have a flat clock (step spread 0.35 %) and keep --sustain
    from .cases import SUSTAIN_HBM
    sustain_s = args.sustain_hbm if (name in SUSTAIN_HBM and args.sustain > 0 and not args.channels) else args.sustain

    from .timing import timed_region
    # --dump-outputs: what the host receives in the last pass of the last step (and the drain behind it), kept as raw records
    dump = bool(headline and rank == 0 and getattr(args, "dump_outputs", None))
    last_raw, last_start = [], []

    def last_pass():
        last_start.append(passes[0] * nout)             # 12.5 kHz samples per channel since the reset before this pass
        return step(raw=last_raw)
    # a plain run times one pass per step and has no burst; --full (or --sustain) adds the burst and sizes the step by it
    T = timed_region(step, drain, barrier, dec, steps, warmup, sustain_s, J, sync=torch.cuda.synchronize,
                     burst=bool(args.full or sustain_s > 0), last_pass=last_pass if dump else None,
                     last_drain=(lambda: drain(raw=last_raw)) if dump else None)
    warm, tim_b, dt_burst, reps, clk0, clk_mid, clk1, tele_mid = (T[k] for k in ('warm', 'tim_b', 'dt_burst', 'reps', 'clk0', 'clk_mid', 'clk1', 'tele_mid'))
    dt_local, tim, step_ms, dt, nfr_total, per_rank = (T[k] for k in ('dt_local', 'tim', 'step_ms', 'dt', 'nfr_total', 'per_rank'))
    if dump:                                            # (before the probes below touch the decoder)
        J.dump = last_step_outputs(dec, last_raw, last_start[0], nch, cb * 1024, repair, bool(args.bitlog), K)
    # measurement aids (--ab, --decoders: same-process A/B of a per-launch switch, further decoders in the same process); not part
    # of the reported value, dead in the default run, and kept out of this function (the timed path must be auditable)
    ab = _probe_ab(args, J, step, drain, steps, nch, nout, M) if (args.ab and world == 1) else None
    trials = (_probe_decoders(args, J, make_decoder, step, drain, steps, reps, dt_local, nch, nout, M, dev)
              if (args.decoders > 1 and world == 1) else None)
    dec.close()
    if rank != 0:
        return None

    samples_per_pass = nch * nout * M                               # complex input samples per GPU per pass over the batch
    samples_per_step = samples_per_pass * reps
    value = world * samples_per_step * steps / dt / 1e6             # channel * Msamples/s
    # algorithmic bytes: 2 B per input sample per channel read (bps for the other formats), 4 B per
    # 12.5 kHz output written, taps (8 B each) read once per launch.  A step is `lps` pipelined FIR launches.
    lps = max(1, round(tim["fir_launches"] / (steps * reps)))       # launches per PASS
    pass_bytes = nstreams * nout * bps * M + nch * nout * 4 + lps * nch * ntaps * 8      # shared-stream mode: a stream's bytes count once
    step_bytes = pass_bytes * reps
    fir_bytes = pass_bytes / lps
    fir_avg_ms = tim["fir_ms"] / max(1, tim["fir_launches"])
    achieved = fir_bytes / (fir_avg_ms * 1e-3) / 1e9
    fir_ms_step = tim["fir_ms"] / steps
    burst = None
    if dt_burst is not None:
        burst = {"value": round(world * samples_per_pass * steps / dt_burst / 1e6, 1), "ms_per_pass": round(dt_burst / steps * 1e3, 4),
                 "timed_region_s": round(dt_burst, 4), "whole_job_frac_of_hbm": round(pass_bytes * steps / dt_burst / 1e9 / HBM_PEAK_GBS, 4),
                 "roofline_frac": round(fir_bytes / (tim_b["fir_ms"] / max(1, tim_b["fir_launches"]) * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                 "note": "`steps` single passes over the batch from a cold-ish device, as rounds 1-2 timed them; not the reported value"}
    msk_ms_step = warm["msk_ms"] / max(1, warmup + gate_passes) * reps          # (the gate's one or two passes are in the sum)
    mm = share > 1 and M in (160, 192, 200) and (cb * 1024) % 64 == 0             # (mirrors acg_fir_mm_takes)
    if fmt == 0:
        # (fir_mm.hip: two tiles in flight on one wave per SIMD where the demodulator shares the CUs -- no CU partition above 2048 channels)
        kname = ("fir_u8_mm_kernel<%d, %d>" % (M // 8, 2 if nch > 2048 else 1) if mm else "fir_u8_shared_kernel") if share > 1 else J.fir_kernel_name(M, nout)
    else:
        # (mirrors acg_launch_fir_fmt: the wave-private kernel <FMT, 16-byte chunks per window (per plane), windows per tile> where it is
        #  instantiated for the window length, else round 1's workgroup-granular kernel)
        fid = {"cs16": 1, "split16": 2, "f32": 3}[fmt_name]
        shape = {("cs16", 160): (40, 32), ("cs16", 192): (48, 32), ("cs16", 200): (50, 32), ("f32", 200): (50, 32), ("f32", 240): (60, 16),
                 ("f32", 480): (120, 8), ("f32", 800): (200, 8), ("split16", 160): (20, 64)}.get((fmt_name, M))
        kname = ("fir_fmt_direct_kernel<%d, %d, %d>" % ((fid,) + shape)) if shape else "fir_fmt_kernel<%d>" % fid
    # HBM traffic of this launch shape from the committed PMC passes (rocprofv3 cannot run inside the timed
    # process): looked up by the full kernel signature and launch shape, not measured in this run -- the source is named next to the number
    traffic, traffic_src = lookup_traffic(kname, nch, M, ntaps, nblk / lps)
    whole = step_bytes * steps / dt / 1e9                            # per GPU
    # the rate over the first ~5 s of the timed region (what rounds 1-5 reported as `value` for every case)
    marks = T["marks"]
    k5 = next((i for i in range(1, len(marks)) if marks[i] - marks[0] >= 5.0), len(marks) - 1)
    burst5s = world * samples_per_step * k5 / (marks[k5] - marks[0]) / 1e6 if (sustain_s > 5.0 and k5 < len(marks) - 1) else None
    tele3 = [T["tele0"], tele_mid, T["tele1"]]
    # the demodulator's own bound (it sets the step of the <= 2048-channel cases): a serial recurrence per channel whose wave
    # issues ~275 instructions per bit period (msk_lean.hip, 8 lanes per channel -- 4: ~40 more --: 261 in a period inside a segment + the segment's
    # set-up and framing spread over its 8 bits; counted in the product's ISA, tests/test_host_logic.py) or ~325 (msk.hip, the other
    # launch shapes) from one wave per SIMD at >= 4 cycles each (profiles/r05_probe_msk_phase_stamps.txt)
    msk_launches = max(1, warm["msk_launches"]) if warm.get("msk_launches") else None     # (none without warm-up and gate)
    roofline_msk = None
    if msk_launches and clk_mid:
        us_bit = warm["msk_ms"] / msk_launches * 1e3 / ((nblk * (warmup + gate_passes) * 1024 / msk_launches) * 2400.0 / 12500.0)
        # (mirrors acg_create: lanes per channel by channel count; <= 2048 channels: the demodulator's own CU partition of 2.5 x its
        #  one-wave-per-SIMD minimum, at most 80 CUs)
        dec_lpc = 8 if nch <= 8192 else 4 if nch <= 16384 else 2 if nch <= 32768 else 1
        msk_waves = nch * dec_lpc / 64.0
        msk_cus = min(80, (5 * max(1, int((msk_waves + 3) // 4)) + 1) // 2) if nch <= 2048 else 256
        waves_per_simd = max(1.0, msk_waves / (4.0 * msk_cus))
        cyc = us_bit * clk_mid / waves_per_simd
        # (mirrors acg_launch_msk: in_callback-shaped launches with 8 lanes per channel take msk_lean.hip)
        nolean = os.environ.get("ACG_ALLOW_TUNING") == "1" and os.environ.get("ACG_MSK_NOLEAN", "0") not in ("", "0")   # (the A/B switch, if this run carries it)
        lean = dec_lpc in (4, 8) and (cb * 1024) % 32 == 0 and not nolean
        # (4 lanes per channel: two mixer evaluations per lane and period, ~40 instructions more in either kernel)
        ipb = (275 if lean else 325) + (40 if dec_lpc == 4 else 0)
        roofline_msk = {"bound": "issue", "kernel": "msk_lean_kernel" if lean else "msk_demod_kernel", "us_per_bit": round(us_bit, 4),
                        "waves_per_simd": round(waves_per_simd, 2),
                        "cycles_per_bit_per_wave": round(cyc, 0), "instr_per_bit": ipb, "floor_cycles_per_bit": 4 * ipb,
                        "frac": round(4.0 * ipb / cyc, 3) if cyc > 0 else None,
                        "note": "launch time / bit periods per channel, at the shader clock read mid-run; floor = %d instructions x 4 issue cycles "
                                "(one wave per SIMD cannot issue faster); the arithmetic is the reference's operation for operation" % ipb}
    out = {
        "value": round(value, 1),
        "ms_per_step": round(dt / steps * 1e3, 4),
        "timed_region_s": round(dt, 4),
        "sustain": {"passes_per_step": reps, "step_ms_min_median_max": [round(step_ms[0], 3), round(step_ms[len(step_ms) // 2], 3), round(step_ms[-1], 3)],
                    "shader_clock_mhz_start_mid_end": [clk0, clk_mid, clk1], "telemetry_mid_run": tele_mid, "telemetry_start_mid_end": tele3,
                    "sustain_s_asked": sustain_s, "burst5s": (round(burst5s, 1) if burst5s else None),
                    "note": "a step = passes_per_step passes over the resident batch (chosen from the burst rate so that the timed region lasts "
                            ">= --sustain seconds); step times from host time stamps at the step boundaries (the host runs at most one call ahead "
                            "of the device); clocks from sysfs while the device is busy (null where the box does not expose them)"},
        "data": "synthetic: " + data_desc,
        "config": {"workload": "%s: %d channels/GPU x %.1f Msps %s, one stream per channel, rtlMult=%d, ntaps=%d; step = %d pass(es) over a resident batch of "
                               "%d callbacks/channel in calls of %d; FIR decimate + MSK demod + framing%s, delivered to the host %d call(s) behind"
                               % (case["tag"], nch, 12500 * M / 1e6, {"u8": "u8 IQ", "cs16": "CS16 IQ", "split16": "split int16 I/Q", "f32": "real f32"}[fmt_name],
                                  M, ntaps, reps, nblk, cb, " + block repair + message split" if repair else "", args.collect_lag),
                   "signal_seconds_per_pass": round(nblk * 0.08192, 3),
                   "callbacks_per_call": cb, "collect_lag": args.collect_lag, "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"),
                   "case": name, "input_format": fmt_name, "channels_per_gpu": nch, "decim": M, "ntaps": ntaps, "blocks_per_step": nblk * reps, "blocks_per_pass": nblk, "passes_per_step": reps,
                   "input_bytes_per_gpu": int(nstreams * row),
                   "realtime_channels_equiv": int(value / (12500 * M / 1e6)),
                   "arithmetic": "%s in, f32 down-converter and matched filter, f64 VCO/PLL/normalisation (as the reference)"
                                 % {"u8": "u8 I/Q", "cs16": "int16 I/Q", "split16": "split int16 I/Q", "f32": "real f32"}[fmt_name],
                   "delivered": ("acg_msg records: blocks checked / repaired on the device (ACG_F_REPAIR, acars.c:93-215) and split into outputmsg()'s fields "
                                 "(output.c:486-560) by acg_collect_msgs, inside the timed region" if repair else
                                 "pre-repair blocks (acg_collect_frames, --raw-blocks)"),
                   "channels_total": nch_total, "blocks_decoded_timed": int(nfr_total),
                   "contexts": "one context from acg_create, as a host gets it (no placement selection)" if not trial_ms or trial_best == 0 else "best of %d contexts (--placement-keep best)" % len(trial_ms),
                   "placement": ({"contexts_tried": len(trial_ms), "ms_per_call": [round(x, 3) for x in trial_ms], "kept": trial_best,
                                  "spread": round(max(trial_ms) / min(trial_ms) - 1.0, 4),
                                  "fir_ms_per_launch": ([round(x, 4) for x in D.best_placed.last_fir_ms] if getattr(D.best_placed, "last_fir_ms", None) else None),
                                  "note": "diagnostic (--placements N), untimed: N contexts alive at once, acg_placement_trial on each after a warm-up round; "
                                          "`kept` is the one timed (0 = the first, unless --placement-keep best)"}
                                 if trial_ms else None)},
        "roofline": {"bound": "hbm", "kernel": kname, "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
                     "traffic_source": (traffic_src + " (rocprofv3 PMC passes of the same launch shape: 2 x FETCH_SIZE + WRITE_SIZE; "
                                        "looked up by the full kernel signature, not collected in this run)") if traffic else None,
                     "bytes_per_launch": int(fir_bytes), "avg_launch_ms": round(fir_avg_ms, 4), "launches_per_step": lps * reps,
                     "launches_per_pass": lps,
                     "timing": "HIP events around every launch of the kernel on its own stream, inside the timed region "
                               "(the demodulator of the previous call / chunk runs beside it)",
                     "frac_of_measured_copy_ceiling_6290": round(achieved / COPY_CEILING_GBS, 4)},
        "whole_job_frac_of_hbm": round(whole / HBM_PEAK_GBS, 4),
        "whole_job_GBs_per_gpu": round(whole, 1),
        "time_dominant_kernel": (roofline_msk or {}).get("kernel", "msk_demod_kernel") if msk_ms_step > fir_ms_step else kname,
        "kernels": {"fir_ms_per_step": round(fir_ms_step, 4), "msk_ms_per_step": round(msk_ms_step, 4),
                    "note": "per-step sums of event-timed launches; the stages overlap (down-converter of call/chunk i+1 beside the "
                            "demodulator of i); the demodulator figure is taken during warm-up (its events are off in the timed region)"},
        "parity": parity,
    }
    if burst is not None:
        out["burst"] = burst
    if roofline_msk:
        out["roofline_msk"] = roofline_msk
    import re
    m_ = re.search(r"profiles/(r\d+)_", traffic_src or "")
    out["roofline"]["traffic_src"] = ((m_.group(1) if m_ else "committed") if traffic else None)      # "live" where bench.py measured it in this run
    if ab:
        out["ab_same_process"] = ab
    if trials:
        out["placement_trials"] = trials
    if ntaps != M:
        out["config"]["filter"] = ("%d-tap low-pass = the channel's NCO taps (rtl.c:283-286) x Hamming window, unit DC gain; the reference "
                                   "only has the boxcar, so the oracle for this filter is the same sum(vb*wf) formula with these taps" % ntaps)
    if world > 1:
        out["per_gpu"] = [round(samples_per_step * steps / t / 1e6, 1) for t in per_rank]
    if J.coll is not None and world == 1:
        out["config"]["collectives"] = "forced through torch.distributed/%s with world size 1 (--rccl-selftest)" % J.backend
    if share > 1:
        out["config"]["channels_per_stream"] = share
        fir_s = tim["fir_ms"] * 1e-3 / max(1, tim["fir_launches"])             # seconds per launch
        flops = 8.0 * nch * (nout / lps) * M / fir_s                            # rtl.c:349-351: 8 flop per channel-sample
        if mm:
            ks = (M // 8 + 1) // 2
            groups = nstreams * ((share + 7) // 8)
            mops = groups * (nout / lps / 32.0) * ks * 2 * 65536.0 / fir_s     # two v_mfma_i32_32x32x32_i8 per 32 windows x 32 bytes x group
            out["roofline"]["note"] = ("rtl.c's shape: %d channels reuse each dongle stream's bytes (a [windows x 2M] x [2M x 2K] contraction); on the "
                                       "matrix pipe (exact int8 digits, fir_mm.hip) it is HBM-bound again: achieved counts each stream ONCE.  Not the "
                                       "figure of the one-stream-per-channel path" % share)
            out["roofline"]["valu_equivalent"] = {"flop_per_s": round(flops, 0), "peak": 157.3e12, "frac": round(flops / 157.3e12, 4),
                                                  "means": "8 flop x channel-samples/s of this kernel against the packed-f32 vector peak "
                                                           "(MI355X_MICROARCH.md: 157.3 TFLOP/s): what a VALU kernel would have to sustain"}
            out["roofline"]["mfma_i8"] = {"ops_per_s": round(mops, 0), "peak": 5.03e15, "frac": round(mops / 5.03e15, 4)}
        else:
            out["roofline"]["note"] = ("shared-stream mode: %d channels reuse each stream's bytes, the vector-pipe down-converter is VALU-bound "
                                       "(8*K flop per 2 B); achieved counts each stream once and is NOT the HBM roofline figure" % share)
            keff = min(share, 8)
            ops = nch * nout * M * (2.0 + 3.0 / keff) * steps / (tim["fir_ms"] * 1e-3)
            out["valu"] = {"kernel": "fir_u8_shared_kernel", "lane_ops_per_s": round(ops, 0), "peak": 256 * 4 * 16 * 2.4e9,
                           "frac": round(ops / (256 * 4 * 16 * 2.4e9), 4), "lane_ops_per_channel_sample": round(2.0 + 3.0 / keff, 3)}
    return out
