"""The 12.5 kHz front ends' own input shape: interleaved PCM frames, all channels in one call (pcm.hip, acg_process_pcm_dev,
acg_feed_pcm_host, acarsdec_amd_pcm_frames).  The de-interleave is exact (int16 * 2^-15, or a bit copy), so every comparison
here is bit for bit: the kernel alone against the numpy transpose, the file's bytes in against the planar entry point and the
committed goldens, the JSON sink behind it against the reference's stdout, the call contract, and the reference program with
soundfile.c's one hunk against the golden text.  GPU box only."""
import hashlib
import json
import os
import re
import subprocess
import wave

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden_blocks, fhex, soft_from_v
import json_model as JM

pytestmark = pytest.mark.gpu

FILL = 0x4B1DF00D                                     # the image's fill: a finite float no input produces
SPECIALS = np.array([0x80000000, 0x00000001, 0x7F800000, 0xFF800000, 0x7FC12345, 0xFF800001], dtype=np.uint32)  # -0.0, a denormal, +-inf, two NaN payloads


@pytest.fixture(scope="module")
def D():
    from acarsdec_amd import decoder
    from acarsdec_amd import _capi as K
    assert K.load().acg_device_count() > 0, "GPU tests need a GPU; the library has no CPU fallback"
    return decoder


@pytest.fixture(scope="module")
def K():
    from acarsdec_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def pcm():
    """test.wav's samples as the file holds them: int16 [53843, 4]"""
    x = np.ascontiguousarray(np.load(os.path.join(GOLDEN, "testwav_pcm16.npz"))["pcm"], dtype=np.int16)
    assert x.shape == (53843, 4)
    return x


def scaled(x):
    return x.astype(np.float32) / np.float32(32768.0)


def frame_fields(f):
    return (int(f.chn), int(f.len), int(f.err), float(f.lvl), bytes(f.crc), bytes(f.txt[:max(0, f.len)]), int(f.end_bit), int(f.end_sample),
            int(f.soh_sample))


def state_key(s):
    return {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in s.items()}


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2, 3, 4, 5, 16, 63, 64, 65, 130])
def test_kernel_alone_equals_the_transpose_and_writes_nothing_else(D, K, nch):
    """acg_lab_pcm_deinterleave: the input in a device buffer of exactly its size, the dm image pre-filled.  Both formats, every
    frame count around the tile edges: columns [0, nframes) equal the numpy transpose bit for bit (int16: -32768 and 32767 at
    both ends of the buffer and across a frame boundary; float32: random words with -0.0, a denormal, the infinities and two NaN
    payloads, compared as words), every other word of the image -- the columns behind nframes, the pitch padding -- still holds
    the fill.  Odd channel counts put frames on 2-byte boundaries and samples of two frames into one word."""
    dec = D.Decoder(nch, decim=8, ntaps=8, max_blocks=2, bitlog=False)
    rng = np.random.default_rng(1000 + nch)
    fill = float(np.array([FILL], dtype=np.uint32).view(np.float32)[0])
    try:
        for nframes in (1, 2, 63, 64, 65, 127, 1024, 1025):
            n = nframes * nch
            pitch = (nframes + 15) // 16 * 16 + 16
            for fmt in (K.PCM_S16, K.PCM_F32):
                if fmt == K.PCM_S16:
                    x = rng.integers(-32768, 32768, size=n).astype(np.int16)
                    x[0], x[-1] = -32768, 32767
                    if n > nch:
                        x[nch - 1], x[nch] = 32767, -32768
                    want = scaled(x).view(np.uint32)
                else:
                    x = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
                    at = rng.choice(n, size=min(n, len(SPECIALS)), replace=False)
                    x[at] = SPECIALS[:len(at)]
                    want = x
                img = np.zeros((nch, pitch), dtype=np.uint32)
                rc = dec.L.acg_lab_pcm_deinterleave(dec.ctx, fmt, x.ctypes.data, nframes, img.ctypes.data, pitch, fill)
                assert rc == K.OK, (fmt, nframes, dec.L.acg_last_error(dec.ctx))
                assert np.array_equal(img[:, :nframes], want.reshape(nframes, nch).T), (fmt, nframes)
                assert np.all(img[:, nframes:] == FILL), (fmt, nframes)
    finally:
        dec.close()


# ---- 2. test.wav, the file's bytes in --------------------------------------------------------------------------------------
def bit_log(dec):
    """the bit records of the last demodulator launch, per channel: (vo, lvl)"""
    counts, vo, lvl = dec.bits_all()
    return [(vo[c, :counts[c]].copy(), lvl[c, :counts[c]].copy()) for c in range(dec.nch)]


def planar_twin(D, x, chunk, max_blocks=4):
    """demod_msk on the de-interleaved floats in chunks of `chunk` frames: blocks, every call's bit log, the state"""
    dec = D.Decoder(x.shape[1], decim=8, ntaps=8, max_blocks=max_blocks)
    frames, bits = [], []
    for s in range(0, x.shape[0], chunk):
        dec.demod_msk(np.ascontiguousarray(x[s:s + chunk].T))
        frames += [frame_fields(f) for f in dec.drain_frames()]
        bits.append(bit_log(dec))
    out = frames, bits, [state_key(dec.state(c)) for c in range(x.shape[1])]
    dec.close()
    return out


def same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for ca, cb in zip(a, b) for x, y in zip(ca, cb))


@pytest.fixture(scope="module")
def twins(D, pcm):
    """computed once: the planar results in soundfile.c's chunks and in chunks of 1000"""
    return {c: planar_twin(D, scaled(pcm), c) for c in (4096, 1000)}


@pytest.mark.parametrize("as_float", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("chunk", [53843, 4096, 1000])
def test_testwav_frames_in_equal_the_planar_path_and_the_golden(D, pcm, golden, golden_bits, twins, chunk, as_float):
    """testwav_pcm16.npz exactly as the file holds it (int16 frames; and the same as float32 frames) through feed_pcm: as ONE call
    (53843 frames > max_len = 4096: the internal chunking runs, in chunks of 4096), in soundfile.c's reads of 4096 frames, in
    reads of 1000.  Blocks (per channel in order), the bit log after EVERY call and the channel state are bit-identical to
    demod_msk on pcm / 32768 in the same chunks (the one call leaves the log of its last chunk: the twin's last).  Against the
    committed golden: the blocks and the integer state exactly; the whole file's bits (chunked runs) and the continuous state
    within tests/test_gpu_parity.py's bounds for the planar path -- the reference's libm against the device's sin/cos, nothing
    of this path: hard decisions equal on strong bits, |d vo| <= 5e-2 and <= 1e-4 for 99 %, levels 1e-4 relative; MskDf, MskPhi
    1e-9, MskClk 1e-6."""
    frames_in = scaled(pcm) if as_float else pcm
    dec = D.Decoder(4, decim=8, ntaps=8, max_blocks=4)
    got, bits = [], []
    for s in range(0, pcm.shape[0], chunk):
        dec.feed_pcm(np.ascontiguousarray(frames_in[s:s + chunk]))
        got += [frame_fields(f) for f in dec.drain_frames()]
        bits.append(bit_log(dec))
    st = [dec.state(c) for c in range(4)]
    dec.close()
    want_frames, want_bits, want_st = twins[min(chunk, 4096)]
    if chunk > 4096:                                   # one call: its blocks come in one drain, per channel in order
        assert sorted(got) == sorted(want_frames)
        for c in range(4):
            assert [g for g in got if g[0] == c] == [w for w in want_frames if w[0] == c], c
        assert same_bits(bits[-1], want_bits[-1])
    else:
        assert got == want_frames
        assert len(bits) == len(want_bits) and all(same_bits(a, b) for a, b in zip(bits, want_bits))
    assert [state_key(s) for s in st] == want_st
    gb = {}
    for t, _ in golden_blocks(golden["file"]["raw_blocks"]):
        gb.setdefault(t[0], []).append(t)
    mine = {}
    for g in got:
        mine.setdefault(g[0], []).append((g[0], g[1], g[2], g[4], g[5]))
    assert mine == gb
    for c in range(4):
        g = golden["file"]["final_state"][c]
        for k in ("MskS", "idx", "nbits", "Acarsstate", "outbits", "MskBitCount"):
            assert st[c][k] == g[k], (c, k)
        dphi = abs(st[c]["MskPhi"] - fhex(g["MskPhi"]))
        assert abs(st[c]["MskDf"] - fhex(g["MskDf"])) <= 1e-9 and abs(st[c]["MskClk"] - fhex(g["MskClk"])) <= 1e-6
        assert min(dphi, abs(dphi - 2 * np.pi)) <= 1e-9
        if chunk <= 4096:
            m = golden_bits["chn"] == c
            vo_o, lvl_o = soft_from_v(golden_bits["vr"][m], golden_bits["vi"][m], golden_bits["MskS"][m])
            vo = np.concatenate([b[c][0] for b in bits])
            lvl = np.concatenate([b[c][1] for b in bits])
            assert len(vo) == golden["file"]["bits_per_channel"][c] == len(vo_o)
            d = np.abs(vo - vo_o)
            strong = np.abs(vo_o) > 0.05
            assert np.array_equal(vo[strong] > 0, vo_o[strong] > 0) and d.max() <= 5e-2 and (d <= 1e-4).mean() >= 0.99
            assert np.allclose(lvl, lvl_o, rtol=1e-4, atol=1e-6)


# ---- 3. wide, the device entry ---------------------------------------------------------------------------------------------
def test_wide_device_entry_equals_the_planar_twin_record_for_record(D, K, pcm):
    """1030 channels (16 full channel tiles and one of 6): test.wav's four channels repeated, channel c rolled by 37 c frames.
    Eight process_pcm calls of 4096 frames from a torch tensor against acg_process_dm_dev on the transposed floats: the blocks
    drained after every call are the same records in the same order, and the dm rows of channels 0, 63, 64 and 1029 hold the
    input's columns."""
    import torch
    nch, per, calls = 1030, 4096, 8
    x = np.empty((per * calls, nch), dtype=np.int16)
    for c in range(nch):
        x[:, c] = np.roll(pcm[:, c % 4], 37 * c)[:per * calls]
    a = D.Decoder(nch, decim=8, ntaps=8, max_blocks=4, bitlog=False)
    b = D.Decoder(nch, decim=8, ntaps=8, max_blocks=4, bitlog=False)
    total = 0
    try:
        for k in range(calls):
            part = x[k * per:(k + 1) * per]
            frames_dev = torch.from_numpy(np.ascontiguousarray(part)).cuda()
            planar_dev = torch.from_numpy(np.ascontiguousarray(scaled(part).T)).cuda()
            a.process_pcm(frames_dev, K.PCM_S16, per)
            b._chk(b.L.acg_process_dm_dev(b.ctx, planar_dev.data_ptr(), per, per, None))
            na, fa = a.drain_frames_raw()
            mine = [frame_fields(fa[i]) for i in range(na)]
            nb, fb = b.drain_frames_raw()
            assert mine == [frame_fields(fb[i]) for i in range(nb)], k
            total += na
            for ch in (0, 63, 64, 1029):
                assert np.array_equal(a.dm(ch, per).view(np.uint32), scaled(part[:, ch]).view(np.uint32)), (k, ch)
        # (the file holds >= 7 blocks per 4 channels; the rolls spread them evenly over its 53843 frames, of which 32768 are played:
        #  ~1000 blocks, less those a roll's wrap or the cut splits)
        assert total >= 300, total
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("nch", [4, 130], ids=["flat", "wide"])
def test_device_entry_on_a_side_stream_lets_the_buffer_be_refilled_in_place(D, K, pcm, nch):
    """acg_process_pcm_dev with a caller's stream that is not the context's: the frames are produced on that stream right before
    the call (a device copy into ONE buffer), and the next copy into the same buffer is enqueued right behind the call, without
    a synchronise -- the kernel, the buffer's only reader, runs on the caller's stream, the demodulator behind an event on its
    own.  24 calls of 2048 frames (0.91 of the file): blocks and final state equal demod_msk's on the same frames."""
    import torch
    per, calls = 2048, 24
    x = np.stack([np.roll(pcm[:, c % 4], 37 * c)[:per * calls] for c in range(nch)], axis=1)
    src = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    buf = torch.empty((per, nch), dtype=torch.int16, device="cuda")
    ts = torch.cuda.Stream()
    ts.wait_stream(torch.cuda.current_stream())
    dec = D.Decoder(nch, decim=8, ntaps=8, max_blocks=2, bitlog=False, max_lag=0)
    ref = D.Decoder(nch, decim=8, ntaps=8, max_blocks=2, bitlog=False)
    try:
        got, want = [], []
        for k0 in range(0, calls, 4):                   # four calls in flight between collections
            with torch.cuda.stream(ts):
                for k in range(k0, k0 + 4):
                    buf.copy_(src[k * per:(k + 1) * per], non_blocking=True)
                    dec.process_pcm(buf, K.PCM_S16, per, stream=ts.cuda_stream)
            got += [frame_fields(f) for f in dec.drain_frames()]
        for k in range(calls):
            ref.demod_msk(np.ascontiguousarray(scaled(x[k * per:(k + 1) * per]).T))
            want += [frame_fields(f) for f in ref.drain_frames()]
        assert sorted(got) == sorted(want) and len(got) >= max(1, nch // 4)
        assert [state_key(dec.state(c)) for c in (0, nch - 1)] == [state_key(ref.state(c)) for c in (0, nch - 1)]
    finally:
        dec.close()
        ref.close()


# ---- 4. the sink end to end ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["none", "Aeb"])
def test_json_sink_behind_the_file_bytes_prints_the_reference_lines(D, variant):
    """msgjson_pcm16.npz (3 channels) as the int16 frames of its file through feed_pcm, JSON sink on as tests/test_gpu_json_sink.py
    configures it: drain_json()'s lines are the reference's stdout (msgjson_golden.json), unfiltered and with -A -e -b, per channel
    byte for byte but for the number of the time stamp (the reference stamps its wall clock).  No sample is converted and no line
    is rendered or ordered on the host."""
    T0, CHUNK = (1792301725, 269667), 4096
    planar = np.load(os.path.join(GOLDEN, "msgjson_pcm16.npz"))["pcm"]
    with open(os.path.join(GOLDEN, "msgjson_golden.json")) as f:
        g = json.load(f)
    assert planar.dtype == np.int16 and planar.shape[0] == g["nch"] == 3
    frames = np.ascontiguousarray(planar.T)                      # the file's layout: [nframes][3]
    app = json.loads(g["variants"]["none"]["lines"][0])["app"]
    args = g["variants"][variant]["args"]
    dec = D.Decoder(3, decim=8, ntaps=8, max_blocks=CHUNK // 1024, repair=True, bitlog=False)
    dec.enable_json(T0, g["station"], app["name"], app["ver"])
    dec.set_msg_filter(downlink_only="-A" in args, skip_empty="-e" in args, labels=g["label_list"] if "-b" in args else None)
    blob = b""
    for s in range(0, frames.shape[0], CHUNK):
        dec.feed_pcm(frames[s:s + CHUNK])
        blob += dec.drain_json()
    dec.close()
    assert blob.endswith(b"\n")
    lines = [ln + b"\n" for ln in blob.split(b"\n")[:-1]]
    ref = [ln.encode("ascii") + b"\n" for ln in g["variants"][variant]["lines"]]
    assert len(lines) == len(ref) > 0
    chn_of = lambda ln: int(re.search(rb',"channel":(-?\d+),"freq":', ln).group(1))
    for c in range(3):
        assert [JM.cut_timestamp(ln)[0] for ln in lines if chn_of(ln) == c] == [JM.cut_timestamp(ln)[0] for ln in ref if chn_of(ln) == c], c


# ---- 5. the contract -------------------------------------------------------------------------------------------------------
def test_contract_errors_empty_calls_and_mixing_with_the_planar_entry(D, K, pcm):
    import torch
    dec = D.Decoder(4, decim=8, ntaps=8, nstreams=1, max_blocks=2)
    L, ctx = dec.L, dec.ctx
    host = np.zeros((2049, 4), dtype=np.int16)
    dev = torch.zeros(2049 * 4 + 2, dtype=torch.int16, device="cuda")
    try:
        for fmt in (0, 3):
            assert L.acg_feed_pcm_host(ctx, fmt, host.ctypes.data, 16) == K.EINVAL
            assert L.acg_process_pcm_dev(ctx, fmt, dev.data_ptr(), 16, None) == K.EINVAL
        assert L.acg_process_pcm_dev(ctx, K.PCM_S16, dev.data_ptr(), 2 * 1024 + 1, None) == K.EINVAL
        assert L.acg_process_pcm_dev(ctx, K.PCM_S16, dev.data_ptr(), -1, None) == K.EINVAL
        assert L.acg_process_pcm_dev(ctx, K.PCM_S16, None, 16, None) == K.EINVAL
        assert L.acg_feed_pcm_host(ctx, K.PCM_S16, None, 16) == K.EINVAL
        for fmt in (K.PCM_S16, K.PCM_F32):                          # a base off by 2 bytes
            assert L.acg_feed_pcm_host(ctx, fmt, host.ctypes.data + 2, 16) == K.EINVAL
            assert L.acg_process_pcm_dev(ctx, fmt, dev.data_ptr() + 2, 16, None) == K.EINVAL
        # a run of frames, then empty calls: OK, and nothing of the state moves
        dec.feed_pcm(np.ascontiguousarray(pcm[:1500]))
        dec.drain_frames()
        before = [state_key(dec.state(c)) for c in range(4)]
        assert L.acg_feed_pcm_host(ctx, K.PCM_S16, host.ctypes.data, 0) == K.OK
        assert L.acg_process_pcm_dev(ctx, K.PCM_F32, dev.data_ptr(), 0, None) == K.OK
        assert [state_key(dec.state(c)) for c in range(4)] == before and dec.drain_frames() == []
        # acg_feed_samples_host leaves 3 of a window's 8 samples in the staging buffers: the PCM feed says so, the u8 path's words
        dec.reset()
        dec.feed(K.FMT_CS16, np.zeros((1, 6), dtype=np.int16))
        assert L.acg_feed_pcm_host(ctx, K.PCM_S16, host.ctypes.data, 16) == K.ESTATE
        msg = L.acg_last_error(ctx)
        assert L.acg_process_iq_u8_host(ctx, host.ctypes.data, 2 * 1024 * 8, 1) == K.ESTATE and L.acg_last_error(ctx) == msg
        dec.reset()
        assert L.acg_feed_pcm_host(ctx, K.PCM_S16, host.ctypes.data, 16) == K.OK
        # frames and planar rows alternate on one context: the all-planar result
        dec.reset()
        dec.drain_frames()
        got = []
        for k, s in enumerate(range(0, pcm.shape[0], 2048)):
            part = pcm[s:s + 2048]
            if k % 2:
                dec.demod_msk(np.ascontiguousarray(scaled(part).T))
            else:
                dec.feed_pcm(np.ascontiguousarray(part) if k % 4 else np.ascontiguousarray(scaled(part)))
            got += [frame_fields(f) for f in dec.drain_frames()]
        st = [state_key(dec.state(c)) for c in range(4)]
    finally:
        dec.close()
    want, _, want_st = planar_twin(D, scaled(pcm), 2048, max_blocks=2)
    assert got == want and len(got) >= 7 and st == want_st


# ---- 6. the legacy view ----------------------------------------------------------------------------------------------------
def test_reference_program_with_the_soundfile_hunk_prints_the_golden_text_in_one_call_per_read(pcm, golden, tmp_path):
    """soundfile.c itself with its one hunk (acarsdec_amd_pcm_frames instead of the per-channel loop) on the libsndfile stand-in:
    `-o 1 -f` and `-o 2 -f` print what lib/acarsdec_gpu prints and what the golden holds, and the entry point is called once per
    4096-frame read -- 14 = ceil(53843 / 4096) -- where the per-channel view makes 4 x 14 = 56."""
    exe = os.path.join(ROOT, "acarsdec_amd", "lib", "acarsdec_gpu_file")
    old = os.path.join(ROOT, "acarsdec_amd", "lib", "acarsdec_gpu")
    if not (os.path.exists(exe) and os.path.exists(old)):
        pytest.skip("demo binaries not built (they need the reference tree at build time)")
    src = str(tmp_path / "t.wav")
    with wave.open(src, "wb") as wv:
        wv.setnchannels(pcm.shape[1])
        wv.setsampwidth(2)
        wv.setframerate(12500)
        wv.writeframes(np.ascontiguousarray(pcm, dtype="<i2").tobytes())
    env = dict(os.environ, ACARSDEC_AMD_STATS="1")
    calls = {}
    for o in ("1", "2"):
        out = {}
        for name, prog in (("file", exe), ("gpu", old)):
            r = subprocess.run([prog, "-o", o, "-f", src], env=env, capture_output=True, timeout=300)
            out[name] = r.stdout
            m = re.search(r"acarsdec_amd compat: (\d+) calls", r.stderr.decode("latin-1"))
            assert m, r.stderr.decode("latin-1")[-600:]
            calls[name] = int(m.group(1))
        assert out["file"] == out["gpu"], o
        assert hashlib.md5(out["file"]).hexdigest() == golden["program"]["o" + o]["md5"], o
        if o == "1":
            assert out["file"].decode("latin-1") == golden["program"]["o1"]["stdout"]
        assert calls == {"file": 14, "gpu": 56}, calls
