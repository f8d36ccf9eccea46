"""The host side of the 12.5 kHz PCM front end, no GPU: the libsndfile stand-in of the file demo under the sanitizers, the
soundfile.c hunk against the reference text, and the resources of pcm.hip's kernels as the product builds them."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

CSRC = os.path.join(ROOT, "acarsdec_amd", "csrc")
DEMO = os.path.join(CSRC, "demo")


def wav_bytes(pcm, extensible=False, data=None, data_size=None):
    nch = pcm.shape[1]
    data = np.ascontiguousarray(pcm, dtype="<i2").tobytes() if data is None else data
    core = struct.pack("<HHIIHH", 0xFFFE if extensible else 1, nch, 12500, 12500 * 2 * nch, 2 * nch, 16)
    if extensible:                                      # cbSize 22: valid bits, channel mask, the PCM sub-format GUID
        core += struct.pack("<HHI", 22, 16, 0) + bytes([1, 0, 0, 0, 0, 0, 0x10, 0, 0x80, 0, 0, 0xAA, 0, 0x38, 0x9B, 0x71])
    body = b"WAVE" + b"LIST" + struct.pack("<I", 3) + b"abc\0" + b"fmt " + struct.pack("<I", len(core)) + core
    body += b"data" + struct.pack("<I", len(data) if data_size is None else data_size) + data
    return b"RIFF" + struct.pack("<I", len(body)) + body


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("gcc"):
        pytest.skip("needs gcc")
    exe = str(tmp_path_factory.mktemp("pcm") / "sndfile_driver")
    r = subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + DEMO, os.path.join(DEMO, "demo_sndfile_wav.c"), os.path.join(ROOT, "tests", "pcm", "sndfile_driver.c"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_driver(args):
    """the driver with the leak check on; where LeakSanitizer cannot run at all (no ptrace in the sandbox) it says so itself and
    the run is repeated without it"""
    for leaks in ("1", "0"):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=%s:abort_on_error=0" % leaks, UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run(args, capture_output=True, text=True, timeout=120, env=env)
        if "LeakSanitizer has encountered a fatal error" not in r.stderr and "LeakSanitizer does not work" not in r.stderr:
            break
    return r


def read_with(driver, tmp_path, blob, req=4096):
    src, out = tmp_path / "in.wav", tmp_path / "out.f32"
    src.write_bytes(blob)
    r = run_driver([driver, str(src), str(req), str(out)])
    assert "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-1000:])
    lines = r.stdout.split()
    return [int(v) for v in lines[:3]], [int(v) for v in lines[3:]], np.fromfile(str(out), dtype=np.float32)


@pytest.mark.parametrize("shape", ["plain", "extensible", "cut_mid_frame", "size_mid_frame"])
def test_sndfile_stand_in_reads_pcm16_wav_like_sf_read_float(driver, tmp_path, shape):
    """demo_sndfile_wav.c + a main of its own under -fsanitize=address,undefined: test.wav's 4-channel PCM16 written as a plain
    header, as WAVE_FORMAT_EXTENSIBLE, with the file cut short inside a frame, and with a data size that ends inside a frame.
    4096-frame requests return exactly pcm / 32768, full counts, the short count at the end, then 0; no sanitizer report."""
    pcm = np.load(os.path.join(GOLDEN, "testwav_pcm16.npz"))["pcm"].astype(np.int16)
    nfr, nch = pcm.shape
    if shape == "cut_mid_frame":
        blob = wav_bytes(pcm)[:-(3 * 2 * nch + 3)]                # the header still promises every frame
        nfr -= 4
    elif shape == "size_mid_frame":
        blob = wav_bytes(pcm, data_size=2 * nch * (nfr - 2) + 5)
        nfr -= 2
    else:
        blob = wav_bytes(pcm, extensible=shape == "extensible")
    info, counts, x = read_with(driver, tmp_path, blob)
    assert info[:2] == [nch, 12500] and info[2] == (pcm.shape[0] if shape == "cut_mid_frame" else nfr)
    full, rest = divmod(nfr, 4096)
    assert counts == [4096 * nch] * full + [rest * nch, 0, 0]
    want = pcm[:nfr].astype(np.float32) / np.float32(32768.0)
    assert x.size == nfr * nch and np.array_equal(x.view(np.uint32), want.reshape(-1).view(np.uint32))


def test_sndfile_stand_in_refuses_what_it_does_not_read(driver, tmp_path):
    pcm = np.zeros((8, 2), dtype=np.int16)
    good = wav_bytes(pcm)
    for blob in (b"", good[:20], good.replace(b"WAVE", b"WAVX"), good.replace(struct.pack("<HH", 2 * 2, 16), struct.pack("<HH", 3 * 2, 24)),
                 good[:good.index(b"data")]):
        src = tmp_path / "bad.wav"
        src.write_bytes(blob)
        r = run_driver([driver, str(src), "16", str(tmp_path / "o")])
        assert r.returncode == 1 and r.stdout == "open failed\n" and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.stdout, r.stderr[-800:])


def test_soundfile_hunk_applies_and_compiles_against_the_stand_in(tmp_path):
    """patched_source("soundfile.c"): its anchors hold on the reference text, the only demodMSK() call is gone, one call of
    acarsdec_amd_pcm_frames stands in its place, and the text compiles (from stdin, as the build passes it) with the stand-in's
    header"""
    from acarsdec_amd import _build as B
    if not os.path.exists(os.path.join(B.REF, "soundfile.c")) or not shutil.which("gcc"):
        pytest.skip("needs the reference tree and gcc")
    src = B.patched_source("soundfile.c")
    ref = open(os.path.join(B.REF, "soundfile.c")).read()
    assert "demodMSK(" not in src and src.count("acarsdec_amd_pcm_frames(sndbuff, nbi / nbch);") == 1 and src.count(B.COMPAT_INCLUDE) == 1
    assert len(ref.splitlines()) - len(src.splitlines()) == 7 - 1 - 1           # seven lines out, the call and the include in
    r = subprocess.run(["gcc", "-O2", "-w", "-DWITH_SNDFILE", "-I" + B.REF, "-I" + B.INC, "-I" + DEMO, "-x", "c", "-c", "-", "-o", str(tmp_path / "s.o")],
                       input=src, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    syms = subprocess.run(["nm", str(tmp_path / "s.o")], capture_output=True, text=True).stdout
    assert " U acarsdec_amd_pcm_frames" in syms and "demodMSK" not in syms


def test_abi_declares_the_pcm_entry_points():
    from acarsdec_amd import _build as B, _capi as K
    names = B.declared_symbols()
    for n in ("acg_process_pcm_dev", "acg_feed_pcm_host", "acg_lab_pcm_deinterleave"):
        assert n in names and (n in K.SYMBOLS or n in K.LAB_SYMBOLS)
    hdr = open(os.path.join(B.INC, "acarsdec_amd.h")).read()
    assert re.search(r"#define ACG_PCM_S16\s+1\b", hdr) and re.search(r"#define ACG_PCM_F32\s+2\b", hdr) and (K.PCM_S16, K.PCM_F32) == (1, 2)
    # the legacy view: declared in a header of its own that the compat header (what a bound front end includes) pulls in
    assert "void acarsdec_amd_pcm_frames(const float *interleaved, int nframes);" in open(os.path.join(B.INC, "acarsdec_amd_compat_pcm.h")).read()
    assert '#include "acarsdec_amd_compat_pcm.h"' in open(os.path.join(B.INC, "acarsdec_amd_compat.h")).read()
    assert re.search(r"^void acarsdec_amd_pcm_frames\(", open(os.path.join(CSRC, "compat_msk.c")).read(), flags=re.M)


# pcm.hip's header comment states these: at most 32 VGPRs, no scratch, no static LDS (the tile is dynamic: <= 16640 bytes)
VGPR_BUDGET = 32


def test_pcm_kernels_use_no_scratch_and_keep_their_budget():
    """pcm.hip compiled for gfx950 with the product's flags: four kernels (two formats x two tiles), a private segment of 0 bytes,
    no scratch instruction, the register budget of its comment; the float32 kernels hold no float arithmetic at all"""
    from acarsdec_amd import _build as B
    hipcc = B.hipcc()
    flags = {name: (f, prod) for name, f, prod in B.UNITS}
    assert flags["pcm.hip"][1] is True
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17", "-I" + CSRC, "-I" + B.INC] + flags["pcm.hip"][0] +
                       ["-S", "-o", "-", os.path.join(CSRC, "pcm.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", r.stdout, flags=re.M)
    scratch = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", r.stdout)]
    vgpr = [int(v) for v in re.findall(r"\.vgpr_count:\s*(\d+)", r.stdout)]
    lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", r.stdout)]
    print("pcm.hip kernels:", list(zip(names, vgpr, lds, scratch)))
    assert sorted(names) == sorted("_Z16pcm_deint_kernelILi%dELb%dEEv8PcmKArgs" % (f, w) for f in (1, 2) for w in (0, 1))
    assert len(scratch) == len(vgpr) == len(lds) == 4 and not any(scratch) and not any(lds) and "scratch_" not in r.stdout
    assert max(vgpr) <= VGPR_BUDGET, vgpr
    # the bodies of the F32 kernels: words move, no float instruction touches them
    for w in (0, 1):
        name = "_Z16pcm_deint_kernelILi2ELb%dEEv8PcmKArgs" % w
        body = r.stdout.split("\n" + name + ":")[1].split(".Lfunc_end")[0]
        assert not re.search(r"\bv_(mul|add|fma|cvt|mac|max|min)\w*_f(16|32|64)", body), name
