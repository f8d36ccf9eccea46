"""The host side of the flight table across contexts, without a GPU: the layout of acg_flight_event as the C compiler, ctypes and
numpy see it; shard.gather_flight_events over gloo; the argument checks of acg_flights_import under the address and
undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from acarsdec_amd import _capi as K
from acarsdec_amd import shard
import host_side
from test_shard_gloo import free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["end_sample", "soh_sample", "sec", "usec", "chn", "addr", "fid", "e_ok", "oooi"]

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "acarsdec_amd.h"
#define F(name) printf(#name " %zu %zu\n", offsetof(acg_flight_event, name), sizeof(((acg_flight_event *)0)->name))
int main(void)
{
	printf("sizeof %zu\n", sizeof(acg_flight_event));
	F(end_sample); F(soh_sample); F(sec); F(usec); F(chn); F(addr); F(fid); F(e_ok); F(oooi);
	return 0;
}
"""


def test_record_layout_is_the_same_in_c_ctypes_and_numpy(tmp_path):
    """sizeof and every offsetof of acg_flight_event, printed by a C program compiled against the public header, equal those of
    K.FlightEvent and of K.FLIGHT_EVENT_DTYPE; 88 bytes, no hole: the fields cover every byte"""
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(LAYOUT_C)
    r = subprocess.run(["gcc", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split("\n")
    assert lines[0] == "sizeof 88"
    c_layout = {ln.split()[0]: (int(ln.split()[1]), int(ln.split()[2])) for ln in lines[1:] if ln}
    assert list(c_layout) == FIELDS
    ct = {n: (getattr(K.FlightEvent, n).offset, getattr(K.FlightEvent, n).size) for n, _ in K.FlightEvent._fields_}
    dt = np.dtype(K.FLIGHT_EVENT_DTYPE)
    npl = {n: (dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names}
    assert ct == c_layout and npl == c_layout
    import ctypes as C
    assert C.sizeof(K.FlightEvent) == dt.itemsize == 88
    covered = sorted(c_layout.values())
    assert covered[0][0] == 0 and all(a + s == b for (a, s), (b, _) in zip(covered, covered[1:])) and sum(covered[-1]) == 88


def events(rank, n):
    """n records whose every byte depends on (rank, index)"""
    rng = np.random.default_rng(100 + rank)
    return np.frombuffer(rng.integers(0, 256, n * 88, dtype=np.uint8).tobytes(), dtype=K.FLIGHT_EVENT_DTYPE)


COUNTS = (0, 5, 700)


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    got = shard.gather_flight_events(events(rank, COUNTS[rank]), dst=0, dist=dist)
    none = shard.gather_flight_events(events(rank, 0), dst=0, dist=dist)             # (nobody has anything: still one exchange)
    if rank == 0:
        q.put((got.tobytes(), str(got.dtype), len(none)))
    else:
        assert got is None and none is None
    dist.barrier()
    dist.destroy_process_group()


def test_gather_flight_events_world3_gloo():
    """ranks with 0, 5 and 700 events: rank 0 receives exactly the concatenation in rank order, the others None"""
    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    blob, dtype, none = q.get(timeout=240)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert blob == b"".join(events(r, COUNTS[r]).tobytes() for r in range(world)) and len(blob) == 705 * 88
    assert dtype == str(np.dtype(K.FLIGHT_EVENT_DTYPE)) and none == 0


def test_channel_map_is_the_inverse_of_the_partition():
    for nch, world in ((64, 4), (3, 3), (3, 2), (10, 4)):
        for r in range(world):
            own = shard.owned_channels(nch, r, world)
            m = shard.flight_channel_map(len(own), r, world)
            assert m.dtype == np.int32 and m.tolist() == own.tolist()
    assert shard.gather_flight_events(events(1, 4)).tobytes() == events(1, 4).tobytes()       # no process group: what went in


def test_event_kernels_have_no_private_segment():
    """flight.hip's export and import kernels, compiled with the product's flags (as tests/test_flight_model.py compiles the
    pass's other kernels): both are there, and neither has a private segment -- nothing of an event goes through scratch"""
    import re
    from acarsdec_amd import _build as B
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "acarsdec_amd", "csrc")
    flags = {name: fl for name, fl, _ in B.UNITS}["flight.hip"]
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include")] +
                       flags + ["-S", "-o", "-", os.path.join(csrc, "flight.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    priv = re.findall(r"\.amdhsa_kernel _Z\d+(fl_events_\w+?_kernel)\w*\n(?:.*\n)*?\s*\.amdhsa_private_segment_fixed_size (\d+)", r.stdout)
    assert sorted(priv) == [("fl_events_export_kernel", "0"), ("fl_events_import_kernel", "0")], priv


def test_import_argument_checks_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """acg_flight_events_check -- what acg_flights_import runs on its events before it looks at the context -- and the NULL-context
    answers of the new entry points, in the host units (host_side.py) built with -fsanitize=address,undefined and
    driven by tests/sanitize/flight_import_driver.c: every rule alone, the limits themselves, a bad record first, in the middle and
    last of 700 on the heap.  Any sanitizer report fails the test."""
    if not (shutil.which("g++") and os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h")):
        pytest.skip("needs g++ and the HIP headers")
    csrc = os.path.join(ROOT, "acarsdec_amd", "csrc")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-O1", "-g", "-w"]
    objs = host_side.compile_host_objects(tmp_path, "flight_import_driver.c", san + inc)
    exe = str(tmp_path / "flight_import_driver")
    libs = ["-L/opt/rocm/lib", "-lamdhip64", "-ldl", "-lm", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(["g++"] + san + objs + ["-o", exe] + libs, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "sanitized flight import driver: ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
