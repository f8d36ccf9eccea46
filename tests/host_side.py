"""The host side of the library as the sanitizer tests build it: the units acarsdec_amd/_build.py names in HOST_UNITS and
HOST_C_UNITS, compiled with the caller's flags next to a driver with its own main (tests/sanitize/), no device unit among them."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

from acarsdec_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# flights.cpp launches flight.hip's kernels, and the drivers stub only the launchers the host runtime names itself: without the
# unit the table is absent (csrc/flights.h: weak references), acg_flights_enable says ACG_ESTATE and nothing else is reachable
WITHOUT = ("flights.cpp",)


def host_sources(driver):
    """(source, compiler, language flags) of every host unit and of tests/sanitize/<driver>"""
    return ([(os.path.join(_build.CSRC, u), "g++", ["-std=c++17"]) for u in _build.HOST_UNITS if u not in WITHOUT] +
            [(os.path.join(_build.CSRC, u), "gcc", ["-ffp-contract=off"]) for u in _build.HOST_C_UNITS] +
            [(os.path.join(ROOT, "tests", "sanitize", driver), "gcc", [])])


def compile_host_objects(tmp_path, driver, flags):
    """the objects of host_sources(driver) under tmp_path, each compiled with its language flags + `flags`; a compiler error fails
    the calling test with the compiler's message"""
    def one(job):
        src, cc, std = job
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        r = subprocess.run([cc] + std + flags + ["-c", src, "-o", obj], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return obj
    with ThreadPoolExecutor(max_workers=4) as pool:
        return list(pool.map(one, host_sources(driver)))
