"""The rule that lets the four library shapes share object files: a unit that _build.SEES does not name for a define has no
preprocessor line that tests it, and neither has any header -- so its object is the same whatever the library defines."""
import os
import re

from acarsdec_amd import _build

DEFINES = ("ACG_LAB", "ACG_MSK_STAMP", "ACG_MSK_SINCOS_POLY")


def defines_tested_in(path):
    """the names of DEFINES on the #if / #ifdef / #ifndef / #elif lines of a file"""
    found = set()
    for line in open(path, errors="replace"):
        if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line):
            found |= set(re.findall(r"\b(%s)\b" % "|".join(DEFINES), line))
    return found


def test_a_unit_tests_only_the_defines_it_is_built_with():
    assert set(_build.SEES) == {"-D" + d for d in DEFINES}
    for name, _flags, _in_product in _build.UNITS:
        given = {d[2:] for d, units in _build.SEES.items() if name in units}
        assert defines_tested_in(os.path.join(_build.CSRC, name)) <= given, name


def test_no_header_tests_a_build_define():
    hdrs = _build.headers()
    assert os.path.join(_build.CSRC, "acg_ctx.h") in hdrs and os.path.join(_build.CSRC, "lab", "fir_tile.inc") in hdrs
    for h in hdrs:
        if h.endswith(".py"):
            continue
        assert not defines_tested_in(h), h


def test_every_source_directly_under_csrc_is_a_unit():
    on_disk = {f for f in os.listdir(_build.CSRC) if f.endswith((".cpp", ".hip"))}
    assert on_disk == {name for name, _flags, _in_product in _build.UNITS}
    assert set(_build.HOST_UNITS) <= on_disk and all(os.path.exists(os.path.join(_build.CSRC, u)) for u in _build.HOST_C_UNITS)
