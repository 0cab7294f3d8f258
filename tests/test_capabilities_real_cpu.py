"""
The capability-table entry of real-valued facets (``SWIFTLY_FEATURE_REAL_FACETS`` = 8, ``swf::why_not_real_facets`` in
csrc/swiftly_caps.h) against literal expectations, without a GPU: the complex64 band pipeline with a power-of-two ``yN`` --
no complex128 output, no ``Q * 2^k`` -- and the two entry points it gates in the header and in the ctypes binding.
"""
import os
import re

from test_capabilities_cpu import C64, C128, _lib, sizes, supports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("swiftly_hip_prepare_facet_band_real", "swiftly_hip_prepare_facet_band_rows_real")


def test_real_facets_power_of_two_boundaries():
    assert _lib().FEATURE_REAL_FACETS == 8
    # (m, xM) = (128, 256): first and last power-of-two yN of the complex64 band pipeline
    for log_yN in (7, 16):
        assert supports("REAL_FACETS", C64, *sizes(7, 8, 1 << log_yN)), log_yN
    # yN = 2^6 passes the length gate but m <= yN has no (m, xM) instance; 2^17 is beyond the band row kernel
    assert not supports("REAL_FACETS", C64, *sizes(6, 8, 1 << 6))
    assert "real facets" in _lib().last_error()
    assert not supports("REAL_FACETS", C64, *sizes(7, 8, 1 << 17))
    assert "real facets" in _lib().last_error() and "yN" in _lib().last_error()
    # every power of two in between answers as the band pipeline does
    for log_yN in range(5, 19):
        s = sizes(min(7, log_yN), 8, 1 << log_yN)
        assert supports("REAL_FACETS", C64, *s) == supports("BAND_PIPELINE", C64, *s), log_yN
    # the facet count plays no part
    assert supports("REAL_FACETS", C64, *sizes(7, 8, 1 << 15), 65)


def test_real_facets_refusals_name_the_reason():
    lib = _lib()
    # Q * 2^k: the band pipeline runs it, the radix-Q pass in front of it has no real load
    s = sizes(7, 8, 3 << 10)
    assert supports("BAND_PIPELINE", C64, *s) and not supports("REAL_FACETS", C64, *s)
    assert "Q * 2^k" in lib.last_error() and "radix-Q" in lib.last_error() and "real load" in lib.last_error()
    # complex128 output (float64 facets): no, at sizes whose complex128 band pipeline exists
    s = sizes(7, 8, 1 << 12)
    assert supports("BAND_PIPELINE_EXPLICIT", C128, *s) and not supports("REAL_FACETS", C128, *s)
    assert "complex128" in lib.last_error()
    # (512, 4096) has no sum_finish pair: the band pipeline's own reason comes through
    s = sizes(9, 12, 1 << 12)
    assert not supports("REAL_FACETS", C64, *s)
    assert "sum_finish" in lib.last_error() and "512" in lib.last_error() and "4096" in lib.last_error()
    # unknown dtype, invalid sizes
    assert not supports("REAL_FACETS", 2, *sizes(7, 8, 1 << 12)) and not supports("REAL_FACETS", -1, *sizes(7, 8, 1 << 12))
    assert not supports("REAL_FACETS", C64, 1050, 512, 256) and "not divisible" in lib.last_error()


def test_real_entry_points_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "swiftly_hip.h"), encoding="utf-8").read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib().load()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        fn = getattr(lib, name)
        twin = getattr(lib, name[: -len("_real")])
        assert fn.restype is twin.restype and list(fn.argtypes) == list(twin.argtypes) and len(fn.argtypes) >= 13
    assert re.search(r"SWIFTLY_FEATURE_REAL_FACETS\s*=\s*8\b", code)
    # a null handle is refused before anything else, through the thread's error text
    rc = lib.swiftly_hip_prepare_facet_band_real(None, C64, None, 1, 8, 8, None, 8, 0, 0, 8, 0, None)
    assert rc == _lib().ERR_PARAM and "null" in _lib().last_error()


def test_python_wrapper_answers_from_the_table():
    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    def core(N, yN, xM):
        c = object.__new__(SwiftlyCoreHip)
        c.N, c.yN_size, c.xM_size, c.xM_yN_size = N, yN, xM, xM * yN // N
        return c

    assert core(65536, 32768, 1024).supports_real_facets()    # the 64k workload
    assert core(131072, 65536, 1024).supports_real_facets()   # 128k
    assert core(1024, 512, 256).supports_real_facets()        # plain band layout
    assert not core(3 * 4096, 3 * 1024, 1024).supports_real_facets() and "Q * 2^k" in _lib().last_error()
    assert not core(32768, 4096, 4096).supports_real_facets() and "sum_finish" in _lib().last_error()  # (512, 4096)
