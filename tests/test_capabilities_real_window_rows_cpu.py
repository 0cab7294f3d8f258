"""
The capability-table entry of float32 facets into the whole-row K1 (``SWIFTLY_FEATURE_REAL_WINDOW_ROWS`` = 11,
``swf::why_not_real_window_rows`` in csrc/swiftly_caps.h), without a GPU: supported exactly where both the window rows
(``SWIFTLY_FEATURE_WINDOW_ROWS``) and the real-load K1 in complex64 (``SWIFTLY_FEATURE_REAL_FACETS``) are, refusals that start with
``real window rows:``, and the entry point it gates in the header, the library and the ctypes binding.
"""
import os
import re

from test_capabilities_cpu import C64, C128, _lib, sizes, supports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINT = "swiftly_hip_prepare_facet_window_rows_real"
PREFIX = "real window rows:"


def _grid():
    for log_m in range(7, 11):
        for log_xM in range(8, 13):
            for yN in [1 << l for l in range(13, 17)] + [3 << 13]:
                if log_m <= log_xM:
                    yield sizes(log_m, log_xM, yN)


def test_feature_is_the_conjunction_of_window_rows_and_real_facets():
    lib = _lib()
    assert lib.FEATURE_REAL_WINDOW_ROWS == 11
    yes = []
    for s in _grid():
        want = supports("WINDOW_ROWS", C64, *s) and supports("REAL_FACETS", C64, *s)
        got = supports("REAL_WINDOW_ROWS", C64, *s)
        assert got == want, s
        if got:
            yes.append(s)
        else:
            assert lib.last_error().startswith(PREFIX), (s, lib.last_error())
        # complex128 output and an unknown dtype: no, with the feature's own text
        for dtype in (C128, -1, 2):
            assert not supports("REAL_WINDOW_ROWS", dtype, *s), (s, dtype)
            assert lib.last_error().startswith(PREFIX), (s, dtype, lib.last_error())
    # the sizes the kernel exists for: yN 32768, m 512 and a sum_finish pair with xM <= 2048 -- the 64k workload among them
    assert set(yes) == {sizes(9, 10, 1 << 15), sizes(9, 11, 1 << 15)} and (65536, 32768, 1024) in yes


def test_refusals_name_the_reason():
    lib = _lib()
    # Q * 2^k: no window rows and no real load
    assert not supports("REAL_WINDOW_ROWS", C64, *sizes(9, 10, 3 << 13)) and lib.last_error().startswith(PREFIX)
    # window rows exist, the output type does not
    s = sizes(9, 10, 1 << 15)
    assert supports("WINDOW_ROWS", C64, *s) and supports("REAL_FACETS", C64, *s) and supports("REAL_WINDOW_ROWS", C64, *s)
    assert not supports("REAL_WINDOW_ROWS", C128, *s)
    assert lib.last_error().startswith(PREFIX) and "complex128" in lib.last_error()
    # real facets exist, window rows do not: 16384-point rows; m = 256
    for s in (sizes(9, 10, 1 << 14), sizes(8, 10, 1 << 15)):
        assert supports("REAL_FACETS", C64, *s) and not supports("WINDOW_ROWS", C64, *s)
        assert not supports("REAL_WINDOW_ROWS", C64, *s)
        assert lib.last_error().startswith(PREFIX) and "window rows: needs yN 32768" in lib.last_error()
    # invalid sizes: the size check's own text, as for every feature
    assert not supports("REAL_WINDOW_ROWS", C64, 1050, 512, 256) and "not divisible" in lib.last_error()


def test_entry_point_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "swiftly_hip.h"), encoding="utf-8").read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+" + ENTRY_POINT + r"\s*\(", code)
    assert re.search(r"SWIFTLY_FEATURE_REAL_WINDOW_ROWS\s*=\s*11\b", code)
    lib = _lib().load()
    fn, twin = getattr(lib, ENTRY_POINT), lib.swiftly_hip_prepare_facet_window_rows  # exported: ctypes resolved the symbol
    assert fn.restype is twin.restype and list(fn.argtypes) == list(twin.argtypes) and len(fn.argtypes) == 17
    # a null handle and a missing window table are refused before anything else, through the thread's error text
    rc = fn(None, C64, None, 1, 8, 8, None, 512, 0, 0, 8, 0, 0, None, 1, 512, None)
    assert rc == _lib().ERR_PARAM and "no windows" in _lib().last_error()


def test_python_wrapper_answers_from_the_table():
    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    def core(N, yN, xM):
        c = object.__new__(SwiftlyCoreHip)
        c.N, c.yN_size, c.xM_size, c.xM_yN_size = N, yN, xM, xM * yN // N
        return c

    lib = _lib()
    c = core(65536, 32768, 1024)
    assert c._supports(lib.FEATURE_REAL_WINDOW_ROWS, None)  # pylint: disable=protected-access
    assert not core(32768, 16384, 1024)._supports(lib.FEATURE_REAL_WINDOW_ROWS, None)  # pylint: disable=protected-access
    assert lib.last_error().startswith(PREFIX)
