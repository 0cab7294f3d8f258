"""
The capability-table entry of real-valued facets on the way OUT (``SWIFTLY_FEATURE_REAL_FACETS_OUT`` = 9,
``swf::why_not_real_facets_out`` in csrc/swiftly_caps.h) against literal expectations, without a GPU: the complex64 backward
band with a power-of-two ``yN`` -- no complex128 input, no ``Q * 2^k`` -- the entry point it gates in the header and in the
ctypes binding, the Python gate, and the ``facet_dtype`` argument of ``SwiftlyBackward`` as far as it is checked before any
data arrives.
"""
import os
import re

import pytest

from test_capabilities_cpu import C64, C128, _lib, sizes, supports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINT = "swiftly_hip_finish_facet_band_real"


def test_real_facets_out_follows_the_backward_band():
    assert _lib().FEATURE_REAL_FACETS_OUT == 9
    # (m, xM) = (128, 256): every power-of-two yN answers as the complex64 backward band does; 64 .. 65536 are taken
    for log_yN in range(5, 19):
        s = sizes(min(7, log_yN), 8, 1 << log_yN)
        assert supports("REAL_FACETS_OUT", C64, *s) == supports("BACKWARD_BAND", C64, *s), log_yN
        assert supports("REAL_FACETS_OUT", C64, *s) == (6 <= log_yN <= 16), log_yN
    assert not supports("REAL_FACETS_OUT", C64, *sizes(7, 8, 1 << 17))
    assert _lib().last_error().startswith("real facet output: ") and "yN" in _lib().last_error()
    # the facet count plays no part
    assert supports("REAL_FACETS_OUT", C64, *sizes(7, 8, 1 << 15), 65)


def test_real_facets_out_refusals_name_the_reason():
    lib = _lib()
    # Q * 2^k: the backward band runs it, the radix-Q pass behind it has no real store
    s = sizes(7, 8, 3 << 10)
    assert supports("BACKWARD_BAND", C64, *s) and not supports("REAL_FACETS_OUT", C64, *s)
    err = lib.last_error()
    assert err.startswith("real facet output: ") and "Q * 2^k" in err and "radix-Q" in err and "real store" in err
    # complex128 input (float64 facets): no, at sizes whose complex128 backward band exists
    s = sizes(7, 8, 1 << 12)
    assert supports("BACKWARD_BAND_EXPLICIT", C128, *s) and not supports("REAL_FACETS_OUT", C128, *s)
    assert lib.last_error().startswith("real facet output: ") and "complex128" in lib.last_error()
    # xM not a power of two: the backward band's own reason comes through, prefixed
    assert not supports("REAL_FACETS_OUT", C64, 3 * 4096, 4096, 3 * 256)
    assert lib.last_error().startswith("real facet output: backward band")
    # unknown dtypes, invalid sizes
    for dtype in (2, -1):
        assert not supports("REAL_FACETS_OUT", dtype, *sizes(7, 8, 1 << 12))
        assert lib.last_error().startswith("real facet output: ") and "dtype" in lib.last_error()
    assert not supports("REAL_FACETS_OUT", C64, 1050, 512, 256) and "not divisible" in lib.last_error()


def test_real_out_entry_point_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "swiftly_hip.h"), encoding="utf-8").read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib().load()
    assert re.search(r"\bint\s+" + ENTRY_POINT + r"\s*\(", code)
    assert re.search(r"SWIFTLY_FEATURE_REAL_FACETS_OUT\s*=\s*9\b", code)
    fn, twin = getattr(lib, ENTRY_POINT), lib.swiftly_hip_finish_facet_band
    assert fn.restype is twin.restype and list(fn.argtypes) == list(twin.argtypes) and len(fn.argtypes) == 13
    # the declared parameter list is the twin's
    def params_of(name):
        return re.sub(r"\s+", " ", re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code).group(1))

    assert params_of(ENTRY_POINT) == params_of("swiftly_hip_finish_facet_band")
    # a null handle is refused before anything else, through the thread's error text
    rc = fn(None, C64, None, 1, 8, 0, 8, None, 8, 0, 8, None, None)
    assert rc == _lib().ERR_PARAM and "null" in _lib().last_error()


def _stand_in(N, yN, xM):
    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    c = object.__new__(SwiftlyCoreHip)
    c.N, c.yN_size, c.xM_size, c.xM_yN_size = N, yN, xM, xM * yN // N
    return c


def test_python_wrapper_answers_from_the_table():
    assert _stand_in(65536, 32768, 1024).supports_real_facets_out()    # the 64k workload
    assert _stand_in(131072, 65536, 1024).supports_real_facets_out()   # 128k
    assert _stand_in(1024, 512, 256).supports_real_facets_out()        # plain band layout
    assert not _stand_in(3 * 4096, 3 * 1024, 1024).supports_real_facets_out() and "Q * 2^k" in _lib().last_error()


def test_backward_facet_dtype_is_checked_at_construction():
    """``SwiftlyBackward`` touches its core only when data arrives: a stand-in configuration is enough here"""
    import types

    import numpy
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    cfg = types.SimpleNamespace(core=_stand_in(1024, 512, 256))
    facets = [sw.FacetConfig(0, 0, 352)]
    for bad in (torch.int32, torch.float16, numpy.int64, "nonsense"):
        with pytest.raises(ValueError, match="facet_dtype"):
            sw.SwiftlyBackward(cfg, facets, facet_dtype=bad)
    # the precision of the data, where `dtype` states it at construction
    for dtype, facet_dtype in ((torch.complex64, torch.float64), (torch.complex128, torch.float32),
                               (torch.complex64, torch.complex128), (numpy.complex64, numpy.float64)):
        with pytest.raises(ValueError, match="does not match"):
            sw.SwiftlyBackward(cfg, facets, dtype=dtype, facet_dtype=facet_dtype)
    # what is accepted, and what the properties say before any data
    bwd = sw.SwiftlyBackward(cfg, facets)
    assert bwd.facet_dtype is None and bwd.real_finish_native is None
    bwd = sw.SwiftlyBackward(cfg, facets, dtype=torch.complex64, facet_dtype=torch.complex64)
    assert bwd.facet_dtype == torch.complex64
    bwd = sw.SwiftlyBackward(cfg, facets, facet_dtype=numpy.float32)
    assert bwd.facet_dtype == torch.float32 and bwd.real_finish_native is None  # (schedule not resolved yet)
    bwd = sw.SwiftlyBackward(cfg, facets, wave_axis=1, facet_dtype=torch.float32)
    assert bwd.facet_dtype == torch.float32 and bwd.real_finish_native is True
    bwd = sw.SwiftlyBackward(cfg, facets, wave_axis=0, facet_dtype=torch.float32)
    assert bwd.real_finish_native is False
    bwd = sw.SwiftlyBackward(cfg, facets, wave_axis=0, dtype=torch.complex128, facet_dtype=torch.float64)
    assert bwd.facet_dtype == torch.float64 and bwd.real_finish_native is False
    # Q * 2^k on the band schedule: real facets through the complex finish
    cq = types.SimpleNamespace(core=_stand_in(3 * 4096, 3 * 1024, 1024))
    bwd = sw.SwiftlyBackward(cq, [sw.FacetConfig(0, 0, 2048)], wave_axis=1, facet_dtype=torch.float32)
    assert bwd.real_finish_native is False
