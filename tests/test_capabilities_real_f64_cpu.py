"""
Float64 facets through the complex128 band passes, without a device: the two capability answers
(``SWIFTLY_FEATURE_REAL_FACETS_F64`` = 14, ``SWIFTLY_FEATURE_REAL_FACETS_OUT_F64`` = 15; ``why_not_real_facets_f64`` /
``why_not_real_facets_out_f64`` of csrc/swiftly_caps.h) against literal expectations, the two entry points in the header, the
library and the binding, that features 8 / 9 answer as before, and what the constructors refuse before they touch anything.
"""
import os
import re
import types

import numpy
import pytest
import torch

from test_capabilities_cpu import C64, C128, _lib, sizes, supports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN_PREFIX, OUT_PREFIX = "real facets, float64: ", "real facet output, float64: "
FEATURES = {"REAL_FACETS_F64": (14, IN_PREFIX), "REAL_FACETS_OUT_F64": (15, OUT_PREFIX)}
ENTRY_POINTS = {"swiftly_hip_prepare_facet_band_real64": "swiftly_hip_prepare_facet_band_real",
                "swiftly_hip_finish_facet_band_real64": "swiftly_hip_finish_facet_band_real"}
# (N, yN, xM)
SMALL = (1024, 512, 256)
N16K = (65536, 16384, 1024)  # 64k[1]-n16k-1k
N32K = (131072, 32768, 1024)  # 128k[1]-n32k-1k


def header():
    return open(os.path.join(ROOT, "include", "swiftly_hip.h"), encoding="utf-8").read()


@pytest.mark.parametrize("name", sorted(FEATURES))
def test_feature_numbers(name):
    number, _ = FEATURES[name]
    assert getattr(_lib(), "FEATURE_" + name) == number
    assert re.search(r"SWIFTLY_FEATURE_" + name + r"\s*=\s*" + str(number) + r"\b", header())


@pytest.mark.parametrize("name", sorted(FEATURES))
def test_yes_in_complex128(name):
    for s in (SMALL, N16K, N32K):
        assert supports(name, C128, *s), (name, s, _lib().last_error())
    # the facet count plays no part
    assert supports(name, C128, *SMALL, 65)


def test_the_answers_are_those_of_the_complex128_band_passes():
    """feature 14 = BAND_PIPELINE_EXPLICIT in complex128 (no facet count), feature 15 = BACKWARD_BAND_EXPLICIT in complex128,
    at every power-of-two yN with (m, xM) = (128, 256)"""
    for log_yN in range(5, 18):
        s = sizes(min(7, log_yN), 8, 1 << log_yN)
        assert supports("REAL_FACETS_F64", C128, *s) == supports("BAND_PIPELINE_EXPLICIT", C128, *s), log_yN
        assert supports("REAL_FACETS_F64", C128, *s) == (7 <= log_yN <= 15), log_yN
        assert supports("REAL_FACETS_OUT_F64", C128, *s) == supports("BACKWARD_BAND_EXPLICIT", C128, *s), log_yN
        assert supports("REAL_FACETS_OUT_F64", C128, *s) == (6 <= log_yN <= 15), log_yN


@pytest.mark.parametrize("name", sorted(FEATURES))
def test_refusals_carry_the_prefix(name):
    lib = _lib()
    _, prefix = FEATURES[name]
    # complex64: no, and the reason names the float32 features
    for s in (SMALL, N16K):
        assert not supports(name, C64, *s)
        err = lib.last_error()
        assert err.startswith(prefix) and "8 / 9" in err and "REAL_FACETS" in err, err
    # Q * 2^k and yN = 65536: the complex128 pass's own reason comes through, prefixed
    for s in (sizes(7, 8, 3 << 10), sizes(7, 8, 1 << 16)):
        assert not supports(name, C128, *s)
        assert lib.last_error().startswith(prefix + "complex128 "), lib.last_error()
    # unknown dtypes; invalid sizes
    for dtype in (2, -1):
        assert not supports(name, dtype, *SMALL)
        assert lib.last_error().startswith(prefix) and "dtype" in lib.last_error()
    assert not supports(name, C128, 1050, 512, 256) and "not divisible" in lib.last_error()


def test_forward_needs_a_complex128_instance_for_m_and_xM():
    """(m, xM) = (512, 2048) and m = 1024 have complex64 instances and no complex128 one: the forward feature says no; the
    backward band has no such table (its gather-sum pass takes every power-of-two m), so feature 15 says yes"""
    lib = _lib()
    for pair in ((9, 11), (10, 11)):
        s = sizes(*pair, 1 << 12)
        assert supports("BAND_PIPELINE", C64, *s)
        assert not supports("REAL_FACETS_F64", C128, *s)
        assert lib.last_error().startswith(IN_PREFIX + "complex128 band pipeline") and "instance" in lib.last_error()
        assert supports("REAL_FACETS_OUT_F64", C128, *s)


def test_features_8_and_9_still_refuse_complex128():
    lib = _lib()
    assert (lib.FEATURE_REAL_FACETS, lib.FEATURE_REAL_FACETS_OUT) == (8, 9)
    for s in (SMALL, N16K):
        assert supports("REAL_FACETS", C64, *s) and supports("REAL_FACETS_OUT", C64, *s)
        assert not supports("REAL_FACETS", C128, *s)
        assert lib.last_error().startswith("real facets: ") and "complex128" in lib.last_error()
        assert not supports("REAL_FACETS_OUT", C128, *s)
        assert lib.last_error().startswith("real facet output: ") and "complex128" in lib.last_error()
    for name in ("REAL_WINDOW_ROWS", "REAL_FACETS_RFFT", "REAL_FACETS_OUT_C2R"):
        assert not supports(name, C128, *N32K) and "complex128" in lib.last_error()


@pytest.mark.parametrize("symbol", sorted(ENTRY_POINTS))
def test_entry_points_are_in_the_header_exported_and_bound(symbol):
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)

    def params_of(name):
        return re.sub(r"\s+", " ", re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code).group(1))

    twin_name = ENTRY_POINTS[symbol]
    assert params_of(symbol) == params_of(twin_name)
    lib = _lib().load()
    fn, twin = getattr(lib, symbol), getattr(lib, twin_name)  # AttributeError: not exported
    assert fn.argtypes is not None and list(fn.argtypes) == list(twin.argtypes) and fn.restype is twin.restype
    assert len(fn.argtypes) == 13
    # a null handle is refused before anything else
    rc = fn(None, C128, None, 1, 8, 8, None, 8, 0, 0, 8, 0, None) if "prepare" in symbol else \
        fn(None, C128, None, 1, 8, 0, 8, None, 8, 0, 8, None, None)
    assert rc == _lib().ERR_PARAM and "null" in _lib().last_error()


def _stand_in(N, yN, xM):
    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    c = object.__new__(SwiftlyCoreHip)
    c.N, c.yN_size, c.xM_size, c.xM_yN_size = N, yN, xM, xM * yN // N
    return c


def test_python_wrappers_answer_from_the_table():
    for s in (SMALL, N16K, N32K):
        core = _stand_in(*s)
        assert core.supports_real_facets_f64() and core.supports_real_facets_out_f64()
    core = _stand_in(131072, 65536, 1024)
    assert not core.supports_real_facets_f64() and _lib().last_error().startswith(IN_PREFIX)
    assert not core.supports_real_facets_out_f64() and _lib().last_error().startswith(OUT_PREFIX)
    core = _stand_in(3 * 4096, 3 * 1024, 1024)
    assert not core.supports_real_facets_f64() and not core.supports_real_facets_out_f64()


def test_core_methods_refuse_other_dtypes_before_any_launch():
    """(the methods are called unbound on an object without a handle: nothing of a core is touched)"""
    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    for dtype in (torch.float32, torch.complex128, torch.complex64):
        with pytest.raises(ValueError, match="float64"):
            SwiftlyCoreHip.prepare_facet_band_float64(object(), torch.zeros((2, 8), dtype=dtype), 0, (0, 16))
    with pytest.raises(ValueError, match="row-major"):
        SwiftlyCoreHip.prepare_facet_band_float64(object(), torch.zeros((2, 16), dtype=torch.float64)[:, ::2], 0, (0, 16))
    for dtype in (torch.complex64, torch.float64):
        with pytest.raises(ValueError, match="complex128"):
            SwiftlyCoreHip.finish_facet_band_float64(object(), torch.zeros((2, 8), dtype=dtype), (0, 8), 0, 4)
    acc = torch.zeros((2, 8), dtype=torch.complex128)
    with pytest.raises(ValueError, match="float64"):
        SwiftlyCoreHip.finish_facet_band_float64(object(), acc, (0, 8), 0, 4, out=torch.zeros((2, 4), dtype=torch.float32))
    for bad in (torch.zeros((2, 5), dtype=torch.float64), torch.zeros((2, 8), dtype=torch.float64)[:, ::2]):
        with pytest.raises(ValueError, match="unit column stride"):
            SwiftlyCoreHip.finish_facet_band_float64(object(), acc, (0, 8), 0, 4, out=bad)


def test_forward_constructor_refusals():
    """before the constructor touches a configuration or a device (there is none here)"""
    from ska_sdp_exec_swiftly_amd import FacetConfig, SwiftlyForward

    fc = FacetConfig(0, 0, 8)
    f64 = numpy.zeros((8, 8))
    # data that are not all float64 (float32, complex128, one of two, a strided tensor, none at all)
    for data in ([numpy.zeros((8, 8), dtype=numpy.float32)], [numpy.zeros((8, 8), dtype=complex)],
                 [f64, numpy.zeros((8, 8), dtype=numpy.float32)], [torch.zeros((8, 16), dtype=torch.float64)[:, ::2]], []):
        for value in (torch.float64, "float64", numpy.float64):
            with pytest.raises(ValueError, match="facet_dtype") as info:
                SwiftlyForward(None, [(fc, d) for d in data], facet_dtype=value)
            assert "facet_dtype must be float32 or None" in str(info.value) and "float64" in str(info.value)
    # the half-length K1 is a float32 form
    with pytest.raises(ValueError, match="half_length_k1=True needs facet_dtype=float32"):
        SwiftlyForward(None, [(fc, f64)], facet_dtype=torch.float64, half_length_k1=True)
    # any other value: the sentence of every forward class, with what this class adds
    for bad in (torch.complex64, torch.complex128, torch.float16, "real", 32):
        with pytest.raises(ValueError, match="facet_dtype must be float32 or None") as info:
            SwiftlyForward(None, [(fc, f64)], facet_dtype=bad)
        assert "float64" in str(info.value)
    # float64 facets with the keyword get past the parsing: the constructor then fails on the missing configuration
    with pytest.raises(AttributeError):
        SwiftlyForward(None, [(fc, f64)], facet_dtype=torch.float64)
    with pytest.raises(AttributeError):
        SwiftlyForward(None, [(fc, torch.zeros((8, 8), dtype=torch.float64))], facet_dtype="float64")


def test_distributed_forward_keeps_its_list():
    from ska_sdp_exec_swiftly_amd.distributed import DistributedForward
    from ska_sdp_exec_swiftly_amd.facet_dtype import FORWARD, FORWARD_SINGLE

    assert FORWARD == ("float32",) and FORWARD_SINGLE == ("float32", "float64")
    with pytest.raises(ValueError, match="facet_dtype must be float32 or None$"):
        DistributedForward(None, [], [], facet_dtype=torch.float64)


def test_backward_properties_before_any_data():
    """``SwiftlyBackward`` touches its core only when data arrives: a stand-in configuration is enough"""
    import ska_sdp_exec_swiftly_amd as sw

    cfg = types.SimpleNamespace(core=_stand_in(*SMALL))
    facets = [sw.FacetConfig(0, 0, 352)]
    bwd = sw.SwiftlyBackward(cfg, facets, wave_axis=1, dtype=torch.complex128, facet_dtype=torch.float64)
    assert bwd.facet_dtype == torch.float64 and bwd.real_finish_native is True and bwd.half_length_finish is False
    bwd = sw.SwiftlyBackward(cfg, facets, wave_axis=0, dtype=torch.complex128, facet_dtype=torch.float64)
    assert bwd.real_finish_native is False
    bwd = sw.SwiftlyBackward(cfg, facets, dtype=torch.complex128, facet_dtype=torch.float64)
    assert bwd.real_finish_native is None  # (schedule not resolved)
    # float32 facets are what they were
    bwd = sw.SwiftlyBackward(cfg, facets, wave_axis=1, facet_dtype=torch.float32)
    assert bwd.real_finish_native is True
    # complex64 data with float64 facets: refused where the data's dtype is stated
    with pytest.raises(ValueError, match="does not match"):
        sw.SwiftlyBackward(cfg, facets, wave_axis=1, dtype=torch.complex64, facet_dtype=torch.float64)
    with pytest.raises(ValueError, match="half_length_finish=True needs facet_dtype=float32"):
        sw.SwiftlyBackward(cfg, facets, wave_axis=1, dtype=torch.complex128, facet_dtype=torch.float64, half_length_finish=True)
    # yN = 65536 has no complex128 backward band: the explicit request is refused as before
    big = types.SimpleNamespace(core=_stand_in(131072, 65536, 1024))
    with pytest.raises(ValueError, match="complex128 backward band"):
        sw.SwiftlyBackward(big, [sw.FacetConfig(0, 0, 1024)], wave_axis=1, dtype=torch.complex128, facet_dtype=torch.float64)
