"""
The half-length backward finish of real-valued facets without a device: the capability answer
(``SWIFTLY_FEATURE_REAL_FACETS_OUT_C2R`` = 13, ``why_not_real_facets_out_c2r`` of csrc/swiftly_caps.h), the entry point in the
header, the library and the binding, and the argument errors of ``SwiftlyBackward(..., half_length_finish=True)``, which are
raised before the constructor touches anything.
"""
import os
import re

import pytest
import torch

from ska_sdp_exec_swiftly_amd import SwiftlyBackward, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = "real facets out, half-length:"
ENTRY_POINT = "swiftly_hip_finish_facet_band_c2r"
# (N, yN, xM)
SIZES_64K = (65536, 32768, 1024)
OTHER_YN = {"16384": (32768, 16384, 1024), "65536": (131072, 65536, 1024), "3*2^12": (24576, 3 << 12, 256)}


def supports(feature, dtype, sizes):
    N, yN, xM = sizes
    return bool(_lib.load().swiftly_hip_supports(feature, dtype, N, yN, xM, 0))


def test_feature_number():
    assert _lib.FEATURE_REAL_FACETS_OUT_C2R == 13
    header = open(os.path.join(ROOT, "include", "swiftly_hip.h"), encoding="utf-8").read()
    assert re.search(r"SWIFTLY_FEATURE_REAL_FACETS_OUT_C2R\s*=\s*13\b", header)


def test_supported_at_32768_in_complex64():
    assert supports(_lib.FEATURE_REAL_FACETS_OUT_C2R, _lib.C64, SIZES_64K)


def test_complex128_is_refused_with_the_prefix():
    assert not supports(_lib.FEATURE_REAL_FACETS_OUT_C2R, _lib.C128, SIZES_64K)
    assert _lib.last_error().startswith(PREFIX), _lib.last_error()
    assert "complex128" in _lib.last_error()


@pytest.mark.parametrize("name", sorted(OTHER_YN))
def test_other_row_lengths_are_refused(name):
    assert not supports(_lib.FEATURE_REAL_FACETS_OUT_C2R, _lib.C64, OTHER_YN[name])
    assert _lib.last_error().startswith(PREFIX), _lib.last_error()


def test_feature_9_answers_as_before():
    """REAL_FACETS_OUT: every power-of-two yN of the backward band in complex64"""
    assert _lib.FEATURE_REAL_FACETS_OUT == 9
    assert supports(9, _lib.C64, SIZES_64K) and not supports(9, _lib.C128, SIZES_64K)
    assert supports(9, _lib.C64, OTHER_YN["16384"]) and supports(9, _lib.C64, OTHER_YN["65536"])
    assert not supports(9, _lib.C64, OTHER_YN["3*2^12"])
    assert _lib.last_error().startswith("real facet output:") and not _lib.last_error().startswith(PREFIX)


def test_entry_point_is_in_the_header_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "swiftly_hip.h"), encoding="utf-8").read()
    assert re.search(r"\bint " + ENTRY_POINT + r"\(swiftly_hip_t\* h, int dtype, const void\* in, int64_t rows, int64_t in_row_stride,", header)
    lib = _lib.load()
    fn = getattr(lib, ENTRY_POINT)  # AttributeError: not exported
    twin = lib.swiftly_hip_finish_facet_band_real
    assert fn.argtypes is not None and list(fn.argtypes) == list(twin.argtypes) and fn.restype is twin.restype


def test_backward_half_length_needs_float32_facets():
    # (no configuration, no facets, no device: the refusal comes first)
    for dtype in (None, torch.complex64, torch.float64, torch.complex128, "float64"):
        with pytest.raises(ValueError, match="half_length_finish=True needs facet_dtype=float32"):
            SwiftlyBackward(None, [], half_length_finish=True, facet_dtype=dtype)
    with pytest.raises(ValueError, match="facet_dtype must be"):
        SwiftlyBackward(None, [], half_length_finish=True, facet_dtype="no dtype")
    # with float32 facets the keyword gets past the parsing: the constructor then fails on the missing configuration
    with pytest.raises(AttributeError):
        SwiftlyBackward(None, [], half_length_finish=True, facet_dtype=torch.float32)
    with pytest.raises(AttributeError):
        SwiftlyBackward(None, [], half_length_finish=False)


def test_core_half_length_needs_real():
    """``finish_facet_band(half_length=True)`` without ``real=True`` is an argument error raised before any launch (the
    method is called unbound on an object without a handle: nothing of a core is touched)"""
    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    band_acc = torch.zeros((2, 8), dtype=torch.complex64)
    with pytest.raises(ValueError, match="half_length=True.*needs real=True"):
        SwiftlyCoreHip.finish_facet_band(object(), band_acc, (0, 8), 0, 4, half_length=True)
