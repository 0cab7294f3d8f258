"""
The half-length K1 of real-valued facets without a device: the capability answer (``SWIFTLY_FEATURE_REAL_FACETS_RFFT`` = 12,
``why_not_real_facets_rfft`` of csrc/swiftly_caps.h), the two entry points in the header, the library and the binding, and the
argument errors of ``SwiftlyForward(..., half_length_k1=True)``, which are raised before the constructor touches anything.
"""
import os
import re

import pytest
import torch

from ska_sdp_exec_swiftly_amd import SwiftlyForward, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = "real facets, half-length:"
ENTRY_POINTS = ("swiftly_hip_prepare_facet_band_rfft", "swiftly_hip_prepare_facet_band_rows_rfft")
# (N, yN, xM)
SIZES_64K = (65536, 32768, 1024)
OTHER_YN = {"16384": (32768, 16384, 1024), "65536": (131072, 65536, 1024), "3*2^12": (24576, 3 << 12, 256)}


def supports(feature, dtype, sizes):
    N, yN, xM = sizes
    return bool(_lib.load().swiftly_hip_supports(feature, dtype, N, yN, xM, 0))


def test_feature_number():
    assert _lib.FEATURE_REAL_FACETS_RFFT == 12
    header = open(os.path.join(ROOT, "include", "swiftly_hip.h"), encoding="utf-8").read()
    assert re.search(r"SWIFTLY_FEATURE_REAL_FACETS_RFFT\s*=\s*12\b", header)


def test_supported_at_32768_in_complex64():
    assert supports(_lib.FEATURE_REAL_FACETS_RFFT, _lib.C64, SIZES_64K)


def test_complex128_is_refused_with_the_prefix():
    assert not supports(_lib.FEATURE_REAL_FACETS_RFFT, _lib.C128, SIZES_64K)
    assert PREFIX in _lib.last_error()
    assert _lib.last_error().startswith(PREFIX)


@pytest.mark.parametrize("name", sorted(OTHER_YN))
def test_other_row_lengths_are_refused(name):
    assert not supports(_lib.FEATURE_REAL_FACETS_RFFT, _lib.C64, OTHER_YN[name])
    assert _lib.last_error().startswith(PREFIX), _lib.last_error()


def test_features_8_and_11_answer_as_before():
    """REAL_FACETS: every power-of-two yN of the band pipeline in complex64; REAL_WINDOW_ROWS: 32768-point rows with m = 512"""
    assert _lib.FEATURE_REAL_FACETS == 8 and _lib.FEATURE_REAL_WINDOW_ROWS == 11
    assert supports(8, _lib.C64, SIZES_64K) and supports(11, _lib.C64, SIZES_64K)
    assert not supports(8, _lib.C128, SIZES_64K) and not supports(11, _lib.C128, SIZES_64K)
    assert supports(8, _lib.C64, OTHER_YN["16384"]) and not supports(11, _lib.C64, OTHER_YN["16384"])
    assert supports(8, _lib.C64, OTHER_YN["65536"]) and not supports(11, _lib.C64, OTHER_YN["65536"])
    assert not supports(8, _lib.C64, OTHER_YN["3*2^12"]) and not supports(11, _lib.C64, OTHER_YN["3*2^12"])
    assert not _lib.last_error().startswith(PREFIX)


@pytest.mark.parametrize("symbol", ENTRY_POINTS)
def test_entry_points_are_in_the_header_exported_and_bound(symbol):
    header = open(os.path.join(ROOT, "include", "swiftly_hip.h"), encoding="utf-8").read()
    assert re.search(r"\bint " + symbol + r"\(swiftly_hip_t\* h, int dtype, const void\* in,", header)
    lib = _lib.load()
    fn = getattr(lib, symbol)  # AttributeError: not exported
    twin = getattr(lib, symbol.replace("_rfft", "_real"))
    assert fn.argtypes is not None and list(fn.argtypes) == list(twin.argtypes) and fn.restype is twin.restype


def test_forward_half_length_needs_float32_facets():
    # (no configuration, no facets, no device: the refusal comes first)
    for dtype in (None,):
        with pytest.raises(ValueError, match="half_length_k1=True needs facet_dtype=float32"):
            SwiftlyForward(None, [], half_length_k1=True, facet_dtype=dtype)
    with pytest.raises(ValueError, match="facet_dtype must be float32 or None"):
        SwiftlyForward(None, [], half_length_k1=True, facet_dtype=torch.complex64)
    # with float32 facets the keyword gets past the parsing: the constructor then fails on the missing configuration
    with pytest.raises(AttributeError):
        SwiftlyForward(None, [], half_length_k1=True, facet_dtype=torch.float32)
    with pytest.raises(AttributeError):
        SwiftlyForward(None, [], half_length_k1=False)
