"""
``SWIFTLY_FEATURE_AXIS1_COLUMNS`` = 18 (``why_not_axis1_columns`` of csrc/swiftly_caps.h) without a device: the gate of
``swiftly_hip_prepare_facet_columns_axis1`` -- K2 of the axis-1-first order with the contiguous-axis finish inside the first
pass of its four-step.  Yes for complex64 at the two sizes with an instance; no, with a reason that names yN, m and xM,
everywhere else; features 0 .. 17 answer what they answered before; the symbol is in the header and in the binding.
"""
import ctypes
import os
import re

import pytest

from ska_sdp_exec_swiftly_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = "axis-1 columns:"
# (N, yN, xM)
SUPPORTED = {"64k[1]-n32k-1k": (65536, 32768, 1024), "32k[1]-n16k-512": (32768, 16384, 512)}
REFUSED = {
    "yN 8192: plain band layout": (16384, 8192, 512),
    "yN 3 * 2^13": (49152, 3 << 13, 256),
    "yN 65536: n2 would be 2048": (131072, 65536, 1024),
    "xM 4096: no placed mode": (262144, 32768, 4096),
}


def supports(feature, dtype, sizes, n_facets=0):
    N, yN, xM = sizes
    return bool(_lib.load().swiftly_hip_supports(feature, dtype, N, yN, xM, n_facets))


def names_the_sizes(text, sizes):
    N, yN, xM = sizes
    return f"yN {yN}" in text and f"m {xM * yN // N}" in text and f"xM {xM}" in text


def test_feature_number_and_symbol():
    assert _lib.FEATURE_AXIS1_COLUMNS == 18
    header = open(os.path.join(ROOT, "include", "swiftly_hip.h"), encoding="utf-8").read()
    assert re.search(r"SWIFTLY_FEATURE_AXIS1_COLUMNS\s*=\s*18\b", header)
    assert re.search(r"\bint\s+swiftly_hip_prepare_facet_columns_axis1\s*\(", header)
    fn = _lib.load().swiftly_hip_prepare_facet_columns_axis1
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 19


@pytest.mark.parametrize("name", sorted(SUPPORTED))
def test_supported_in_complex64(name):
    assert supports(18, _lib.C64, SUPPORTED[name]), _lib.last_error()


@pytest.mark.parametrize("name", sorted(SUPPORTED))
def test_complex128_is_refused(name):
    assert not supports(18, _lib.C128, SUPPORTED[name])
    why = _lib.last_error()
    assert why.startswith(PREFIX) and "complex64" in why and names_the_sizes(why, SUPPORTED[name]), why


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_other_sizes_are_refused_with_the_sizes_in_the_reason(name):
    assert not supports(18, _lib.C64, REFUSED[name])
    why = _lib.last_error()
    assert why.startswith(PREFIX) and names_the_sizes(why, REFUSED[name]), why


#: features 0 .. 17 in (complex64, complex128) at the sizes above with three facets, recorded from the capability table
#: as it stood before feature 18 was added
BEFORE = {
    "64k[1]-n32k-1k": ("111111111111110000", "001011110000001100"),
    "32k[1]-n16k-512": ("111110111100000000", "001010110000001100"),
    "yN 8192: plain band layout": ("111100111100000000", "001000110000001100"),
    "yN 3 * 2^13": ("111100110010000000", "000000010000000000"),
    "yN 65536: n2 would be 2048": ("111110111110000011", "000010010000000000"),
    "xM 4096: no placed mode": ("000110100100010000", "000010100000000100"),
}


@pytest.mark.parametrize("name", sorted(BEFORE))
def test_features_0_to_17_answer_as_before(name):
    sizes = {**SUPPORTED, **REFUSED}[name]
    for dtype, want in zip((_lib.C64, _lib.C128), BEFORE[name]):
        got = "".join(str(int(supports(f, dtype, sizes, 3))) for f in range(18))
        assert got == want, (name, dtype, got)
    assert not supports(19, _lib.C64, sizes) and "unknown feature" in _lib.last_error()
