"""
The half-length forms on 65536-point rows without a device: the capability answers of
``SWIFTLY_FEATURE_REAL_FACETS_RFFT_64K`` = 16 (``why_not_real_facets_rfft_64k`` of csrc/swiftly_caps.h) and
``SWIFTLY_FEATURE_REAL_FACETS_OUT_C2R_64K`` = 17 (``why_not_real_facets_out_c2r_64k``), their numbers in the header and the
binding, and that the features next to them -- 12 and 13 (the 32768-point forms), 8 and 9 (real facets in and out) -- answer
at every size here what they answered before the two existed.
"""
import os
import re

import pytest

from ska_sdp_exec_swiftly_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#: feature: (name in the header, prefix of its refusals)
NEW = {16: ("SWIFTLY_FEATURE_REAL_FACETS_RFFT_64K", "real facets, half-length:"),
       17: ("SWIFTLY_FEATURE_REAL_FACETS_OUT_C2R_64K", "real facets out, half-length:")}
# (N, yN, xM)
SUPPORTED = {"xM 1024": (131072, 65536, 1024), "xM 256": (131072, 65536, 256)}
REFUSED = {"16384": (32768, 16384, 1024), "32768": (65536, 32768, 1024), "3*2^12": (24576, 3 << 12, 256)}


def supports(feature, dtype, sizes):
    N, yN, xM = sizes
    return bool(_lib.load().swiftly_hip_supports(feature, dtype, N, yN, xM, 0))


def test_feature_numbers():
    assert _lib.FEATURE_REAL_FACETS_RFFT_64K == 16 and _lib.FEATURE_REAL_FACETS_OUT_C2R_64K == 17
    header = open(os.path.join(ROOT, "include", "swiftly_hip.h"), encoding="utf-8").read()
    for number, (name, _) in NEW.items():
        assert re.search(name + r"\s*=\s*%d\b" % number, header), name


@pytest.mark.parametrize("feature", sorted(NEW))
@pytest.mark.parametrize("name", sorted(SUPPORTED))
def test_supported_at_65536_in_complex64(feature, name):
    assert supports(feature, _lib.C64, SUPPORTED[name]), _lib.last_error()


@pytest.mark.parametrize("feature", sorted(NEW))
@pytest.mark.parametrize("name", sorted(SUPPORTED))
def test_complex128_is_refused_with_the_prefix(feature, name):
    assert not supports(feature, _lib.C128, SUPPORTED[name])
    assert _lib.last_error().startswith(NEW[feature][1]), _lib.last_error()


@pytest.mark.parametrize("feature", sorted(NEW))
@pytest.mark.parametrize("name", sorted(REFUSED))
def test_other_row_lengths_are_refused_with_the_prefix(feature, name):
    assert not supports(feature, _lib.C64, REFUSED[name])
    assert _lib.last_error().startswith(NEW[feature][1]), _lib.last_error()


def test_features_12_13_8_and_9_answer_as_before():
    """12 / 13: yN 32768 in complex64 and nothing else (65536 refused with their prefix); 8 / 9: every power-of-two yN here in
    complex64, no Q * 2^k, no complex128"""
    assert (_lib.FEATURE_REAL_FACETS, _lib.FEATURE_REAL_FACETS_OUT) == (8, 9)
    assert (_lib.FEATURE_REAL_FACETS_RFFT, _lib.FEATURE_REAL_FACETS_OUT_C2R) == (12, 13)
    for half, real in ((12, 8), (13, 9)):
        prefix = NEW[half + 4][1]
        for name, sizes in {**SUPPORTED, **REFUSED}.items():
            assert supports(half, _lib.C64, sizes) == (name == "32768"), (half, name)
            if name != "32768":
                assert _lib.last_error().startswith(prefix), (half, name, _lib.last_error())
            assert not supports(half, _lib.C128, sizes) and _lib.last_error().startswith(prefix), (half, name)
            assert supports(real, _lib.C64, sizes) == (name != "3*2^12"), (real, name)
            assert not supports(real, _lib.C128, sizes), (real, name)
            assert not _lib.last_error().startswith(prefix), (real, name, _lib.last_error())
