"""
The two capability-table entries of the complex128 backward band schedule (``swiftly_hip_supports``, csrc/swiftly_caps.h)
against literal expectations, without a GPU:

* ``BACKWARD_BAND_EXPLICIT`` (6): what ``BACKWARD_BAND`` answers in complex64; in complex128 a power-of-two ``yN`` of
  64 .. 32768 with power-of-two ``xM`` and ``m``, no ``Q * 2^k``.  ``BACKWARD_BAND`` itself keeps answering no for complex128.
* ``SPLIT_PREPARE`` (7): what ``FUSED_SUBGRID`` answers in complex64; in complex128 the pairs of ``SPLIT_PAIRS_C128``, at
  most 64 facets.
"""
from test_capabilities_cpu import C64, C128, _lib, sizes, supports


def test_backward_band_explicit_complex128_boundaries():
    for log_yN, want in ((5, False), (6, True), (15, True), (16, False)):
        assert supports("BACKWARD_BAND_EXPLICIT", C128, *sizes(0, 0, 1 << log_yN)) == want, log_yN
        if not want:
            assert "complex128" in _lib().last_error()
        # the default gate still answers no for complex128, at every length
        assert not supports("BACKWARD_BAND", C128, *sizes(0, 0, 1 << log_yN))
    # no radix-Q gather-sum pass in float64
    for k in (6, 10, 15):
        assert not supports("BACKWARD_BAND_EXPLICIT", C128, *sizes(5, 5, 3 << k)), k
        assert "complex128" in _lib().last_error() and "Q * 2^k" in _lib().last_error()
    # xM (and with it m) not a power of two; an unknown dtype
    assert not supports("BACKWARD_BAND_EXPLICIT", C128, 3 * 4096, 4096, 3 * 256)
    assert not supports("BACKWARD_BAND_EXPLICIT", 2, *sizes(0, 0, 1 << 10))
    # the facet count plays no part
    assert supports("BACKWARD_BAND_EXPLICIT", C128, *sizes(8, 10, 1 << 14), 65)


def test_backward_band_explicit_complex64_is_backward_band():
    for log_yN in range(5, 18):
        s = sizes(0, 0, 1 << log_yN)
        assert supports("BACKWARD_BAND_EXPLICIT", C64, *s) == supports("BACKWARD_BAND", C64, *s), log_yN
    assert supports("BACKWARD_BAND_EXPLICIT", C64, *sizes(0, 0, 1 << 16)) and not supports("BACKWARD_BAND_EXPLICIT", C64, *sizes(0, 0, 1 << 17))
    for k in range(5, 17):
        s = sizes(5, 5, 3 << k)
        assert supports("BACKWARD_BAND_EXPLICIT", C64, *s) == supports("BACKWARD_BAND", C64, *s), k
    assert supports("BACKWARD_BAND_EXPLICIT", C64, *sizes(5, 5, 3 << 10))


def _pairs(feature, dtype, log_ms, log_xMs, yN=1 << 12):
    return {(lm, lx) for lm in log_ms for lx in log_xMs if lm <= lx and supports(feature, dtype, *sizes(lm, lx, yN))}


def test_split_prepare_pairs():
    # complex64: the pairs grid of test_capabilities_cpu.py, and every pair of the complex128 sweep range
    for pair in ((6, 8), (7, 8), (9, 11), (9, 12), (10, 12), (11, 12)):
        s = sizes(*pair, 1 << 12)
        assert supports("SPLIT_PREPARE", C64, *s) == supports("FUSED_SUBGRID", C64, *s), pair
    grid = (range(5, 12), range(7, 13))
    assert _pairs("SPLIT_PREPARE", C64, *grid) == _pairs("FUSED_SUBGRID", C64, *grid)
    got = _pairs("SPLIT_PREPARE", C128, *grid)
    # SPLIT_PAIRS_C128 of csrc/swiftly_caps.h
    assert got == {(7, 8), (7, 10), (8, 9), (8, 10), (9, 10)}
    assert {(7, 8), (8, 10)} <= got  # (8, 10): both W = 13.56 1k families
    assert got <= _pairs("BAND_PIPELINE_EXPLICIT", C128, *grid)
    assert all(lm <= 9 for lm, _ in got)  # the axis-0 remainder is one complex128 column pass: m <= 512
    assert not supports("SPLIT_PREPARE", C128, *sizes(9, 11, 1 << 12)) and "complex128" in _lib().last_error()
    # the answer does not depend on yN
    assert supports("SPLIT_PREPARE", C128, *sizes(8, 10, 3 << 12)) and supports("SPLIT_PREPARE", C128, *sizes(8, 10, 1 << 17))
    for dtype in (C64, C128):
        for n_facets, want in ((0, True), (1, True), (64, True), (65, False)):
            assert supports("SPLIT_PREPARE", dtype, *sizes(8, 10, 1 << 12), n_facets) == want, (dtype, n_facets)
        assert "64" in _lib().last_error() and "65" in _lib().last_error()
    assert not supports("SPLIT_PREPARE", 2, *sizes(7, 8, 1 << 12))
    assert not supports("SPLIT_PREPARE", C128, 3 * 4096, 4096, 3 * 256)


def test_unknown_feature_and_invalid_sizes_still_answer_no():
    lib = _lib()
    assert not lib.load().swiftly_hip_supports(99, C64, *sizes(7, 8, 1 << 12), 0)
    assert not lib.load().swiftly_hip_supports(8, C128, *sizes(7, 8, 1 << 12), 0)
    assert (lib.FEATURE_BACKWARD_BAND_EXPLICIT, lib.FEATURE_SPLIT_PREPARE) == (6, 7)
    for feature in ("BACKWARD_BAND_EXPLICIT", "SPLIT_PREPARE"):
        assert not supports(feature, C128, 1050, 512, 256) and "not divisible" in lib.last_error()


def test_python_wrappers_return_the_library_answers():
    import torch

    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    def core(N, yN, xM):
        c = object.__new__(SwiftlyCoreHip)
        c.N, c.yN_size, c.xM_size, c.xM_yN_size = N, yN, xM, xM * yN // N
        return c

    c = core(65536, 16384, 1024)  # 64k[1]-n16k-1k: m = 256
    assert c.supports_backward_band() and c.supports_backward_band(torch.complex64, explicit=True)
    assert not c.supports_backward_band(torch.complex128) and c.supports_backward_band(torch.complex128, explicit=True)
    assert not c.supports_backward_band(torch.float64, explicit=True)
    assert c.supports_split_prepare() and c.supports_split_prepare(torch.complex64, 64)
    assert c.supports_split_prepare(torch.complex128) and c.supports_split_prepare(torch.complex128, n_facets=64)
    assert not c.supports_split_prepare(torch.complex128, n_facets=65) and not c.supports_split_prepare(torch.float32)
    assert not c.supports_fused_subgrid(torch.complex128)
    c = core(131072, 65536, 1024)  # yN = 65536: complex64 only
    assert c.supports_backward_band(torch.complex64, explicit=True) and not c.supports_backward_band(torch.complex128, explicit=True)
    c = core(3 * 4096, 3 * 1024, 1024)  # yN = 3 * 2^10
    assert c.supports_backward_band(torch.complex64) and not c.supports_backward_band(torch.complex128, explicit=True)
    c = core(16384, 4096, 2048)  # (m, xM) = (512, 2048): a complex64 pair only
    assert c.supports_split_prepare(torch.complex64) and not c.supports_split_prepare(torch.complex128)
    assert c.supports_backward_band(torch.complex128, explicit=True)  # the band schedule does not need the split kernel
