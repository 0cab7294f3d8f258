"""
Boundaries of the native capability table (``swiftly_hip_supports`` / ``swiftly_hip_limit``, csrc/swiftly_caps.h) against
literal expectations, without a GPU: for every pipeline-level feature the first and last supported value and the first
unsupported one on each side.  The expectations are written out here; they are what the ``supports_*`` gates of
``SwiftlyCoreHip`` answered when they still held these rules themselves.
"""


def _lib():
    from ska_sdp_exec_swiftly_amd import _lib as lib

    return lib


def supports(feature, dtype, N, yN, xM, n_facets=0):
    lib = _lib()
    return bool(lib.load().swiftly_hip_supports(getattr(lib, "FEATURE_" + feature), dtype, N, yN, xM, n_facets))


def sizes(log_m, log_xM, yN):
    """(N, yN, xM) with ``m = 2^log_m`` and ``xM = 2^log_xM``"""
    xM = 1 << log_xM
    assert (xM * yN) % (1 << log_m) == 0
    return (xM * yN) >> log_m, yN, xM


C64, C128 = 0, 1


def test_band_pipeline_complex64_boundaries():
    # (m <= yN and the smallest instance has m = 128: a power-of-two yN of 64 passes the length gate and still has no pair)
    for log_yN, want in ((5, False), (6, False), (7, True), (16, True), (17, False)):
        assert supports("BAND_PIPELINE", C64, *sizes(min(7, log_yN), 8, 1 << log_yN)) == want, log_yN
    assert supports("BAND_PIPELINE", C64, *sizes(7, 10, 1 << 16)) and not supports("BAND_PIPELINE", C64, *sizes(7, 10, 1 << 17))
    # yN = 3 * 2^k: a valid N needs 2^k >= m
    for k, want in ((5, False), (6, False), (7, True), (15, True), (16, False)):
        assert supports("BAND_PIPELINE", C64, *sizes(min(7, k), 8, 3 << k)) == want, k
    for Q, want in ((3, True), (5, True), (7, True), (9, True), (11, False), (15, False)):
        assert supports("BAND_PIPELINE", C64, *sizes(7, 8, Q << 10)) == want, Q
    # the answer does not depend on `explicit` in complex64
    for log_yN in (5, 7, 16, 17):
        s = sizes(min(7, log_yN), 8, 1 << log_yN)
        assert supports("BAND_PIPELINE", C64, *s) == supports("BAND_PIPELINE_EXPLICIT", C64, *s)
    # (m, xM): m = 64 has no instance, (1024, 4096) is the last one, (2048, 4096) and (512, 4096) have none
    for pair, want in (((6, 8), False), ((7, 8), True), ((9, 11), True), ((9, 12), False), ((10, 12), True), ((11, 12), False)):
        assert supports("BAND_PIPELINE", C64, *sizes(*pair, 1 << 12)) == want, pair
        assert supports("FUSED_SUBGRID", C64, *sizes(*pair, 1 << 12)) == want, pair
    # xM not a power of two; an unknown dtype
    assert not supports("FUSED_SUBGRID", C64, 3 * 4096, 4096, 3 * 256)
    assert not supports("FUSED_SUBGRID", 2, *sizes(7, 8, 1 << 12)) and not supports("FUSED_SUBGRID", -1, *sizes(7, 8, 1 << 12))


def test_facet_limit():
    lib = _lib()
    assert lib.load().swiftly_hip_limit(lib.LIMIT_FUSED_FACETS) == 64
    s = sizes(8, 10, 1 << 12)
    for feature, dtype in (("FUSED_SUBGRID", C64), ("BAND_PIPELINE", C64), ("BAND_PIPELINE_EXPLICIT", C64),
                           ("BAND_PIPELINE_EXPLICIT", C128)):
        for n_facets, want in ((0, True), (1, True), (64, True), (65, False)):
            assert supports(feature, dtype, *s, n_facets) == want, (feature, dtype, n_facets)
    assert "64" in lib.last_error() and "65" in lib.last_error()
    # features without a facet sum ignore the count
    assert supports("BACKWARD_BAND", C64, *s, 65) and supports("SPLIT_BAND", C64, *sizes(8, 10, 1 << 14), 65)


def test_band_pipeline_complex128_only_when_explicit():
    for log_yN, want in ((6, False), (7, True), (15, True), (16, False)):
        s = sizes(min(7, log_yN), 8, 1 << log_yN)
        assert supports("BAND_PIPELINE_EXPLICIT", C128, *s) == want, log_yN
        assert not supports("BAND_PIPELINE", C128, *s)
        assert "complex128" in _lib().last_error()
    assert not supports("FUSED_SUBGRID", C128, *sizes(7, 8, 1 << 10))
    # no radix-Q pass in complex128; m = 1024 and (512, 2048) are complex64 instances only
    assert not supports("BAND_PIPELINE_EXPLICIT", C128, *sizes(7, 8, 3 << 10))
    for pair, want in (((6, 8), False), ((7, 8), True), ((9, 10), True), ((9, 11), False), ((10, 11), False)):
        assert supports("BAND_PIPELINE_EXPLICIT", C128, *sizes(*pair, 1 << 12)) == want, pair


def test_backward_band_boundaries():
    # 64 .. 65536: the lengths accumulate_facet_columns AND finish_facet_band run (twiddle tables exist for 2^3 .. 2^16, the
    # finishing row kernels end at 65536) and tests/test_hip_facet_sweep_gpu.py sweeps; the gate used to answer yes for
    # 4 .. 262144, where the entry points refused
    for log_yN, want in ((5, False), (6, True), (16, True), (17, False)):
        assert supports("BACKWARD_BAND", C64, *sizes(0, 0, 1 << log_yN)) == want, log_yN
        assert not supports("BACKWARD_BAND", C128, *sizes(0, 0, 1 << log_yN))
    for k, want in ((5, False), (6, True), (15, True), (16, False)):
        assert supports("BACKWARD_BAND", C64, *sizes(5, 5, 3 << k)) == want, k
    assert not supports("BACKWARD_BAND", C64, *sizes(5, 5, 11 << 10))
    # xM (and with it m) not a power of two
    assert not supports("BACKWARD_BAND", C64, 3 * 4096, 4096, 3 * 256) and not supports("BACKWARD_BAND", C64, 3 * 4096, 3 * 1024, 3 * 256)


def test_split_band_layout_boundaries():
    for log_yN, want in ((13, False), (14, True), (16, True), (17, False)):
        assert supports("SPLIT_BAND", C64, *sizes(7, 8, 1 << log_yN)) == want, log_yN
    assert not supports("SPLIT_BAND", C64, *sizes(7, 8, 3 << 13))


def test_window_rows_sizes_and_limits():
    lib = _lib()
    for log_m, log_xM, log_yN, want in ((9, 10, 15, True), (9, 11, 15, True), (9, 12, 15, False), (9, 10, 14, False),
                                        (9, 10, 16, False), (8, 10, 15, False), (10, 11, 15, False)):
        assert supports("WINDOW_ROWS", C64, *sizes(log_m, log_xM, 1 << log_yN)) == want, (log_m, log_xM, log_yN)
    assert lib.load().swiftly_hip_limit(lib.LIMIT_WINDOW_ROWS_WINDOWS) == 256
    # follows row_pass_whole_stage_columns() for the current LDS geometry: RGeoWhole has 139264 bytes of LDS, the 512-point
    # exchange rows take 36864, the rest holds 8-byte columns, rounded down to a multiple of 32
    assert (139264 - 36864) // 8 // 32 * 32 == 12800
    assert lib.load().swiftly_hip_limit(lib.LIMIT_WINDOW_ROWS_STAGE_COLUMNS) == 12800
    assert lib.load().swiftly_hip_limit(99) == -1


def test_invalid_sizes_and_features_answer_no_with_the_reason():
    lib = _lib()
    for feature in ("FUSED_SUBGRID", "BAND_PIPELINE", "BACKWARD_BAND", "SPLIT_BAND", "WINDOW_ROWS"):
        assert not supports(feature, C64, 1050, 512, 256)
        assert "not divisible" in lib.last_error()
        assert not supports(feature, C64, 1024, 512, 0)
    assert not supports("FUSED_SUBGRID", C64, 1024, 96, 256) and "not divisible" in lib.last_error()
    assert not supports("FUSED_SUBGRID", C64, 4096, 64, 32) and "Contribution size" in lib.last_error()
    assert not lib.load().swiftly_hip_supports(99, C64, *sizes(7, 8, 1 << 12), 0)


def test_python_gates_are_the_library_answers():
    """the wrappers of ``SwiftlyCoreHip`` (no handle needed: the table is asked by size): defaults, dtype mapping, limits"""
    import torch

    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    def core(N, yN, xM):
        c = object.__new__(SwiftlyCoreHip)
        c.N, c.yN_size, c.xM_size, c.xM_yN_size = N, yN, xM, xM * yN // N
        return c

    c = core(65536, 32768, 1024)  # the benchmarked configuration
    assert c.MAX_FUSED_FACETS == 64 and c.WINDOW_ROWS_STAGE_COLUMNS == 12800
    assert c.supports_fused_subgrid() and c.supports_fused_subgrid(torch.complex64, 64)
    assert not c.supports_fused_subgrid(torch.complex64, 65) and not c.supports_fused_subgrid(torch.complex128)
    assert c.supports_band_pipeline() and c.supports_band_pipeline(torch.complex64, 9, explicit=True)
    assert not c.supports_band_pipeline(torch.complex128) and c.supports_band_pipeline(torch.complex128, explicit=True)
    assert not c.supports_band_pipeline(torch.complex128, 65, explicit=True)
    assert not c.supports_band_pipeline(torch.float32) and not c.supports_backward_band(torch.float64)
    assert c.supports_backward_band() and not c.supports_backward_band(torch.complex128)
    assert c.band_for_offsets([0]) != (0, 32768)
    c = core(4096, 2048, 1024)
    assert c.band_for_offsets([0, 512]) == (0, 2048)
    c = core(3 * 4096, 3 * 1024, 1024)  # m = 256, yN = 3 * 2^10
    assert c.supports_band_pipeline(torch.complex64) and c.supports_backward_band(torch.complex64)
    assert not c.supports_band_pipeline(torch.complex128, explicit=True) and c.band_for_offsets([0]) == (0, 3 * 1024)
