"""
The one route of ``choose_row_route`` (csrc/swiftly_rowroute.h) no other GPU test reaches, at the smallest shape that takes
it, against the 1-D oracle ("The row route": every other kind has a test there).

``Split32k``: a complex64 transform of 32768 points along the contiguous axis with an identity store whose load map is
not the one of a ``prepare_*`` primitive -- the contribution map of ``extract_from_subgrid`` at m = 32768 (xM = 65536).
Bound: the facet sweep's for float32 arithmetic (tests/test_hip_facet_sweep_gpu.py), relative RMSE over the whole output
below ``2e-6 * sqrt(min(L, 15) / 15)`` with L = 15.
"""
import numpy
import pytest

from oracle import swiftly_oracle as orc

pytestmark = pytest.mark.gpu


def test_split_32k_extract_from_subgrid():
    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    W, N, xM, yN = 10.875, 65536, 65536, 32768
    core = SwiftlyCoreHip(W, N, xM, yN)
    ref = orc.OracleCore(W, N, xM, yN)
    assert core.xM_yN_size == 32768
    rng = numpy.random.default_rng(27)
    rows = (rng.standard_normal((3, xM)) + 1j * rng.standard_normal((3, xM))).astype(numpy.complex64)
    for off in (0, 7, -12345):  # aligned, rotated either way
        got = core.extract_from_subgrid(rows, off, axis=1)
        want = ref.extract_from_subgrid(rows.astype(complex), off, 1)
        rel = numpy.sqrt(numpy.mean(numpy.abs(got - want) ** 2) / numpy.mean(numpy.abs(want) ** 2))
        print(f"extract_from_subgrid, m = 32768, off {off}: relative RMSE {rel:.3e}")
        assert got.dtype == numpy.complex64 and got.shape == (3, 32768) and rel < 2e-6, rel
