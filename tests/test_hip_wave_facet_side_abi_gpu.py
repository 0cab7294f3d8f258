"""
``swiftly_hip_wave_facet_side`` through raw ctypes.  The streaming classes call K2 and ``transform_contributions_pieces``
separately; the one-call form stays in the ABI for native callers and promises the same launch sequence,
so its workspace and its blocks must equal those of the two separate calls bit for bit -- with ``compute_q`` on and off,
in both output forms, in complex64 and complex128 -- and bad row counts / strides are refused before anything is launched.
"""
import ctypes

import pytest

from test_hip_c128_band_pipeline_gpu import SMALL, _crandn
from test_hip_k2_slabs_gpu import M, bands_of_plan, problem, xA

pytestmark = pytest.mark.gpu

cvp = ctypes.c_void_p


def facet_side(core, bands, off0s, band, off1, rowmap, n_rows, q_work, q_facet_stride, compute_q, sub_off0s, g_out,
               g_layout=None):
    """return code of swiftly_hip_wave_facet_side; ``bands`` may be None (NULL) when ``compute_q`` is off"""
    F = len(off0s)
    scr = core.scratch("k2", core._k2_scratch_bytes(F, q_work.element_size()))
    if g_layout is None:
        fs, ss, offs, fstr = g_out.stride(0), g_out.stride(1), None, None
    else:
        fs, ss, offs, fstr = 0, 0, core._i64(g_layout[0]), core._i64(g_layout[1])
    return core._lib.swiftly_hip_wave_facet_side(
        core._handle, core._code(q_work), cvp(bands.data_ptr()) if bands is not None else None,
        int(bands.shape[1]) if bands is not None else 0, bands.stride(1) if bands is not None else 0,
        bands.stride(0) if bands is not None else 0, F, core._i64(off0s), int(band[0]), int(band[1]), int(off1),
        cvp(rowmap.data_ptr()), int(n_rows), cvp(q_work.data_ptr()), int(q_facet_stride), int(compute_q), len(sub_off0s),
        core._i64(sub_off0s), cvp(g_out.data_ptr()), fs, ss, offs, fstr, cvp(scr.data_ptr()), scr.numel(), core._stream(),
    )


def nan_workspace(torch, core, F, n_rows, m, dtype):
    """(NaN-filled workspace with 3 rows of slack behind every facet, its facet stride, the view ``Q[F, n_rows, m]``)"""
    stride = (n_rows + 3) * m
    work = torch.full((F, stride), float("nan"), dtype=dtype, device=core.device)
    return work, stride, work[:, : n_rows * m].view(F, n_rows, m)


def test_one_call_equals_k2_then_k3_from_one_piece_c64():
    from ska_sdp_exec_swiftly_amd import _lib

    torch = problem()[0]
    core, bands, band, off0s = bands_of_plan()
    off1, sub_off0s = 3 * xA, [0, 2 * xA, 69 * xA]  # wave i1 = 3 of the plan
    rowmap, n_rows = core.subgrid_column_rows(sub_off0s)
    F, S = len(off0s), len(sub_off0s)
    Q = core.prepare_facet_columns(bands, off0s, band, off1, rowmap, n_rows)
    want = torch.empty((F, S, M, M), dtype=torch.complex64, device=core.device)
    core.transform_contributions_pieces([(Q, rowmap, n_rows, 0, M)], off0s, sub_off0s, want)

    work, stride, q_view = nan_workspace(torch, core, F, n_rows, M, torch.complex64)
    got = torch.full_like(want, float("nan"))
    _lib.check(facet_side(core, bands, off0s, band, off1, rowmap, n_rows, work, stride, 1, sub_off0s, got))
    assert torch.equal(q_view, Q)
    assert torch.isnan(work[:, n_rows * M:].real).all()  # the slack behind every facet is not written
    assert torch.equal(got, want)
    # compute_q = 0 without band buffers: K3 + K4a from the workspace as it stands
    again = torch.full_like(want, float("nan"))
    _lib.check(facet_side(core, None, off0s, band, off1, rowmap, n_rows, work, stride, 0, sub_off0s, again))
    assert torch.equal(q_view, Q) and torch.equal(again, want)

    # the flat-buffer form: subgrid-major, block (f, b) at 64 + (b*F + f) * m*m, behind a guard that must stay zero
    layout = ([64 + b * F * M * M for b in range(S)], [M * M] * S)
    for compute_q, src in ((1, bands), (0, None)):
        if compute_q:
            work.fill_(float("nan"))
        flat = torch.zeros(F * S * M * M + 64, dtype=torch.complex64, device=core.device)
        _lib.check(facet_side(core, src, off0s, band, off1, rowmap, n_rows, work, stride, compute_q, sub_off0s, flat,
                              g_layout=layout))
        assert torch.equal(q_view, Q), compute_q
        assert torch.equal(flat[64:].view(S, F, M, M).transpose(0, 1), want) and not flat[:64].any(), compute_q


def test_one_call_equals_k2_then_k3_from_one_piece_c128():
    import numpy
    import torch

    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip, _lib

    p = SMALL
    core = SwiftlyCoreHip(p["W"], p["N"], p["xM_size"], p["yN_size"])
    m, yN = core.xM_yN_size, core.yN_size
    F, off1, sub_off0s = 2, -5 * p["xA_size"], [0, 3 * p["xA_size"]]
    bands = torch.from_numpy(_crandn(numpy.random.default_rng(32), (F, 96, yN))).cuda()
    off0s = [0, -3 * core.facet_off_step * 8]
    rowmap, n_rows = core.subgrid_column_rows(sub_off0s)
    Q = core.prepare_facet_columns(bands, off0s, (0, yN), off1, rowmap, n_rows)
    want = torch.empty((F, len(sub_off0s), m, m), dtype=torch.complex128, device=core.device)
    core.transform_contributions_pieces([(Q, rowmap, n_rows, 0, m)], off0s, sub_off0s, want)

    work, stride, q_view = nan_workspace(torch, core, F, n_rows, m, torch.complex128)
    got = torch.full_like(want, float("nan"))
    _lib.check(facet_side(core, bands, off0s, (0, yN), off1, rowmap, n_rows, work, stride, 1, sub_off0s, got))
    assert torch.equal(q_view, Q) and torch.equal(got, want)


@pytest.mark.parametrize("case", ["no rows", "short facet stride"])
def test_bad_workspace_is_refused_before_any_launch(case):
    from ska_sdp_exec_swiftly_amd import _lib

    torch = problem()[0]
    core, bands, band, off0s = bands_of_plan()
    off1, sub_off0s = 3 * xA, [0, 2 * xA, 69 * xA]
    rowmap, n_rows = core.subgrid_column_rows(sub_off0s)
    F, S = len(off0s), len(sub_off0s)
    work, stride, _ = nan_workspace(torch, core, F, n_rows, M, torch.complex64)
    g_out = torch.full((F, S, M, M), float("nan"), dtype=torch.complex64, device=core.device)
    rows, q_stride = (0, stride) if case == "no rows" else (n_rows, n_rows * M - 1)
    assert facet_side(core, bands, off0s, band, off1, rowmap, rows, work, q_stride, 1, sub_off0s, g_out) == _lib.ERR_PARAM
    torch.cuda.synchronize()
    assert torch.isnan(work.real).all() and torch.isnan(g_out.real).all()  # nothing ran
