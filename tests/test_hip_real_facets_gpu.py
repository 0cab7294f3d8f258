"""
Real-valued (float32) facets through the forward K1 and ``SwiftlyForward`` (``swiftly_hip_prepare_facet_band_real``, the
REAL instances of the row kernels) on the GPU.

Two checks per case.  (a) ``torch.equal`` with the PROMOTED path -- the same facet as complex64 through the complex entry
point: the real instances keep the element-to-lane map, the tables and the butterflies of the complex ones and every
operation on a zero imaginary part is exact, so the values are the same (at most the sign of a zero differs, which
``torch.equal`` ignores).  (b) relative RMS against ``oracle.prepare_facet`` below 2e-6, the bound of
``test_hip_band_pipeline_gpu.py::test_prepare_facet_band`` (one float32 transform of un-amplified data).

Only the columns inside the band are compared: the padding columns of a band buffer are never written.

The promoted tensor is always ``real.to(complex64)``, the contiguous copy a real facet used to become, whatever the pitch
and the base of the real rows: the real launcher picks the geometry, the segment count and the rotation that the complex
one picks for that copy, and pitch and alignment only decide how a lane fetches its two adjacent reals.
"""
import ctypes

import numpy
import pytest

from oracle import swiftly_oracle as orc
from test_hip_band_pipeline_gpu import W64, N64, xM64, yN64, yB64, _small_rows_problem, band_cols, core64, relrms

pytestmark = pytest.mark.gpu

BOUND = 2e-6
OFFSETS_64K = ((0, False), (64 * 352, True), (-64 * 352, False), (-64 * 320, True), (64 * 351, False), (64 * 352 + 2, True),
               (4097, False))
_shared = {}


def _real_rows(seed, rows, size):
    return numpy.random.default_rng(seed).standard_normal((rows, size)).astype(numpy.float32)


def _case64(key, seed, rows, size, offsets):
    """float32 rows, their device tensor and the oracle's prepare_facet per offset: computed once, shared, never changed"""
    import torch

    if key not in _shared:
        ref = core64()[1]
        x = _real_rows(seed, rows, size)
        want = {off: ref.prepare_facet(x.astype(complex), off, 1) for off in offsets}
        _shared[key] = (x, torch.from_numpy(x).cuda(), want)
    return _shared[key]


def _check(core, real, promoted, off, band, want, fold_window=None, **kw):
    """K1 of the float32 tensor against K1 of the promoted one (equal) and against the oracle's rows ``want``"""
    import torch

    assert real.dtype == torch.float32 and promoted.dtype == torch.complex64
    fold = fold_window is not None
    got = core.prepare_facet_band(real, off, band, fold_other_axis_window=fold or "rows_of" in kw, **kw)
    base = core.prepare_facet_band(promoted, off, band, fold_other_axis_window=fold or "rows_of" in kw, **kw)
    assert got.dtype == torch.complex64 and got.shape == (real.shape[0], core.band_columns(band))
    # physical column of every logical one: parity-split from 16384 points on, else the plain layout (whole axis)
    pc = band_cols(core.yN_size, band) if core.yN_size >= 16384 else numpy.arange(core.yN_size)
    keep = pc >= 0
    idx = torch.from_numpy(pc[keep]).cuda()
    assert torch.equal(got[:, idx], base[:, idx]), (off, band)
    if fold_window is not None:
        want = want * fold_window[:, None]
    rel = relrms(got.cpu().numpy()[:, pc[keep]], want[:, keep])
    print(f"yN={core.yN_size} off={off} band={band} relative RMS vs oracle {rel:.3e}")
    assert rel < BOUND, (off, band, rel)


@pytest.mark.parametrize("band", [(0, yN64), (10736, 11472), (32001, 2049)])
def test_real_k1_32768(band):
    """22528 reals in 32768-point rows: the tuned pair instances with 22 and 24 data segments at three rotations, and an
    odd offset, which takes the 512 x 32 geometry without pair loads in both forms"""
    core, ref = core64()
    assert core.supports_real_facets()
    rows = 7
    x, xt, want = _case64("22528", 31, rows, yB64, [o for o, _ in OFFSETS_64K])
    import torch

    xc = xt.to(torch.complex64)
    for off, fold in OFFSETS_64K:
        _check(core, xt, xc, off, band, want[off], ref.facet_window(rows) if fold else None)


def test_real_k1_32768_16_segment_facets():
    """16384 reals: exactly 16 data segments at aligned offsets (the instance whose window table has no (r, r + 16) pairs),
    17 at an unaligned one (the 22-segment instance with empty tail segments)"""
    import torch

    core, _ = core64()
    offsets = (0, 16384, 16384 + 2 * 333)
    x, xt, want = _case64("16384", 33, 7, 16384, offsets)
    xc = xt.to(torch.complex64)
    for off in offsets:
        _check(core, xt, xc, off, (10736, 11472), want[off])


def test_real_k1_32768_all_segments():
    """26624 reals: 26 or 27 data segments, more than the tuned instances skip.  The all-segment real instances differ from
    the complex one in the last bit (``core._real_rows_match_promoted``), so ``prepare_facet_band`` promotes such a facet:
    the values of the promoted path, also for a view at a 4-byte-aligned base with an odd pitch"""
    import torch

    core, _ = core64()
    size, offsets = 26624, (0, 2 * 333)
    assert not core._real_rows_match_promoted(size) and core._real_rows_match_promoted(yB64)
    x, xt, want = _case64("26624", 41, 3, size, offsets)
    big = torch.zeros((3, size + 3), dtype=torch.float32, device="cuda")
    big[:, 1 : 1 + size] = xt
    for off in offsets:
        _check(core, xt, xt.to(torch.complex64), off, (10736, 11472), want[off])
        _check(core, big[:, 1 : 1 + size], xt.to(torch.complex64), off, (10736, 11472), want[off])


def test_real_k1_32768_all_segment_instances_through_the_abi():
    """The all-segment pair instances themselves (``swiftly_hip_prepare_facet_band_real`` called directly, which the Python
    layer avoids for such facets): 8-byte loads on contiguous rows, 4-byte loads on a view with an odd pitch at a
    4-byte-aligned base.  Within the oracle bound; equality with the complex form is NOT claimed here"""
    import torch

    from ska_sdp_exec_swiftly_amd import _lib

    core, _ = core64()
    size, offsets, band = 26624, (0, 2 * 333), (10736, 11472)
    x, xt, want = _case64("26624", 41, 3, size, offsets)
    big = torch.zeros((3, size + 3), dtype=torch.float32, device="cuda")
    big[:, 1 : 1 + size] = xt
    pc = band_cols(yN64, band)
    keep = pc >= 0
    lib = _lib.load()
    for src in (xt, big[:, 1 : 1 + size]):
        for off in offsets:
            out = torch.zeros((3, core.band_columns(band)), dtype=torch.complex64, device="cuda")
            rc = lib.swiftly_hip_prepare_facet_band_real(  # pylint: disable=protected-access
                core._handle, _lib.C64, ctypes.c_void_p(src.data_ptr()), 3, size, src.stride(0),
                ctypes.c_void_p(out.data_ptr()), out.stride(0), off, band[0], band[1], 0, None)
            assert rc == 0, _lib.last_error()
            torch.cuda.synchronize()
            rel = relrms(out.cpu().numpy()[:, pc[keep]], want[off][:, keep])
            print(f"all-segment instance, pitch {src.stride(0)} off={off} relative RMS vs oracle {rel:.3e}")
            assert rel < BOUND, (src.stride(0), off, rel)


def test_real_k1_alignment():
    """Rows the 8-byte loads cannot take must run (no fault, no refusal) and give the values of the promoted facet: an odd
    pitch with a base that is only 4-byte aligned, an even pitch with such a base (pair geometry, two 4-byte loads per lane
    and segment), and even pitches larger than the facet at an 8-byte-aligned base (the 8-byte loads)."""
    import torch

    core, _ = core64()
    rows = 7
    x, _, want = _case64("22528", 31, rows, yB64, [o for o, _ in OFFSETS_64K])
    band = (10736, 11472)
    for width, first in ((yB64 + 3, 1), (yB64 + 3, 2), (yB64 + 64, 1), (yB64 + 64, 0), (yB64 + 64, 2)):
        big = torch.zeros((rows, width), dtype=torch.float32, device="cuda")
        big[:, first : first + yB64] = torch.from_numpy(x).cuda()
        view = big[:, first : first + yB64]
        assert view.stride(0) == width and view.data_ptr() % 8 == (4 if first % 2 else 0)
        promoted = view.to(torch.complex64)
        assert promoted.is_contiguous()
        for off in (0, 64 * 352, 64 * 351, 64 * 352 + 2, 4097):
            _check(core, view, promoted, off, band, want[off])


def test_real_k1_without_window_table():
    """A core whose window-table cache is full (64 tables, none is ever evicted) runs the same instances with the plain
    window loads, for real rows as for complex ones: equal to each other and to what a core with the table gives"""
    import torch

    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    shared, _ = core64()
    core = SwiftlyCoreHip(W64, N64, xM64, yN64)
    band = (10736, 11472)
    xt = torch.from_numpy(_real_rows(39, 2, yB64)).cuda()
    xc = xt.to(torch.complex64)
    for k in range(1, 81):  # every even shift is a table of its own
        core.prepare_facet_band(xt, 2 * k, band)
    pc = band_cols(yN64, band)
    idx = torch.from_numpy(pc[pc >= 0]).cuda()
    for off in (0, 64 * 352, 64 * 351):
        got = core.prepare_facet_band(xt, off, band)[:, idx]
        assert torch.equal(got, core.prepare_facet_band(xc, off, band)[:, idx]), off
        assert torch.equal(got, shared.prepare_facet_band(xt, off, band)[:, idx]), off


@pytest.mark.parametrize("N,yN,size", [(32768, 16384, 11264), (131072, 65536, 45056)])
def test_real_k1_16384_and_65536(N, yN, size):
    """The general real instances of the 16384- and 65536-point geometries and the 44-segment form of the latter (aligned
    offsets: 44 of its 64 segments hold data; 128 * 351 shifts the facet off the segment grid: 45, the general instance)"""
    import torch

    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    core, ref = SwiftlyCoreHip(W64, N, xM64, yN), orc.OracleCore(W64, N, xM64, yN)
    assert core.supports_real_facets()
    rows = 3
    x = _real_rows(35, rows, size)
    xt = torch.from_numpy(x).cuda()
    xc = xt.to(torch.complex64)
    step = core.facet_off_step
    band = (10736 * yN // yN64, 11472 * yN // yN64)
    for off in (0, step * 352, step * 351):
        _check(core, xt, xc, off, band, ref.prepare_facet(x.astype(complex), off, 1))


@pytest.mark.parametrize("N,yN,size", [(1024, 512, 352), (8192, 4096, 2816), (16384, 8192, 5632)])
def test_real_k1_plain_layout(N, yN, size):
    """Plain band layout (whole padded axis): the generic row kernel's real load (512 and 4096 points: radix 8 and 16) and
    the lean 8192-point row kernel's"""
    import torch

    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    W, xM, rows = 11.0, 256, 5
    core, ref = SwiftlyCoreHip(W, N, xM, yN), orc.OracleCore(W, N, xM, yN)
    assert core.supports_real_facets() and core.band_columns((0, yN)) == yN
    x = _real_rows(37, rows, size)
    xt = torch.from_numpy(x).cuda()
    xc = xt.to(torch.complex64)
    for off, fold in ((0, False), (core.facet_off_step * 11, True)):
        _check(core, xt, xc, off, (0, yN), ref.prepare_facet(x.astype(complex), off, 1), ref.facet_window(rows) if fold else None)
    with pytest.raises(NotImplementedError):  # the plain layout keeps the whole axis, for real rows as for complex ones
        core.prepare_facet_band(xt, 0, (1, yN - 1))


def test_real_k1_rows_of():
    """rows [100, 107) of a facet with 352 rows: the folded axis-0 window is that facet's"""
    import torch

    core, ref = core64()
    x, xt, want = _case64("22528", 31, 7, yB64, [o for o, _ in OFFSETS_64K])
    xc = xt.to(torch.complex64)
    for off in (0, 64 * 352):
        _check(core, xt, xc, off, (10736, 11472), want[off] * ref.facet_window(352)[100:107, None], rows_of=(352, 100))


def test_real_k1_refusals():
    import torch

    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip, _lib

    core, _ = core64()
    band = (0, yN64)
    for bad in (torch.int32, torch.float16, torch.float64):
        with pytest.raises(ValueError):
            core.prepare_facet_band(torch.zeros((2, yB64), dtype=bad, device="cuda"), 0, band)
    # a complex64 output buffer is what a float32 facet needs
    xt = torch.zeros((2, yB64), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        core.prepare_facet_band(xt, 0, band, out=torch.empty((2, core.band_columns(band)), dtype=torch.complex128, device="cuda"))
    # the raw entry point: complex128 output is refused through the capability rule, nothing is launched
    out = torch.zeros((2, core.band_columns(band)), dtype=torch.complex128, device="cuda")
    lib = _lib.load()
    args = (ctypes.c_void_p(xt.data_ptr()), 2, yB64, xt.stride(0), ctypes.c_void_p(out.data_ptr()), out.stride(0), 0, 0, yN64)
    rc = lib.swiftly_hip_prepare_facet_band_real(core._handle, _lib.C128, *args, 0, None)  # pylint: disable=protected-access
    assert rc == _lib.ERR_UNSUPPORTED and "complex128" in _lib.last_error()
    rc = lib.swiftly_hip_prepare_facet_band_rows_real(core._handle, _lib.C128, *args, 0, 0, None)  # pylint: disable=protected-access
    assert rc == _lib.ERR_UNSUPPORTED and "complex128" in _lib.last_error()
    torch.cuda.synchronize()
    assert not out.any()
    # yN = 3 * 2^12: the radix-Q pass has no real load
    q = SwiftlyCoreHip(11.0, 24576, 256, 3 << 12)
    assert q.supports_band_pipeline(torch.complex64) and not q.supports_real_facets()
    with pytest.raises(NotImplementedError, match="radix-Q"):
        q.prepare_facet_band(torch.zeros((2, 8448), dtype=torch.float32, device="cuda"), 0, (0, 3 << 12))
    got = q.prepare_facet_band(torch.zeros((2, 8448), dtype=torch.complex64, device="cuda"), 0, (0, 3 << 12))
    assert got.dtype == torch.complex64


def _real_problem(seed):
    torch, sw, cfg, facet_cfgs, facets, sg_cfgs = _small_rows_problem(seed=seed)
    reals = [f.real.contiguous() for f in facets]
    ordered = sorted(sg_cfgs, key=lambda c: (c.off1, c.off0))
    return torch, sw, cfg, facet_cfgs, reals, sg_cfgs, ordered


def _run(sw, cfg, facet_cfgs, data, sg_cfgs, ordered, **kw):
    fwd = sw.SwiftlyForward(cfg, list(zip(facet_cfgs, data)), subgrid_configs=sg_cfgs, **kw)
    return fwd, fwd.get_subgrid_tasks(ordered)


def test_forward_keeps_float32_facets_real():
    """SwiftlyForward(wave_axis=1) on the small-rows problem of test_hip_band_pipeline_gpu.py with real facets: float32 device
    tensors and float32 host arrays stay float32 (resident and on the wire) and give the subgrids of the promoted facets"""
    torch, sw, cfg, facet_cfgs, reals, sg_cfgs, ordered = _real_problem(43)
    assert cfg.core.supports_real_facets()
    base_fwd, base = _run(sw, cfg, facet_cfgs, [r.to(torch.complex64) for r in reals], sg_cfgs, ordered, wave_axis=1)
    assert base_fwd.facet_dtype == torch.complex64 == base_fwd.dtype
    assert all(float(b.abs().max()) > 0 for b in base)
    for data in (reals, [r.cpu().numpy() for r in reals]):
        assert all(d.dtype in (torch.float32, numpy.float32) for d in data)
        fwd, got = _run(sw, cfg, facet_cfgs, data, sg_cfgs, ordered, wave_axis=1)
        assert fwd.facet_dtype == torch.float32 and fwd.dtype == torch.complex64
        ingested = [fwd._ingest.ready(j) for j in range(len(reals))]  # pylint: disable=protected-access
        assert all(t.dtype == torch.float32 and t.is_cuda and torch.equal(t, r) for t, r in zip(ingested, reals))
        assert len(got) == len(base) == 12
        for g, b in zip(got, base):
            assert g.dtype == torch.complex64 and torch.equal(g, b)
    # the default axis with a plan is the same pipeline
    fwd, got = _run(sw, cfg, facet_cfgs, reals, sg_cfgs, ordered)
    assert fwd.wave_axis == 1 and fwd.facet_dtype == torch.float32 and all(torch.equal(g, b) for g, b in zip(got, base))
    # a complex facet among them: everything is promoted as before
    mixed = [reals[0], reals[1].to(torch.complex64), reals[2]]
    for data in (mixed,):
        fwd, got = _run(sw, cfg, facet_cfgs, data, sg_cfgs, ordered, wave_axis=1)
        assert fwd.facet_dtype == torch.complex64 and all(torch.equal(g, b) for g, b in zip(got, base))
        assert fwd._ingest.ready(0).dtype == torch.complex64  # pylint: disable=protected-access


@pytest.mark.parametrize("how", ["axis1_first", "wave_axis0"])
def test_forward_promotes_float32_facets_where_k1_has_no_real_form(how):
    """The whole-row K1 of ``axis1_first=True`` (mode 2) and the column-pass K1 of ``wave_axis=0`` load complex rows: float32
    facets are promoted exactly as before and give the values of the promoted run"""
    torch, sw, cfg, facet_cfgs, reals, sg_cfgs, ordered = _real_problem(45)
    kw = dict(wave_axis=1)
    if how == "axis1_first":
        P = dict(W=W64, fov=1.0, N=N64, yB_size=352, yN_size=yN64, xA_size=928, xM_size=xM64)
        cfg = sw.SwiftlyConfig(backend="hip", axis1_first=True, **P)
    else:
        kw = dict(wave_axis=0)
        ordered = sorted(sg_cfgs, key=lambda c: (c.off0, c.off1))
    _, base = _run(sw, cfg, facet_cfgs, [r.to(torch.complex64) for r in reals], sg_cfgs, ordered, **kw)
    for data in (reals, [r.cpu().numpy() for r in reals]):
        fwd, got = _run(sw, cfg, facet_cfgs, data, sg_cfgs, ordered, **kw)
        assert fwd.facet_dtype == torch.complex64
        assert fwd._ingest.ready(0).dtype == torch.complex64  # pylint: disable=protected-access
        if how == "axis1_first":
            assert fwd._axis1() == 2  # pylint: disable=protected-access
        assert all(torch.equal(g, b) for g, b in zip(got, base))
