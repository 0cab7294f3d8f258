"""
Real-valued facets out of the backward band pass: ``finish_facet_band(..., real=True)`` / ``swiftly_hip_finish_facet_band_real``
and ``SwiftlyBackward(..., facet_dtype=torch.float32)``.

The real-store forms of the finishing row kernels compute the stored value as the complex forms do and write its real
part, so every check here is exact: the float32 output is ``torch.equal`` to the ``.real`` of what the complex entry point
gives on the same input.  On top of that the real output is compared with the 1-D oracle under the bounds of the facet
sweep (tests/test_hip_facet_sweep_gpu.py: relative RMSE below ``2e-6 * sqrt(min(L, 15) / 15)``, per-row peak at most 2e-5) --
the sweep's own bounds for the complex form, taken over the real parts.

(a) one case per instance, ``yN = 2^L`` for L = 6 .. 16 (the sweep's cores): the generic rows (64 .. 4096 points), the lean
    row kernel (8192, 16384; mapped load and identity load), the 32768-point kernels -- pair geometry with 13, 16 and all 32
    load segments and the geometry without pair loads -- and the 65536-point kernel.  Every output lies in a sentinel-filled
    float32 buffer at an odd pitch and a base that is 4-byte but not 8-byte aligned.
(b) odd facet sizes with odd facet offsets.
(c) refusals leave the output alone and name their reason.
(d) whole ``SwiftlyBackward`` passes in the plain (L = 9) and the split (L = 14) band layout.

Every case prints a ``REALOUT`` line with its figures.
"""
import numpy
import pytest

from test_hip_facet_sweep_gpu import _sizes, cores, crandn, f32_bound, facet_size, params, relrms, vector_peak

pytestmark = pytest.mark.gpu

SENTINEL = 7.5
ROWS = 24
LENGTHS = list(range(6, 17))


def band_segments(yN, band, seglen):
    """the run of load segments that can hold band data (data_segment_run of csrc/row_pass.hip for the load map of a band:
    ``ld_a = -band_start mod yN``, ``ld_len = band length``)"""
    start, length = band
    base = ((-start) % yN + yN // 2) % yN
    lows = [(seglen * r + base) % yN for r in range(yN // seglen)]
    return sum(lo < length or lo + seglen > yN for lo in lows)


def sweep_bands(L, yN, yB):
    """the three bands of test_finish_facet_band_lengths (interior, wrapping, full) with its facet offsets, and its fourth at
    L = 15"""
    cases = [((yN // 2 - 5 * yN // 32, 11 * yN // 32 + 8), 0), ((yN - 3 * yN // 32, 7 * yN // 32 + 1), yB), ((0, yN), -yB)]
    if L == 15:
        cases.append(((yN // 4 + 1, 15000), 3 * 352))
    assert cases[1][0][0] + cases[1][0][1] > yN
    return cases


def real_finish_case(core, ref, L, rng, band, off, yB, mask, note=""):
    """one band through the complex and the real entry point; all assertions of (a)"""
    import torch

    yN = core.yN_size
    start, length = band
    data = crandn(rng, (ROWS, length))
    full = numpy.zeros((ROWS, yN), dtype=complex)
    full[:, (start + numpy.arange(length)) % yN] = data
    want = ref.finish_facet(full, off, yB, axis=1).real * mask[None, :]
    dev = torch.from_numpy(data).cuda()
    complex_out = core.finish_facet_band(dev, band, off, yB, mask=mask)
    assert complex_out.dtype == torch.complex64 and tuple(complex_out.shape) == (ROWS, yB)
    obuf = torch.full((ROWS + 1, yB + 5), SENTINEL, dtype=torch.float32, device="cuda")
    out = obuf[:ROWS, 1 : yB + 1]
    # a 4-byte aligned base that is not 8-byte aligned, and for the even facet sizes of (a) an odd pitch
    assert out.data_ptr() % 8 == 4 and out.stride(0) == yB + 5 and (yB % 2 or out.stride(0) % 2 == 1)
    res = core.finish_facet_band(dev, band, off, yB, mask=mask, out=out, real=True)
    assert res is out and res.dtype == torch.float32
    assert bool((obuf[ROWS] == SENTINEL).all()) and bool((obuf[:, 0] == SENTINEL).all()) and \
        bool((obuf[:, yB + 1 :] == SENTINEL).all()), "finish_facet_band(real=True) wrote outside its rows"
    got = out.cpu().numpy()
    assert numpy.isfinite(got).all()
    assert not got[:, mask == 0].any()  # masked pixels are exactly zero
    same = torch.equal(out, complex_out.real)
    err, bound = relrms(got, want), f32_bound(L)
    peak = vector_peak(got, want, 1)
    ndiff = int((out != complex_out.real).sum())
    print(f"REALOUT finish_facet_band L={L:<3d} {err:.3e} (bound {bound:.2e}) peak {peak:.2e} "
          f"differing from complex .real: {ndiff} of {got.size} {note}")
    assert same, (L, note, ndiff)
    assert err < bound, (L, note, err, bound)
    assert peak <= 2e-5, (L, note, peak)
    # allocating form: the same values in a tensor of its own
    fresh = core.finish_facet_band(dev, band, off, yB, mask=mask, real=True)
    assert fresh.dtype == torch.float32 and tuple(fresh.shape) == (ROWS, yB) and fresh.is_contiguous()
    assert torch.equal(fresh, out)


@pytest.mark.parametrize("L", LENGTHS)
def test_real_finish_facet_band_lengths(L):
    """(a) every power-of-two length of the gate; at L = 15 the cases are checked to reach the pair instances with 13, 16
    and all 32 load segments and the geometry without pair loads"""
    core, ref = cores(params(L))
    assert core.supports_real_facets_out()
    yN = core.yN_size
    yB = facet_size(L)
    rng = numpy.random.default_rng(5100 + L)
    mask = (rng.random(yB) > 0.15).astype(float)
    assert 0 < mask.sum() < yB
    cases = sweep_bands(L, yN, yB)
    if L == 15:
        # an even start: the pair geometry, 15 or 16 segments of data (the odd start of the fourth case has no pair loads)
        cases.append(((yN // 4 + 2, 15000), 3 * 352))
        pair = [band_segments(yN, b, 1024) for b, _ in cases if b[0] % 2 == 0 and b[1] % 2 == 0]
        odd = [b for b, _ in cases if b[0] % 2 or b[1] % 2]
        assert any(s <= 13 for s in pair) and any(13 < s <= 16 for s in pair) and any(s == 32 for s in pair) and odd, (pair, odd)
    for k, (band, off) in enumerate(cases):
        real_finish_case(core, ref, L, rng, band, off, yB, mask, note=f"band {k}")


@pytest.mark.parametrize("L", [9, 15])
def test_real_finish_facet_band_odd_facet(L):
    """(b) an odd facet size at an odd facet offset: generic rows and the 32768-point kernels"""
    core, ref = cores(params(L))
    yN = core.yN_size
    yB = facet_size(L, odd=True)
    off = -(yB // 3) | 1
    assert yB % 2 == 1 and off % 2 == 1 and off < 0
    rng = numpy.random.default_rng(5200 + L)
    mask = (rng.random(yB) > 0.15).astype(float)
    for k, band in enumerate([(yN // 2 - 5 * yN // 32, 11 * yN // 32 + 8), (0, yN)]):
        real_finish_case(core, ref, L, rng, band, off, yB, mask, note=f"odd facet {yB} off {off} band {k}")


def test_real_finish_refusals():
    """(c) every refused call raises, names its reason and leaves a sentinel-filled output untouched"""
    import ctypes

    import torch

    from ska_sdp_exec_swiftly_amd import _lib

    core, _ = cores(params(9))
    yN, yB, rows = core.yN_size, facet_size(9), 4
    band = (0, yN)
    d64 = torch.zeros((rows, yN), dtype=torch.complex64, device="cuda")
    d128 = torch.zeros((rows, yN), dtype=torch.complex128, device="cuda")
    rout = torch.full((rows, yB), SENTINEL, dtype=torch.float32, device="cuda")
    cout = torch.full((rows, yB), complex(SENTINEL, SENTINEL), dtype=torch.complex64, device="cuda")
    # complex128 input: the capability table refuses
    with pytest.raises(NotImplementedError, match="complex128"):
        core.finish_facet_band(d128, band, 0, yB, out=rout, real=True)
    assert "real facet output" in _lib.last_error() and "complex128" in _lib.last_error()
    # a float32 out without real=True, a complex out with it: refused before any launch
    with pytest.raises(ValueError, match="float32"):
        core.finish_facet_band(d64, band, 0, yB, out=rout)
    with pytest.raises(ValueError, match="complex64"):
        core.finish_facet_band(d64, band, 0, yB, out=cout, real=True)
    with pytest.raises(ValueError, match="unit column stride"):
        core.finish_facet_band(d64, band, 0, yB, out=torch.full((rows, 2 * yB), SENTINEL, dtype=torch.float32, device="cuda")[:, ::2],
                               real=True)
    # overlapping output rows through the raw entry point
    cvp = ctypes.c_void_p
    lib = _lib.load()
    rc = lib.swiftly_hip_finish_facet_band_real(core._handle, _lib.C64, cvp(d64.data_ptr()), rows, d64.stride(0), 0, yN,  # pylint: disable=protected-access
                                                cvp(rout.data_ptr()), yB - 1, 0, yB, None, core._stream())  # pylint: disable=protected-access
    assert rc == _lib.ERR_PARAM and "out_row_stride" in _lib.last_error() and "facet_size" in _lib.last_error()
    # ... and the dtype argument is the INPUT dtype: complex128 there is refused too
    rc = lib.swiftly_hip_finish_facet_band_real(core._handle, _lib.C128, cvp(d128.data_ptr()), rows, d128.stride(0), 0, yN,  # pylint: disable=protected-access
                                                cvp(rout.data_ptr()), yB, 0, yB, None, core._stream())  # pylint: disable=protected-access
    assert rc == _lib.ERR_UNSUPPORTED and "complex128" in _lib.last_error()
    # yN = 3 * 2^10: the backward band runs, the real store does not exist
    coreq, _ = cores(_sizes(7, 8, 3 << 10))
    assert coreq.supports_backward_band() and not coreq.supports_real_facets_out()
    dq = torch.zeros((rows, coreq.yN_size), dtype=torch.complex64, device="cuda")
    with pytest.raises(NotImplementedError, match=r"Q \* 2\^k"):
        coreq.finish_facet_band(dq, (0, coreq.yN_size), 0, yB, out=rout, real=True)
    assert "real facet output" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((rout == SENTINEL).all()) and bool((cout == complex(SENTINEL, SENTINEL)).all())


# ------------------------------------------------------------------------------------ (d) whole passes
YB, XA = 352, 192
#: facet (off0, off1) and subgrid (off0, off1): multiples of the offset steps of both cores (128 and 2 at L = 14, 4 and 2
#: at L = 9); two waves (off1 = 0, 192) of three subgrids whose rows overlap, four facets
FACET_OFFS = [(0, 0), (384, 0), (0, 384), (-384, 384)]
SUBGRID_OFFS = [(o0, o1) for o1 in (0, 192) for o0 in (0, 192, 384)]

_PASS = {}


def pass_problem(L):
    """configuration, facets, subgrids and subgrid data of the whole-pass tests, built once per L"""
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    if L not in _PASS:
        p = params(L)
        cfg = sw.SwiftlyConfig(backend="hip", W=11.0, fov=1.0, N=p["N"], yB_size=YB, yN_size=p["yN"], xA_size=XA, xM_size=p["xM"])
        assert all(o % cfg.facet_off_step == 0 for offs in FACET_OFFS for o in offs)
        assert all(o % cfg.subgrid_off_step == 0 for offs in SUBGRID_OFFS for o in offs)
        mask = numpy.ones(YB)
        mask[:17] = 0
        facets = [sw.FacetConfig(o0, o1, YB, None if i % 2 else mask, mask if i % 2 else None) for i, (o0, o1) in enumerate(FACET_OFFS)]
        sgs = [sw.SubgridConfig(o0, o1, XA) for o0, o1 in SUBGRID_OFFS]
        gen = torch.Generator(device="cpu").manual_seed(70 + L)
        data = [torch.randn((XA, XA), dtype=torch.complex64, generator=gen).cuda() for _ in sgs]
        _PASS[L] = (sw, cfg, facets, sgs, data)
    return _PASS[L]


def run_pass(L, wave_axis, **kw):
    """one backward pass; returns the object, its facets and the device memory ``finish()`` added at its peak"""
    import torch

    sw, cfg, facets, sgs, data = pass_problem(L)
    plan = dict(subgrid_configs=sgs) if wave_axis == 1 else {}
    bwd = sw.SwiftlyBackward(cfg, facets, wave_axis=wave_axis, **plan, **kw)
    bwd.add_new_subgrid_tasks(sgs, data)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = bwd.finish()
    torch.cuda.synchronize()
    return bwd, out, torch.cuda.max_memory_allocated() - before


@pytest.mark.parametrize("L", [9, 14])
def test_backward_real_facets_band_schedule(L):
    """the band schedule with and without ``facet_dtype=torch.float32`` on the same subgrids: equal real parts, the native
    path, and no complex facet in the real run"""
    import torch

    bwd_c, out_c, peak_c = run_pass(L, 1)
    assert bwd_c.facet_dtype == torch.complex64 and bwd_c.real_finish_native is False
    bwd_r, out_r, peak_r = run_pass(L, 1, facet_dtype=torch.float32)
    assert bwd_r.facet_dtype == torch.float32 and bwd_r.real_finish_native is True
    assert len(out_r) == len(out_c) == len(FACET_OFFS)
    for fr, fc in zip(out_r, out_c):
        assert fr.dtype == torch.float32 and fc.dtype == torch.complex64 and tuple(fr.shape) == (YB, YB)
        assert bool(fc.real.abs().max() > 0)
        assert torch.equal(fr, fc.real)
    # Memory.  max_memory_allocated counts the bytes of live tensors, each rounded up to the allocator's 512-byte
    # granule, and finish() allocates nothing but the facets: 4 x 352^2 x 8 B = 3.97 MB complex, 1.98 MB real.  The
    # facets are sized so that the margin asked for -- half the complex bytes minus one complex facet, 0.99 MB -- is far
    # above the rounding (at most 512 B per facet), and so that a single complex facet (0.99 MB) could not hide in the
    # real run either.
    facet_c = YB * YB * 8
    total_c = len(out_c) * facet_c
    print(f"REALOUT pass L={L}: finish() peak complex {peak_c} B, real {peak_r} B (complex facets {total_c} B)")
    assert peak_c >= total_c
    assert peak_c - peak_r >= total_c // 2 - facet_c
    assert peak_r < total_c // 2 + facet_c // 2, "the real run allocated a complex tensor of facet size"


def test_backward_real_facets_other_paths():
    """a pass without contributions, the reference's schedule (``wave_axis=0``) and delayed results"""
    import torch

    L = 9
    sw, cfg, facets, sgs, _ = pass_problem(L)
    # no contribution: float32 zeros
    for axis in (0, 1):
        empty = sw.SwiftlyBackward(cfg, facets, wave_axis=axis, subgrid_configs=sgs if axis else None, facet_dtype=torch.float32)
        zeros = empty.finish()
        assert len(zeros) == len(facets)
        assert all(z.dtype == torch.float32 and tuple(z.shape) == (YB, YB) and not bool(z.any()) for z in zeros)
    # wave_axis=0: complex finish, real part copied out
    _, out_c, _ = run_pass(L, 0)
    bwd_r, out_r, _ = run_pass(L, 0, facet_dtype=torch.float32)
    assert bwd_r.real_finish_native is False and bwd_r.facet_dtype == torch.float32
    for fr, fc in zip(out_r, out_c):
        assert fr.dtype == torch.float32 and fr.is_contiguous() and tuple(fr.shape) == (YB, YB)
        assert bool(fc.real.abs().max() > 0) and torch.equal(fr, fc.real)
    # delayed=True: tasks that resolve to float32, equal to the band schedule's complex real parts
    _, band_c, _ = run_pass(L, 1)
    _, tasks, _ = run_pass(L, 1, facet_dtype=torch.float32, delayed=True)
    for task, fc in zip(tasks, band_c):
        assert isinstance(task, sw.DeviceTask) and task.dtype == torch.float32
        host = task.compute()
        assert host.dtype == numpy.float32 and numpy.array_equal(host, fc.real.cpu().numpy())
    # complex64 data into a float64 request: refused at the first data
    bad = sw.SwiftlyBackward(cfg, facets, wave_axis=0, facet_dtype=torch.float64)
    with pytest.raises(ValueError, match="does not match"):
        bad.add_new_subgrid_tasks(sgs[:1], [torch.zeros((XA, XA), dtype=torch.complex64, device="cuda")])
