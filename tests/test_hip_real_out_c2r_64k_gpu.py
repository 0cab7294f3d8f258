"""
The half-length backward finish of real-valued facets on 65536-point band rows (``swiftly_hip_finish_facet_band_c2r`` on a
handle ``SWIFTLY_FEATURE_REAL_FACETS_OUT_C2R_64K`` supports; csrc/swiftly_rowc2r.h, the 1024-thread instance) on the GPU: the
recombination of a band row and its mirror into one 32768-point complex transform per row, the loads that are skipped
because their 1024 indices lie outside the band, the pair store into the float32 facet row.  The cases of
tests/test_hip_real_out_c2r_gpu.py at the scaled sizes.

Every expected value comes from the complex128 oracle (``OracleCore.finish_facet`` along the contiguous axis, real part,
times the mask): no other HIP path is a reference here, because the half-length form rounds differently from the real-store
form -- which is also how the tests see that it ran.  Bounds: the project's relative RMSE of one float32 transform,
``f32_bound(16)`` = 2e-6, and per row ``max|err| <= 2e-5 max|want|`` (``PEAK_BOUND``), both of tests/_band_sweep_worker.py.
Every case prints a ``C2R64K`` line with the relative RMSE of both forms.

The whole passes compare the half-length run with the real-store run on bit-identical band accumulators, as the whole-pass
test of tests/test_hip_real_out_c2r_gpu.py does: each is within the bound of the exact transform of those accumulators, so
they differ by at most twice the bound.  Facets of one pass share their size and every facet offset is a multiple of an
even step, so "a facet at an odd position" is a pass whose facets have 354 pixels (``yN/2 - 177`` is odd).

Measured (MI355X, the cases below; relative RMSE against the oracle, half-length form / real-store form on the same rows):

    facets 704 .. 65534 pixels, plan-like band (48 pairs)   1.68e-7 .. 1.83e-7  /  1.63e-7 .. 1.81e-7
    full band (all 128 pairs loaded)                        1.83e-7  /  1.78e-7
    wrapping band (10 pairs), odd start and length (48)     1.72e-7, 1.78e-7  /  1.69e-7, 1.75e-7
    two columns (3 pairs loaded)                            1.03e-7  /  1.50e-7

of the bound 2e-6.  Worst per-row peak 3.9e-7 (the two-column band), 2.3e-7 .. 3.3e-7 elsewhere; impulse rows 3.4e-7 of the row
peak; anti-Hermitian rows exactly zero; whole pass against the real-store pass 1.6e-7 per facet (bound 4e-6).
"""
import ctypes

import numpy
import pytest

from _band_sweep_worker import PEAK_BOUND, cores, f32_bound, last_instance, relrms, vector_peak

pytestmark = pytest.mark.gpu

YN, M, T, P = 65536, 32768, 1024, 32
PREFIX = "real facets out, half-length:"
PLAN_BAND = (21440, 22976)
BOUND = f32_bound(16)
SENTINEL = 7.5
#: (facet size, facet offset): a small facet; the three cover offsets of the 128k workload; 49152 points; nearly the whole row
#: (whose position in the padded row is even at ODD facet offsets: ``yN/2 - 32767`` is odd)
FACETS = [(704, 8194), (45056, 0), (45056, 45056), (45056, -45056), (49152, 666), (65534, 667)]
#: whole axis; the plan-like band; wrapping past 65535; odd start and odd length; two columns
BANDS = [(0, YN), PLAN_BAND, (64001, 4097), (21473, 22943), (32767, 2)]
_data, _masks, _want = {}, {}, {}


def loaded_pairs(band):
    """(register, source) pairs the kernel requests: the 1024 consecutive band indices of a pair are not wholly outside the
    band (sources 0 / 1 ascend with the lane, 2 / 3 descend) -- ``loaded_pairs`` of tests/test_real_out_c2r_model_cpu.py at
    T = 1024"""
    start, length = band
    count = 0
    for r in range(P):
        for base in ((T * r + M - start) % YN, (T * r - start) % YN, (M - start - T * r - (T - 1)) % YN, (-start - T * r - (T - 1)) % YN):
            count += not (base >= length and base + (T - 1) < YN)
    return count


def _rows(rows, length):
    """complex64 band rows, seeded by the shape: shared, never changed"""
    if (rows, length) not in _data:
        rng = numpy.random.default_rng(8000 + 13 * rows + length)
        _data[rows, length] = (rng.standard_normal((rows, length)) + 1j * rng.standard_normal((rows, length))).astype(numpy.complex64)
    return _data[rows, length]


def _mask(yB):
    """a mask with zeros, float64 on the host"""
    if yB not in _masks:
        _masks[yB] = (numpy.random.default_rng(yB).random(yB) > 0.15).astype(float)
        assert 0 < _masks[yB].sum() < yB
    return _masks[yB]


def _oracle(data, band, off, yB, mask, key=None):
    """``finish_facet(full, off, yB, axis=1).real * mask`` in complex128, once per ``key``"""
    if key is None or key not in _want:
        start, length = band
        full = numpy.zeros((data.shape[0], YN), dtype=complex)
        full[:, (start + numpy.arange(length)) % YN] = data
        want = cores("c16")[1].finish_facet(full, off, yB, axis=1).real
        if mask is not None:
            want = want * mask[None, :]
        if key is None:
            return want
        _want[key] = want
    return _want[key]


def _device_rows(x, pitch=None, fill=0.0):
    import torch

    pitch = pitch or x.shape[1]
    storage = torch.full((x.shape[0], pitch), complex(fill, fill), dtype=torch.complex64, device="cuda")
    view = storage[:, : x.shape[1]]
    view.copy_(torch.from_numpy(x))
    return view


def _frame(rows, yB, pitch=None, base=2):
    """a sentinel-filled float32 buffer ``[rows + 2, pitch]`` and the view ``[rows, yB]`` inside it: by default an even
    pitch larger than yB and a base that is 8-byte but not 16-byte aligned"""
    import torch

    pitch = pitch or yB + (12 if yB % 4 == 0 else 14)
    frame = torch.full((rows + 2, pitch), SENTINEL, dtype=torch.float32, device="cuda")
    return frame, frame[1 : rows + 1, base : base + yB]


def _frame_intact(frame, rows, yB, base=2):
    ok = (frame[0] == SENTINEL).all() and (frame[rows + 1] == SENTINEL).all()
    return bool(ok and (frame[:, :base] == SENTINEL).all() and (frame[:, base + yB :] == SENTINEL).all())


def _mask_on_device(mask):
    import torch

    return None if mask is None else torch.from_numpy(mask.astype(numpy.float32)).cuda()


def _call(core, src, band, off, yB, mask, out, dtype=None, out_stride=None):
    """the raw entry point: its return code (the device is idle afterwards)"""
    import torch

    from ska_sdp_exec_swiftly_amd import _lib

    mdev = _mask_on_device(mask)
    cvp = ctypes.c_void_p
    rc = _lib.load().swiftly_hip_finish_facet_band_c2r(
        core._handle, _lib.C64 if dtype is None else dtype, cvp(src.data_ptr()), src.shape[0], src.stride(0), band[0], band[1],  # pylint: disable=protected-access
        cvp(out.data_ptr()), out.stride(0) if out_stride is None else out_stride, off, yB, cvp(mdev.data_ptr()) if mdev is not None else None,
        None)
    torch.cuda.synchronize()
    return rc


def _check(yB, off, band, rows, in_pitch=None, fill=0.0):
    """one call against the oracle: the frame, masked pixels, RMSE and per-row peak, and the dispatch; returns the RMSE"""
    import torch

    from ska_sdp_exec_swiftly_amd import _lib

    core, _ = cores("c16")
    data, mask = _rows(rows, band[1]), _mask(yB)
    src = _device_rows(data, in_pitch, fill)
    frame, out = _frame(rows, yB)
    assert out.data_ptr() % 16 == 8 and out.stride(0) % 2 == 0 and out.stride(0) > yB
    before, _ = last_instance()
    rc = _call(core, src, band, off, yB, mask, out)
    assert rc == 0, _lib.last_error()
    assert last_instance()[0] == before, "a half-length call went through the band row kernel's launcher"
    assert _frame_intact(frame, rows, yB), "wrote outside the facet rows"
    got = out.cpu().numpy()
    assert got.dtype == numpy.float32 and numpy.isfinite(got).all()
    assert not got[:, mask == 0].any(), "a masked pixel is not exactly zero"
    want = _oracle(data, band, off, yB, mask, key=(rows, band, off, yB))
    # the real-store form on the same rows: its figure, and a different rounding
    store = core.finish_facet_band(src, band, off, yB, mask=mask, real=True)
    err, err_store = relrms(got, want), relrms(store.cpu().numpy(), want)
    peak = vector_peak(got.astype(numpy.complex64), want, 1)
    print(f"C2R64K size {yB} off {off} band {band} rows {rows}: relrmse {err:.3e} (real-store form {err_store:.3e}, bound {BOUND:.2e}) "
          f"peak {peak:.2e}, {loaded_pairs(band)} of 128 (register, source) pairs loaded")
    assert err < BOUND, (yB, off, band, err)
    assert peak <= PEAK_BOUND, (yB, off, band, peak)
    assert not torch.equal(out, store), "bit for bit the real-store form: did the half-length kernel run?"
    return err


@pytest.mark.parametrize("yB,off", FACETS, ids=[f"{s}@{o}" for s, o in FACETS])
def test_facet_sizes_and_offsets(yB, off):
    """every facet class on the plan-like band (7 rows), a mask with zeros"""
    _check(yB, off, PLAN_BAND, rows=7)


@pytest.mark.parametrize("band", BANDS, ids=[f"{s}+{n}" for s, n in BANDS])
def test_bands(band):
    """whole axis (every pair loaded), the plan-like band, a band that wraps past 65535, odd start with odd length, two
    columns: 9 rows (a second block of eight)"""
    _check(45056, 45056, band, rows=9)


def test_impulse_band_rows():
    """rows that are ONE column holding 1 + 2i: plain k = 0, M/2, M, 3M/2 (their own mirrors or each other's), 1024 v and
    1024 v + M for every v (lane 0's sources, whose mirrors are lane 0's too) and two ordinary columns, element by element
    within the per-row peak bound.  No mask: the window is the PSWF table itself."""
    from ska_sdp_exec_swiftly_amd import _lib

    core, _ = cores("c16")
    yB, off, band = 45056, 0, (0, YN)
    v = T * numpy.arange(32)
    plain = numpy.unique(numpy.concatenate([[0, M // 2, M, M + M // 2], v, v + M, [2468, 40001]]))
    data = numpy.zeros((len(plain), YN), dtype=numpy.complex64)
    data[numpy.arange(len(plain)), (plain + YN // 2) % YN] = 1 + 2j  # band (0, yN): element d is centred column d
    frame, out = _frame(len(plain), yB)
    rc = _call(core, _device_rows(data), band, off, yB, None, out)
    assert rc == 0, _lib.last_error()
    assert _frame_intact(frame, len(plain), yB)
    want = _oracle(data, band, off, yB, None)
    got = out.cpu().numpy()
    tol = PEAK_BOUND * numpy.abs(want).max(axis=1)[:, None]
    err = numpy.abs(got - want)
    print(f"C2R64K impulses: worst |err| / (row peak) {float((err / tol).max()) * PEAK_BOUND:.2e} over {len(plain)} rows")
    assert (tol > 0).all()
    assert (err <= tol).all(), (plain[(err > tol).any(axis=1)], float((err / tol).max()))


def test_anti_hermitian_rows_give_nothing():
    """a full-axis row with X[k] = -conj X[N - k] has a purely imaginary transform: the output stays below
    2e-5 max|cfft(X)| -- the Hermitian part is really formed (a 352-pixel facet at the centre: the window is about 1)"""
    from ska_sdp_exec_swiftly_amd import _lib

    core, ref = cores("c16")
    rows, yB, off, band = 7, 352, 0, (0, YN)
    rng = numpy.random.default_rng(78)
    plain = (rng.standard_normal((rows, YN)) + 1j * rng.standard_normal((rows, YN))).astype(numpy.complex64)
    k = numpy.arange(YN)
    plain = (plain - numpy.conj(plain[:, (YN - k) % YN])).astype(numpy.complex64)
    assert numpy.array_equal(plain, -numpy.conj(plain[:, (YN - k) % YN])) and numpy.abs(plain).min(axis=1).max() > 0
    data = numpy.ascontiguousarray(plain[:, (k - YN // 2) % YN])  # centred column c holds plain (c - N/2) mod N
    spectrum = numpy.fft.fft(plain.astype(complex), axis=1)
    assert numpy.abs(spectrum.real).max() < 1e-9 * numpy.abs(spectrum).max()
    assert ref.facet_window(yB).max() < 1.5
    frame, out = _frame(rows, yB)
    rc = _call(core, _device_rows(data), band, off, yB, None, out)
    assert rc == 0, _lib.last_error()
    assert _frame_intact(frame, rows, yB)
    got = numpy.abs(out.cpu().numpy()).max(axis=1)
    limit = 2e-5 * numpy.abs(spectrum).max(axis=1)
    print(f"C2R64K anti-Hermitian rows: max|out| / max|cfft(X)| = {float((got / limit).max()) * 2e-5:.2e}")
    assert (got <= limit).all(), (got, limit)
    # ... and the same rows give the oracle's facet once they are not anti-Hermitian any more
    data2 = data.copy()
    data2[:, 5000] += 3 - 1j
    rc = _call(core, _device_rows(data2), band, off, yB, None, out)
    assert rc == 0, _lib.last_error()
    want = _oracle(data2, band, off, yB, None)
    assert vector_peak(out.cpu().numpy().astype(numpy.complex64), want, 1) <= PEAK_BOUND


def test_nan_gap_between_the_input_rows():
    """input rows at a pitch larger than the band whose gap holds NaN: nothing outside the band rows is read into the
    result (the output sits, as everywhere here, in a sentinel frame at an even pitch on an 8-byte, not 16-byte aligned base)"""
    _check(45056, -45056, PLAN_BAND, rows=7, in_pitch=PLAN_BAND[1] + 37, fill=float("nan"))
    _check(704, 8194, (21473, 22943), rows=7, in_pitch=22943 + 1, fill=float("nan"))


def test_refusals_write_nothing():
    """odd facet size, odd position, odd out pitch, a 4-byte-aligned out, complex128, a 16384-point core: ERR_UNSUPPORTED with
    the prefix; overlapping output rows: ERR_PARAM.  The output keeps its sentinel and no kernel ran."""
    import torch

    from ska_sdp_exec_swiftly_amd import _lib

    core, _ = cores("c16")
    small, _ = cores("c14")
    rows, yB = 7, 45056
    src = _device_rows(_rows(rows, PLAN_BAND[1]))
    src128 = src.to(torch.complex128)
    src14 = _device_rows(_rows(rows, 5477))
    # name: (core, rows, band, off, yB, frame pitch, base, dtype, stride handed over, code)
    cases = {
        "odd facet size": (core, src, PLAN_BAND, 1, yB - 1, yB + 12, 2, None, None, _lib.ERR_UNSUPPORTED),
        "odd position": (core, src, PLAN_BAND, 45057, yB, yB + 12, 2, None, None, _lib.ERR_UNSUPPORTED),
        "odd out pitch": (core, src, PLAN_BAND, 0, yB, yB + 13, 2, None, None, _lib.ERR_UNSUPPORTED),
        "4-byte out": (core, src, PLAN_BAND, 0, yB, yB + 12, 1, None, None, _lib.ERR_UNSUPPORTED),
        "complex128": (core, src128, PLAN_BAND, 0, yB, yB + 12, 2, _lib.C128, None, _lib.ERR_UNSUPPORTED),
        "16384-point core": (small, src14, (5461, 5477), 0, 11264, 11264 + 12, 2, None, None, _lib.ERR_UNSUPPORTED),
        "overlapping rows": (core, src, PLAN_BAND, 0, yB, yB + 12, 2, None, yB - 2, _lib.ERR_PARAM),
    }
    before, _ = last_instance()
    for name, (c, s, band, off, size, pitch, base, dtype, stride, code) in cases.items():
        frame, out = _frame(rows, size, pitch, base)
        rc = _call(c, s, band, off, size, _mask(size) if size == yB else None, out, dtype=dtype, out_stride=stride)
        assert rc == code, (name, rc, _lib.last_error())
        if code == _lib.ERR_UNSUPPORTED:
            assert PREFIX in _lib.last_error(), (name, _lib.last_error())
        else:
            assert "out_row_stride" in _lib.last_error() and "facet_size" in _lib.last_error(), _lib.last_error()
        assert bool((frame == SENTINEL).all()), name
    assert last_instance()[0] == before
    # the same refusals through the Python door: the library's NotImplementedError, nothing written
    assert core.supports_real_facets_out_c2r() and not small.supports_real_facets_out_c2r()
    doors = {
        "odd facet size": (core, src, PLAN_BAND, 1, yB - 1, yB + 12, 2),
        "odd position": (core, src, PLAN_BAND, 45057, yB, yB + 12, 2),
        "odd out pitch": (core, src, PLAN_BAND, 0, yB, yB + 13, 2),
        "4-byte out": (core, src, PLAN_BAND, 0, yB, yB + 12, 1),
        "complex128": (core, src128, PLAN_BAND, 0, yB, yB + 12, 2),
        "16384-point core": (small, src14, (5461, 5477), 0, 11264, 11264 + 12, 2),
    }
    for name, (c, s, band, off, size, pitch, base) in doors.items():
        frame, out = _frame(rows, size, pitch, base)
        with pytest.raises(NotImplementedError, match=PREFIX):
            c.finish_facet_band(s, band, off, size, out=out, real=True, half_length=True)
        torch.cuda.synchronize()
        assert bool((frame == SENTINEL).all()), name
    with pytest.raises(ValueError, match="needs real=True"):
        core.finish_facet_band(src, PLAN_BAND, 0, yB, half_length=True)
    assert last_instance()[0] == before


def test_python_door_matches_the_entry_point():
    """``finish_facet_band(..., real=True, half_length=True)``: the entry point's bits, into ``out`` and into a tensor of its own"""
    import torch

    core, _ = cores("c16")
    rows, yB, off = 7, 45056, 0
    data, mask = _rows(rows, PLAN_BAND[1]), _mask(yB)
    src = _device_rows(data)
    _, raw = _frame(rows, yB)
    assert _call(core, src, PLAN_BAND, off, yB, mask, raw) == 0
    frame, out = _frame(rows, yB)
    res = core.finish_facet_band(src, PLAN_BAND, off, yB, mask=mask, out=out, real=True, half_length=True)
    assert res is out and torch.equal(out, raw) and _frame_intact(frame, rows, yB)
    fresh = core.finish_facet_band(src, PLAN_BAND, off, yB, mask=mask, real=True, half_length=True)
    assert fresh.dtype == torch.float32 and tuple(fresh.shape) == (rows, yB) and torch.equal(fresh, raw)


# -- the whole pass ---------------------------------------------------------------------------------------------------
#: the whole-pass problem of tests/test_hip_real_out_c2r_gpu.py on the 65536-point sweep core (``params(16)`` of
#: tests/test_hip_facet_sweep_gpu.py: facet offset step 512): facet offsets of 1536 -- 352-pixel facets at even positions --
#: the same subgrids (two waves of three whose rows overlap) and the same masks
YB, XA = 352, 192
FACET_OFFS_16 = [(0, 0), (1536, 0), (0, 1536), (-1536, 1536)]
SUBGRID_OFFS = [(o0, o1) for o1 in (0, 192) for o0 in (0, 192, 384)]
_PASS = {}


def _pass_problem(yB=YB):
    import torch

    import ska_sdp_exec_swiftly_amd as sw
    from test_hip_facet_sweep_gpu import params

    if yB not in _PASS:
        p = params(16)
        cfg = sw.SwiftlyConfig(backend="hip", W=11.0, fov=1.0, N=p["N"], yB_size=yB, yN_size=p["yN"], xA_size=XA, xM_size=p["xM"])
        assert p["yN"] == YN
        assert all(o % cfg.facet_off_step == 0 for offs in FACET_OFFS_16 for o in offs)
        assert all(o % cfg.subgrid_off_step == 0 for offs in SUBGRID_OFFS for o in offs)
        mask = numpy.ones(yB)
        mask[:17] = 0
        facets = [sw.FacetConfig(o0, o1, yB, None if i % 2 else mask, mask if i % 2 else None) for i, (o0, o1) in enumerate(FACET_OFFS_16)]
        sgs = [sw.SubgridConfig(o0, o1, XA) for o0, o1 in SUBGRID_OFFS]
        gen = torch.Generator(device="cpu").manual_seed(86)
        data = [torch.randn((XA, XA), dtype=torch.complex64, generator=gen).cuda() for _ in sgs]
        _PASS[yB] = (sw, cfg, facets, sgs, data)
    return _PASS[yB]


def _run_pass(yB=YB, **kw):
    """one backward pass on the band schedule: the object and its facets"""
    import torch

    sw, cfg, facets, sgs, data = _pass_problem(yB)
    bwd = sw.SwiftlyBackward(cfg, facets, wave_axis=1, subgrid_configs=sgs, **kw)
    bwd.add_new_subgrid_tasks(sgs, data)
    out = bwd.finish()
    torch.cuda.synchronize()
    return bwd, out


def test_backward_half_length_finish():
    """352-pixel facets at even positions: the half-length finish runs, stays within twice the bound of the real-store run
    on the same accumulators, and is not that run; without the keyword nothing changes"""
    import torch

    sw, cfg, facets, _, _ = _pass_problem()
    assert all(f.size % 2 == 0 and (YN // 2 - f.size // 2 + f.off1) % 2 == 0 for f in facets)
    bwd_r, out_r = _run_pass(facet_dtype=torch.float32)
    assert bwd_r.real_finish_native is True and bwd_r.half_length_finish is False
    bwd_h, out_h = _run_pass(facet_dtype=torch.float32, half_length_finish=True)
    assert bwd_h.half_length_finish is True and bwd_h.real_finish_native is True and bwd_h.facet_dtype == torch.float32
    assert len(out_h) == len(out_r) == len(facets)
    worst = 0.0
    for fh, fr in zip(out_h, out_r):
        assert fh.dtype == torch.float32 and tuple(fh.shape) == tuple(fr.shape) == (YB, YB) and fh.is_contiguous()
        assert bool(fr.abs().max() > 0)
        worst = max(worst, relrms(fh.cpu().numpy().astype(float), fr.cpu().numpy().astype(float)))
    print(f"C2R64K whole pass: worst facet relative RMSE against the real-store run {worst:.3e} (bound {2 * BOUND:.2e})")
    assert worst < 2 * BOUND, worst
    assert not all(torch.equal(fh, fr) for fh, fr in zip(out_h, out_r)), "the half-length form rounds differently: did it run?"
    # without the keyword, and with it switched off: today's bits
    for kw in ({}, dict(half_length_finish=False)):
        bwd, out = _run_pass(facet_dtype=torch.float32, **kw)
        assert bwd.half_length_finish is False
        assert all(torch.equal(a, b) for a, b in zip(out, out_r)), kw
    # the reference's schedule has no half-length finish
    bwd0 = sw.SwiftlyBackward(cfg, facets, wave_axis=0, facet_dtype=torch.float32, half_length_finish=True)
    assert bwd0.half_length_finish is False and bwd0.real_finish_native is False


def test_backward_odd_position_runs_what_it_runs_today():
    """354-pixel facets sit at odd positions of the padded row (the facets of a pass share their size, and every facet offset
    is a multiple of an even step): the object says so and gives the real-store form's bits"""
    import torch

    yB = 354
    _, _, facets, _, _ = _pass_problem(yB)
    assert all(f.size % 2 == 0 and (YN // 2 - yB // 2 + f.off1) % 2 == 1 for f in facets)
    _, today = _run_pass(yB, facet_dtype=torch.float32)
    bwd, out = _run_pass(yB, facet_dtype=torch.float32, half_length_finish=True)
    assert bwd.half_length_finish is False and bwd.real_finish_native is True
    assert all(o.dtype == torch.float32 and tuple(o.shape) == (yB, yB) and bool(o.abs().max() > 0) for o in out)
    assert all(torch.equal(o, t) for o, t in zip(out, today))
