"""
The half-length K1 of real-valued facets on 65536-point rows (``swiftly_hip_prepare_facet_band_rfft`` / ``_rows_rfft`` on a
handle ``SWIFTLY_FEATURE_REAL_FACETS_RFFT_64K`` supports; csrc/swiftly_rowreal.h, the 1024-thread instance) on the GPU: one
32768-point complex transform per 65536-point real row, the mirror exchange in the 132 KB buffer (whose far half no LDS
instruction reaches from the lane's base), the recombination, the parity-split band store.  The cases of
tests/test_hip_real_rfft_gpu.py at the scaled sizes.

Every expected value comes from the complex128 oracle (``OracleCore.prepare_facet`` along the contiguous axis, times
``facet_window`` of the other axis where that window is folded): no other HIP path is a reference here.  Bounds: the
project's relative RMSE of one float32 transform, ``f32_bound(16)`` = 2e-6, and per row ``max|err| <= 2e-5 max|want|``
(``PEAK_BOUND``), both of tests/_band_sweep_worker.py.

Facet sizes: the entry points take ``facet_size < yN_size``, so "all 32 segments" is the 65534-point facet (whose position
in the padded row is even at ODD facet offsets: ``yN/2 - 32767`` is odd).  The whole pass runs the 128k workload's
parameters (W 10.875, N 131072, yN 65536, xA 928, xM 1024) on the small-rows problem of
tests/test_hip_band_pipeline_gpu.py: three 352 x 352 real separable facets, 12 subgrids in 4 waves.

Measured (MI355X, the cases below, worst relative RMSE against the oracle per facet size = data segments of 32):

    704 points (1 segment)             1.68e-7
    45056 points (22 segments)         1.82e-7   (aligned offset; 1.77e-7 .. 1.95e-7 over bands, row counts, folding)
    45056 points (24 segments, wraps)  1.81e-7
    49152 points (24 segments)         1.73e-7
    65534 points (32 segments)         1.63e-7

of the bound 2e-6; the two-column band 1.33e-7.  Worst per-row peak 5.0e-7 (the two-column band), 2.4e-7 .. 3.1e-7 elsewhere;
self-mirrored outputs and lane 0 within 1.0e-7 of the row peak element by element; impulse rows within 4.3e-7 of the modulus;
whole pass on the small-rows problem 3.9e-7 (bound 2e-5).
"""
import ctypes

import numpy
import pytest

import bench
from _band_sweep_worker import PEAK_BOUND, SENTINEL, band_cols, cores, f32_bound, last_instance, relrms, vector_peak
from oracle import separable as sep
from oracle import swiftly_oracle as orc

pytestmark = pytest.mark.gpu

YN, M, T = 65536, 32768, 1024
PREFIX = "real facets, half-length:"
PLAN_BAND = (21440, 22976)
BOUND = f32_bound(16)
#: (facet size, facet offset): one segment of 2048 reals; the three cover offsets of the 128k workload (22 segments at the
#: aligned position, 24 where the data wraps around the end of the padded row); 49152 points; all 32 segments
FACETS = [(704, 2 * 4097), (45056, 0), (45056, 45056), (45056, -45056), (49152, 2 * 333), (65534, 2 * 333 + 1)]
#: whole axis; the plan-like band; odd start and odd length, wrapping past 65535; two columns
BANDS = [(0, YN), PLAN_BAND, (64001, 4097), (32767, 2)]
_rows, _want = {}, {}


def _x(rows, size):
    """float32 rows, seeded by the shape: shared, never changed"""
    if (rows, size) not in _rows:
        _rows[rows, size] = numpy.random.default_rng(6000 + 17 * rows + size).standard_normal((rows, size)).astype(numpy.float32)
    return _rows[rows, size]


def _oracle(x, key, off):
    """``prepare_facet(x, off, axis=1)`` in complex128, once per (rows, offset)"""
    if (key, off) not in _want:
        _want[key, off] = cores("c16")[1].prepare_facet(x.astype(complex), off, 1)
    return _want[key, off]


def _device_rows(x, pitch=None, base=0, fill=0.0):
    import torch

    pitch = pitch or x.shape[1]
    storage = torch.full((x.shape[0], pitch), fill, dtype=torch.float32, device="cuda")
    view = storage[:, base : base + x.shape[1]]
    view.copy_(torch.from_numpy(x))
    return view


def _call(core, src, size, off, band, fold_rows=0, row0=0, dtype=None, rows_entry=False):
    """the raw entry point on a sentinel-framed output: ``(rc, frame, out)``"""
    import torch

    from ska_sdp_exec_swiftly_amd import _lib

    rows, ncols = src.shape[0], core.band_columns(band)
    frame = torch.full((rows + 2, ncols + 12), SENTINEL, dtype=torch.complex64, device="cuda")
    out = frame[1 : rows + 1, 4 : 4 + ncols]
    lib = _lib.load()
    args = (core._handle, _lib.C64 if dtype is None else dtype, ctypes.c_void_p(src.data_ptr()), rows, size, src.stride(0),  # pylint: disable=protected-access
            ctypes.c_void_p(out.data_ptr()), out.stride(0), off, band[0], band[1])
    if rows_entry:
        rc = lib.swiftly_hip_prepare_facet_band_rows_rfft(*args, fold_rows, row0, None)
    else:
        rc = lib.swiftly_hip_prepare_facet_band_rfft(*args, int(bool(fold_rows)), None)
    torch.cuda.synchronize()
    return rc, frame, out


def _frame_intact(frame, rows, ncols):
    ok = (frame[0] == SENTINEL).all() and (frame[rows + 1] == SENTINEL).all()
    return bool(ok and (frame[:, :4] == SENTINEL).all() and (frame[:, 4 + ncols :] == SENTINEL).all())


def _check(size, off, band, rows, fold=False, rows_of=None, pitch=None, base=0, fill=0.0):
    """one call against the oracle: RMSE, per-row peak, the frame and the columns outside the band; returns the RMSE"""
    from ska_sdp_exec_swiftly_amd import _lib

    core, ref = cores("c16")
    x = _x(rows, size)
    src = _device_rows(x, pitch, base, fill)
    assert src.data_ptr() % 16 == (4 * base) % 16 and src.data_ptr() % 8 == 0 and src.stride(0) % 2 == 0
    before, _ = last_instance()
    if rows_of is not None:
        rc, frame, out = _call(core, src, size, off, band, rows_of[0], rows_of[1], rows_entry=True)
    else:
        rc, frame, out = _call(core, src, size, off, band, rows if fold else 0)
    assert rc == 0, _lib.last_error()
    assert last_instance()[0] == before, "a half-length call went through the band row kernel's launcher"
    want = _oracle(x, (rows, size), off)
    if rows_of is not None:
        want = want * ref.facet_window(rows_of[0])[rows_of[1] : rows_of[1] + rows, None]
    elif fold:
        want = want * ref.facet_window(rows)[:, None]
    ncols = core.band_columns(band)
    assert _frame_intact(frame, rows, ncols), "wrote outside the band buffer"
    pc = band_cols(YN, band)
    keep = pc >= 0
    got = out.cpu().numpy()
    outside = numpy.ones(ncols, dtype=bool)
    outside[pc[keep]] = False
    assert (got[:, outside] == SENTINEL).all(), "a column outside the band was written"
    got, want = got[:, pc[keep]], want[:, keep]
    assert got.dtype == numpy.complex64 and numpy.isfinite(got).all()
    err, peak = relrms(got, want), vector_peak(got, want, 1)
    print(f"RFFT64K size {size} off {off} band {band} rows {rows} fold {fold or rows_of}: relrmse {err:.3e} (bound {BOUND:.2e}) peak {peak:.2e}")
    assert err < BOUND, (size, off, band, err)
    assert peak <= PEAK_BOUND, (size, off, band, peak)
    return err


@pytest.mark.parametrize("size,off", FACETS, ids=[f"{s}@{o}" for s, o in FACETS])
def test_facet_sizes_and_offsets(size, off):
    """every segment count on the plan-like band (7 rows) -- 1, 22, 24 (wrapping), 24 and all 32 segments"""
    _check(size, off, PLAN_BAND, rows=7)


@pytest.mark.parametrize("band", BANDS, ids=[f"{s}+{n}" for s, n in BANDS])
def test_bands(band):
    """whole axis, the plan-like band, a band with odd start and odd length that wraps past 65535, two columns: 9 rows (a
    second block of eight), the other axis' window folded"""
    _check(45056, 45056, band, rows=9, fold=True)


@pytest.mark.parametrize("rows", [1, 7, 9])
def test_row_counts_without_the_folded_window(rows):
    _check(45056, -45056, PLAN_BAND, rows=rows)


def test_rows_of_a_larger_facet():
    """rows [100, 107) of a facet with 704 rows: the folded window is that facet's"""
    _check(45056, 0, PLAN_BAND, rows=7, rows_of=(704, 100))


def test_self_mirrored_outputs_and_lane_zero():
    """whole axis: plain outputs k = 0, M/2, M, M + M/2 (their own mirrors) and every output lane 0 owns (e = 1024 v, whose
    mirror is lane 0's register (32 - v) mod 32), element by element within the per-row peak bound"""
    from ska_sdp_exec_swiftly_amd import _lib

    core, _ = cores("c16")
    size, off, rows = 45056, 45056, 7
    x = _x(rows, size)
    rc, _, out = _call(core, _device_rows(x), size, off, (0, YN))
    assert rc == 0, _lib.last_error()
    want = _oracle(x, (rows, size), off)
    got = out.cpu().numpy()[:, band_cols(YN, (0, YN))]
    e = T * numpy.arange(32)
    plain = numpy.concatenate([[0, M // 2, M, M + M // 2], e, e + M])
    centred = (plain + YN // 2) % YN
    tol = PEAK_BOUND * numpy.abs(want).max(axis=1)[:, None]
    err = numpy.abs(got[:, centred] - want[:, centred])
    print(f"RFFT64K self-mirrored outputs and lane 0: worst |err| / (row peak) {float((err / tol).max()) * PEAK_BOUND:.2e}")
    assert (err <= tol).all(), (plain[(err > tol).any(axis=0)], float((err / tol).max()))


@pytest.mark.parametrize("position", [20000, 20001], ids=["even", "odd"])
def test_impulse_rows(position):
    """a row that is one impulse: every output has the modulus window * scale and the oracle's phase (an E / O or sign
    mix-up moves the phase ramp or the modulus of half the outputs, which an RMSE over random rows can hide)"""
    from ska_sdp_exec_swiftly_amd import _lib

    core, ref = cores("c16")
    size, off = 45056, 0
    x = numpy.zeros((1, size), dtype=numpy.float32)
    x[0, position] = 1.0
    rc, _, out = _call(core, _device_rows(x), size, off, (0, YN))
    assert rc == 0, _lib.last_error()
    want = ref.prepare_facet(x.astype(complex), off, 1)
    got = out.cpu().numpy()[:, band_cols(YN, (0, YN))]
    modulus = ref.facet_window(size)[position] / YN
    assert numpy.allclose(numpy.abs(want), modulus, rtol=1e-9, atol=0)
    print(f"RFFT64K impulse at {position}: modulus off by {float(numpy.abs(numpy.abs(got) - modulus).max() / modulus):.2e}, "
          f"value by {float(numpy.abs(got - want).max() / modulus):.2e} of the modulus")
    assert numpy.abs(numpy.abs(got) - modulus).max() <= PEAK_BOUND * modulus
    assert numpy.abs(got - want).max() <= PEAK_BOUND * modulus


def test_nan_gap_between_the_rows():
    """a view with an even pitch larger than the facet whose gap holds NaN, on a base that is 8-byte but not 16-byte aligned:
    nothing outside the rows is read into the result"""
    _check(45056, 45056, PLAN_BAND, rows=7, pitch=45056 + 66, base=2, fill=float("nan"))


def test_refusals_write_nothing():
    """odd facet size, odd position, odd pitch, a 4-byte-aligned base, complex128 and a 16384-point core: ERR_UNSUPPORTED
    with the prefix, the output keeps its sentinel, no other kernel runs"""
    from ska_sdp_exec_swiftly_amd import _lib

    core, _ = cores("c16")
    small, _ = cores("c14")
    x = _x(7, 45056)
    cases = {
        "odd facet size": (core, _device_rows(x[:, :45055], 45056), 45055, 1, None),
        "odd offset": (core, _device_rows(x), 45056, 45057, None),
        "odd pitch": (core, _device_rows(x, 45056 + 3), 45056, 0, None),
        "4-byte base": (core, _device_rows(x, 45056 + 4, 1), 45056, 0, None),
        "complex128": (core, _device_rows(x), 45056, 0, _lib.C128),
        "16384-point core": (small, _device_rows(x[:, :11264].copy()), 11264, 0, None),
    }
    before, _ = last_instance()
    for name, (c, src, size, off, dtype) in cases.items():
        band = (0, c.yN_size)
        for rows_entry in (False, True):
            rc, frame, _ = _call(c, src, size, off, band, dtype=dtype, rows_entry=rows_entry)
            assert rc == _lib.ERR_UNSUPPORTED, (name, rc, _lib.last_error())
            assert PREFIX in _lib.last_error(), (name, _lib.last_error())
            assert bool((frame == SENTINEL).all()), name
    assert last_instance()[0] == before
    # through the Python layer: the library's NotImplementedError; a complex facet is an argument error
    import torch

    with pytest.raises(NotImplementedError, match=PREFIX):
        core.prepare_facet_band(_device_rows(x, 45056 + 3), 0, PLAN_BAND, half_length=True)
    with pytest.raises(ValueError):
        core.prepare_facet_band(_device_rows(x).to(torch.complex64), 0, PLAN_BAND, half_length=True)
    assert core.supports_real_facets_rfft() and not small.supports_real_facets_rfft()
    with pytest.raises(NotImplementedError, match=PREFIX):
        small.prepare_facet_band(_device_rows(x[:, :11264].copy()), 0, (0, 16384), half_length=True)


def test_python_door_matches_the_oracle():
    """``prepare_facet_band(..., half_length=True)`` and ``rows_of``: against the oracle, as the entry points"""
    import torch

    core, ref = cores("c16")
    x = _x(7, 45056)
    src = _device_rows(x)
    pc = band_cols(YN, PLAN_BAND)
    keep = pc >= 0
    want = _oracle(x, (7, 45056), 0)
    got = core.prepare_facet_band(src, 0, PLAN_BAND, half_length=True)
    assert got.dtype == torch.complex64
    assert relrms(got.cpu().numpy()[:, pc[keep]], (want * ref.facet_window(7)[:, None])[:, keep]) < BOUND
    got = core.prepare_facet_band(src, 0, PLAN_BAND, rows_of=(704, 100), half_length=True)
    assert relrms(got.cpu().numpy()[:, pc[keep]], (want * ref.facet_window(704)[100:107, None])[:, keep]) < BOUND


# -- the whole pass ---------------------------------------------------------------------------------------------------
#: the 128k workload's parameters (BASELINE configuration 5) with 352-pixel facets
P128 = dict(W=10.875, fov=1.0, N=131072, yB_size=352, yN_size=YN, xA_size=928, xM_size=1024)


def _real_problem(seed):
    """the small-rows problem of test_hip_band_pipeline_gpu.py on the 128k parameters, with REAL separable facets:
    Re(a (x) b) as the rank-4 sum Re a (x) Re b - Im a (x) Im b of real vectors, which the separable oracle takes as they are"""
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    yB, xA = P128["yB_size"], P128["xA_size"]
    cfg = sw.SwiftlyConfig(backend="hip", **P128)
    fstep = cfg.facet_off_step
    facet_cfgs = [sw.FacetConfig(o0, o1, yB) for o0, o1 in ((0, 0), (0, 50 * fstep), (-70 * fstep, 0))]
    sg_cfgs = [sw.SubgridConfig(i0 * xA, i1 * xA, xA) for i0 in (0, 2, 69) for i1 in (0, 3, 4, 70)]
    vectors = []
    for j in range(len(facet_cfgs)):
        a, b = sep.facet_vectors(seed + j, yB, rank=2)
        vectors.append((numpy.concatenate([a.real, -a.imag]).astype(complex), numpy.concatenate([b.real, b.imag]).astype(complex)))
    facets = [bench.separable_facet(torch, v, c) for v, c in zip(vectors, facet_cfgs)]
    assert all(float(f.imag.abs().max()) == 0 for f in facets)
    reals = [f.real.contiguous() for f in facets]
    ordered = sorted(sg_cfgs, key=lambda c: (c.off1, c.off0))
    return torch, sw, cfg, facet_cfgs, vectors, reals, sg_cfgs, ordered


def _run(sw, cfg, facet_cfgs, data, sg_cfgs, ordered, **kw):
    fwd = sw.SwiftlyForward(cfg, list(zip(facet_cfgs, data)), subgrid_configs=sg_cfgs, **kw)
    return fwd, fwd.get_subgrid_tasks(ordered)


def test_forward_half_length_k1():
    torch, sw, cfg, facet_cfgs, vectors, reals, sg_cfgs, ordered = _real_problem(47)
    # without the keyword nothing changes: float32 facets give the subgrids of the promoted ones, bit for bit, as before
    _, today = _run(sw, cfg, facet_cfgs, [r.to(torch.complex64) for r in reals], sg_cfgs, ordered, wave_axis=1)
    for kw in ({}, dict(facet_dtype=torch.float32), dict(facet_dtype=torch.float32, half_length_k1=False)):
        fwd, got = _run(sw, cfg, facet_cfgs, reals, sg_cfgs, ordered, **kw)
        assert fwd.half_length_k1 is False and fwd.facet_dtype == torch.float32
        assert all(torch.equal(g, t) for g, t in zip(got, today)), kw
    # with it: the half-length K1, float32 facets, every subgrid within the whole-pass bound of the separable oracle
    before, _ = last_instance()
    fwd, got = _run(sw, cfg, facet_cfgs, reals, sg_cfgs, ordered, facet_dtype=torch.float32, half_length_k1=True)
    assert fwd.half_length_k1 is True and fwd.facet_dtype == torch.float32 and fwd.wave_axis == 1
    assert last_instance()[0] == before, "K1 went through the band row kernel"
    ref = orc.OracleCore(P128["W"], P128["N"], P128["xM_size"], P128["yN_size"])
    so = sep.SeparableOracle(ref, [orc.CoverItem(c.off0, c.off1, c.size) for c in facet_cfgs], vectors)
    assert len(got) == len(ordered) == 12
    worst = 0.0
    for g, c in zip(got, ordered):
        assert g.dtype == torch.complex64
        worst = max(worst, relrms(g.cpu().numpy(), so.subgrid(orc.CoverItem(c.off0, c.off1, c.size))))
    print(f"RFFT64K whole pass: worst subgrid relative RMSE {worst:.3e}")
    assert worst < 2e-5, worst
    assert not all(torch.equal(g, t) for g, t in zip(got, today)), "the half-length form rounds differently: did it run?"
