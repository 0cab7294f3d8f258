"""
Float64 facets kept real through the complex128 band passes ("K1 on float64 facets", and section 7):
``swiftly_hip_prepare_facet_band_real64`` / ``swiftly_hip_finish_facet_band_real64``, their doors on ``SwiftlyCoreHip``, and
``SwiftlyForward(..., facet_dtype=torch.float64)`` / ``SwiftlyBackward(..., dtype=torch.complex128, facet_dtype=torch.float64)``.

Two kinds of expectation, both asserted for every case:

* the VALUE CONTRACT of include/swiftly_hip.h: the float64 forms give, bit for bit, what the complex128 entry points give for
  the promoted facet (K1) / the real part of what they store (finish) -- ``torch.equal``, no instance exempt;
* the 1-D oracle (oracle/swiftly_oracle.py) in complex128: ``max|err| <= 5e-12 * max|want|`` for single entry points
  (``C128_TOL`` of the complex128 modules), relative RMSE ``<= 1e-10`` against oracle/separable.py for whole passes.

Cores: those of the facet sweep (``N = 2 * 2^L``, ``xM`` 256, ``m`` 128) at L = 9 (the smallest single-workgroup double row of
these cores), 13 (the largest), 14 and 15 (both long-row lengths: pass A loads the reals, pass B stores them), 3 rows per call
(no multiple of any row block); whole passes on the SMALL full cover and on ``64k[1]-n16k-1k``.

The peak-memory bounds (``yB^2 * 8`` bytes less than the promoted / complex run) follow from 8 against 16 bytes per resident
pixel; they are not measurements.

Every case prints its figure (``REALF64 ...`` lines, ``pytest -s``).
"""
import gc
import os
import subprocess
import sys

import numpy
import pytest

import bench
import test_hip_c128_backward_band_gpu as bwd128
import test_hip_c128_band_pipeline_gpu as fwd128
import test_hip_facet_sweep_gpu as fs
from oracle import separable as sep

pytestmark = pytest.mark.gpu

C128_TOL = fwd128.C128_TOL  # 5e-12: max|err| / max|want|, single entry points
PASS_TOL = fwd128.PASS_TOL  # 1e-10: relative RMSE of whole passes against the separable oracle
SMALL = fwd128.SMALL
LENGTHS = [9, 13, 14, 15]
ROWS = 3
PAD = 5  # extra columns of the padded input / output rows
SENTINEL = fs.SENTINEL
SENTINEL_R = -7.25
IN_PREFIX, OUT_PREFIX = "real facets, float64: ", "real facet output, float64: "


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    import torch

    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def maxrel(got, want):
    assert got.shape == want.shape and numpy.isfinite(got).all(), (got.shape, want.shape)
    return float(numpy.max(numpy.abs(got - want)) / numpy.max(numpy.abs(want)))


def padded_rows(x):
    """the float64 rows ``x`` on the device inside a wider buffer (pitch ``yB + PAD``) whose padding is NaN: a load past a row
    would show in the result"""
    import torch

    buf = torch.full((x.shape[0], x.shape[1] + PAD), float("nan"), dtype=torch.float64, device="cuda")
    view = buf[:, : x.shape[1]]
    view.copy_(torch.from_numpy(x))
    assert view.stride(0) == x.shape[1] + PAD and view.stride(1) == 1
    return view


def framed(rows, cols, dtype, sentinel):
    """an output view ``[rows, cols]`` with sentinels above, below, left and right of it; ``(view, buffer, intact())``"""
    import torch

    buf = torch.full((rows + 2, cols + 2 * PAD), sentinel, dtype=dtype, device="cuda")
    view = buf[1 : rows + 1, PAD : PAD + cols]

    def intact():
        frame = buf.clone()
        frame[1 : rows + 1, PAD : PAD + cols] = sentinel
        return bool((frame == sentinel).all())

    return view, buf, intact


# ------------------------------------------------------------------------------------------------------------------ K1
def k1_case(core, ref, x, xin, promoted, off, fold, note):
    import torch

    yN = core.yN_size
    rows = x.shape[0]
    out, _, intact = framed(rows, yN, torch.complex128, SENTINEL)
    res = core.prepare_facet_band_float64(xin, off, (0, yN), out=out, fold_other_axis_window=fold)
    assert res is out
    assert intact(), "prepare_facet_band_float64 wrote outside the rows and columns of `out`"
    twin = core.prepare_facet_band(promoted, off, (0, yN), fold_other_axis_window=fold)
    assert twin.dtype == torch.complex128
    assert torch.equal(out, twin), f"float64 K1 differs from the complex128 K1 of the promoted facet ({note})"
    want = ref.prepare_facet(x.astype(complex), off, 1)
    if fold:
        want = want * ref.facet_window(rows)[:, None]
    err = maxrel(out.cpu().numpy(), want)
    print(f"REALF64 prepare_facet_band_float64 {note:<34s} {err:.3e} (bound {C128_TOL:.1e})")
    assert err <= C128_TOL, (note, err)
    # without an `out`: a fresh complex128 tensor with the same values
    if not fold:
        fresh = core.prepare_facet_band_float64(xin, off, (0, yN), fold_other_axis_window=False)
        assert fresh.dtype == torch.complex128 and tuple(fresh.shape) == (rows, yN) and torch.equal(fresh, twin)


@pytest.mark.parametrize("L", LENGTHS)
def test_prepare_facet_band_float64_lengths(L):
    """the float64-load K1: one workgroup per row at 512 and 8192 points, pass A of the long rows at 16384 and 32768; offsets
    0, a positive multiple of the subgrid step and ``-yB``; with and without the folded window of the other axis"""
    import torch

    core, ref = fs.cores(fs.params(L))
    assert core.supports_real_facets_f64() and core.supports_band_pipeline(torch.complex128, explicit=True)
    yB = fs.facet_size(L)
    step = core.N // core.xM_size
    rng = numpy.random.default_rng(6100 + L)
    x = rng.standard_normal((ROWS, yB))
    assert (x.astype(numpy.float32) != x).any()  # values float32 cannot hold
    xin = padded_rows(x)
    promoted = torch.from_numpy(x).cuda().to(torch.complex128)
    for io, off in enumerate((0, 37 * step, -yB)):
        for fold in (False, True):
            k1_case(core, ref, x, xin, promoted, off, fold, f"L {L} off {io} fold {int(fold)}")


_CHUNK_CHILD = r"""
import sys, numpy, torch
sys.path[:0] = [sys.argv[2] + "/tests", sys.argv[2], sys.argv[3]]
import test_hip_facet_sweep_gpu as fs
import test_hip_real_f64_gpu as t
L, rows = 14, int(sys.argv[4])
core, ref = fs.cores(fs.params(L))
yN, yB = core.yN_size, fs.facet_size(L)
x = numpy.random.default_rng(6200).standard_normal((rows, yB))
xin = t.padded_rows(x)
off = 37 * (core.N // core.xM_size)
out, _, intact = t.framed(rows, yN, torch.complex128, t.SENTINEL)
core.prepare_facet_band_float64(xin, off, (0, yN), out=out, fold_other_axis_window=True)
assert intact()
twin = core.prepare_facet_band(torch.from_numpy(x).cuda().to(torch.complex128), off, (0, yN), fold_other_axis_window=True)
assert torch.equal(out, twin)
want = ref.prepare_facet(x.astype(complex), off, 1) * ref.facet_window(rows)[:, None]
err = t.maxrel(out.cpu().numpy(), want)
assert err <= t.C128_TOL, err
numpy.save(sys.argv[1], out.cpu().numpy())
print("REALF64 chunked K1", err)
"""


def test_prepare_facet_band_float64_more_rows_than_one_scratch_chunk(tmp_path):
    """L = 14, 9 rows with ``SWIFTLY_LONG_ROWS_CHUNK_MB=1`` (4 rows of 16384 complex128 points per scratch chunk: chunks of
    4, 4 and 1 rows -- pass A's ``row0`` and the real row pitch) in a child process: bit-equal to the promoted K1 there, within
    the oracle bound, and bit-equal to the one-chunk result of this process"""
    import torch

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "ska-sdp-distributed-fourier-transform_amd")
    rows = 9
    path = str(tmp_path / "chunked.npy")
    env = dict(os.environ, SWIFTLY_LONG_ROWS_CHUNK_MB="1")
    res = subprocess.run([sys.executable, "-c", _CHUNK_CHILD, path, root, pkg, str(rows)], env=env, cwd=root, timeout=300,
                         capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-3000:])
    print(res.stdout.strip().splitlines()[-1])
    chunked = numpy.load(path)
    assert "SWIFTLY_LONG_ROWS_CHUNK_MB" not in os.environ
    core, _ = fs.cores(fs.params(14))
    x = numpy.random.default_rng(6200).standard_normal((rows, fs.facet_size(14)))
    one = core.prepare_facet_band_float64(padded_rows(x), 37 * (core.N // core.xM_size), (0, core.yN_size))
    assert one.dtype == torch.complex128 and numpy.array_equal(one.cpu().numpy(), chunked)


# -------------------------------------------------------------------------------------------------------------- finish
def finish_cases(L, yN, yB):
    """the bands and offsets of ``test_finish_facet_band_c128_lengths``: interior, wrapping, full (and, at L = 15, a band of
    15000 columns from an odd start)"""
    cases = [((yN // 2 - 5 * yN // 32, 11 * yN // 32 + 8), 0), ((yN - 3 * yN // 32, 7 * yN // 32 + 1), yB), ((0, yN), -yB)]
    if L == 15:
        cases.append(((yN // 4 + 1, 15000), 3 * 352))
    assert cases[1][0][0] + cases[1][0][1] > yN
    return cases


@pytest.mark.parametrize("L", LENGTHS)
def test_finish_facet_band_float64_lengths(L):
    """the float64-store finish: one workgroup per row at 512 and 8192 points, pass B of the long rows (128 / 256 points
    behind n1 = 128) at 16384 and 32768; a partial mask; output rows at a pitch of ``yB + 5``"""
    import torch

    core, ref = fs.cores(fs.params(L))
    assert core.supports_real_facets_out_f64() and core.supports_backward_band(torch.complex128, explicit=True)
    yN, yB = core.yN_size, fs.facet_size(L)
    rng = numpy.random.default_rng(7100 + L)
    mask = (rng.random(yB) > 0.15).astype(float)
    assert 0 < mask.sum() < yB
    for k, (band, off) in enumerate(finish_cases(L, yN, yB)):
        start, length = band
        data = rng.standard_normal((ROWS, length)) + 1j * rng.standard_normal((ROWS, length))
        full = numpy.zeros((ROWS, yN), dtype=complex)
        full[:, (start + numpy.arange(length)) % yN] = data
        want = ref.finish_facet(full, off, yB, axis=1).real * mask[None, :]
        acc = torch.from_numpy(data).cuda()
        obuf = torch.full((ROWS + 1, yB + PAD), SENTINEL_R, dtype=torch.float64, device="cuda")
        out = obuf[:ROWS, :yB]
        res = core.finish_facet_band_float64(acc, band, off, yB, mask=mask, out=out)
        assert res is out and out.stride(0) == yB + PAD
        assert bool((obuf[ROWS] == SENTINEL_R).all()) and bool((obuf[:, yB:] == SENTINEL_R).all()), \
            "finish_facet_band_float64 wrote outside its rows"
        twin = core.finish_facet_band(acc, band, off, yB, mask=mask)
        assert twin.dtype == torch.complex128
        assert torch.equal(out, twin.real), f"float64 finish differs from the real part of the complex128 finish (L {L} band {k})"
        got = out.cpu().numpy()
        assert not got[:, mask == 0].any()  # masked pixels are exactly zero
        err = maxrel(got, want)
        print(f"REALF64 finish_facet_band_float64  L {L} band {k:<26d} {err:.3e} (bound {C128_TOL:.1e})")
        assert err <= C128_TOL, (L, k, err)
    # without an `out` and without a mask: a fresh float64 tensor
    fresh = core.finish_facet_band_float64(acc, band, off, yB)
    assert fresh.dtype == torch.float64 and tuple(fresh.shape) == (ROWS, yB)
    assert torch.equal(fresh, core.finish_facet_band(acc, band, off, yB).real)


# ------------------------------------------------------------------------------------------------------------ refusals
def _raw_k1(core, name, code, xin, out, band):
    import ctypes

    cvp = ctypes.c_void_p
    fn = getattr(core._lib, name)  # pylint: disable=protected-access
    return fn(core._handle, code, cvp(xin.data_ptr()), xin.shape[0], xin.shape[1], xin.stride(0), cvp(out.data_ptr()),  # pylint: disable=protected-access
              out.stride(0), 0, band[0], band[1], 0, core._stream())  # pylint: disable=protected-access


def _raw_finish(core, name, code, acc, out, band, yB, out_stride=None):
    import ctypes

    cvp = ctypes.c_void_p
    fn = getattr(core._lib, name)  # pylint: disable=protected-access
    return fn(core._handle, code, cvp(acc.data_ptr()), acc.shape[0], acc.stride(0), band[0], band[1], cvp(out.data_ptr()),  # pylint: disable=protected-access
              out.stride(0) if out_stride is None else out_stride, 0, yB, None, core._stream())  # pylint: disable=protected-access


def test_refusals_leave_the_output_untouched():
    import torch

    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip, _lib

    core, _ = fs.cores(fs.params(9))
    yN, yB = core.yN_size, fs.facet_size(9)
    xin = padded_rows(numpy.random.default_rng(1).standard_normal((ROWS, yB)))
    out, _, k1_intact = framed(ROWS, yN, torch.complex128, SENTINEL)
    out[:] = SENTINEL

    def k1_untouched():
        torch.cuda.synchronize()
        return k1_intact() and bool((out == SENTINEL).all())

    acc = torch.zeros((ROWS, yN), dtype=torch.complex128, device="cuda")
    rout = torch.full((ROWS, yB + PAD), SENTINEL_R, dtype=torch.float64, device="cuda")

    def finish_untouched():
        torch.cuda.synchronize()
        return bool((rout == SENTINEL_R).all())

    # SWIFTLY_C64 as dtype: both raw entry points refuse through the new rules
    assert _raw_k1(core, "swiftly_hip_prepare_facet_band_real64", _lib.C64, xin, out, (0, yN)) == _lib.ERR_UNSUPPORTED
    assert IN_PREFIX in _lib.last_error() and "8 / 9" in _lib.last_error(), _lib.last_error()
    assert k1_untouched()
    assert _raw_finish(core, "swiftly_hip_finish_facet_band_real64", _lib.C64, acc, rout, (0, yN), yB) == _lib.ERR_UNSUPPORTED
    assert OUT_PREFIX in _lib.last_error() and "8 / 9" in _lib.last_error(), _lib.last_error()
    assert finish_untouched()
    # a pruned band into K1: raw and through the door
    assert _raw_k1(core, "swiftly_hip_prepare_facet_band_real64", _lib.C128, xin, out, (0, yN // 2)) == _lib.ERR_UNSUPPORTED
    assert "whole padded axis" in _lib.last_error()
    pruned = torch.full((ROWS, core.band_columns((0, yN // 2))), SENTINEL, dtype=torch.complex128, device="cuda")
    with pytest.raises(NotImplementedError, match="whole padded axis"):
        core.prepare_facet_band_float64(xin, 0, (0, yN // 2), out=pruned)
    torch.cuda.synchronize()
    assert k1_untouched() and bool((pruned == SENTINEL).all())
    # out_row_stride < facet_size: raw and through the door (a view whose rows overlap)
    assert _raw_finish(core, "swiftly_hip_finish_facet_band_real64", _lib.C128, acc, rout, (0, yN), yB, yB - 1) == _lib.ERR_PARAM
    assert "out_row_stride" in _lib.last_error()
    overlapping = torch.as_strided(rout, (ROWS, yB), (yB - 1, 1))
    with pytest.raises(ValueError, match="out_row_stride"):
        core.finish_facet_band_float64(acc, (0, yN), 0, yB, out=overlapping)
    assert finish_untouched()
    # wrong dtypes and strides through the doors
    with pytest.raises(ValueError, match="float64"):
        core.prepare_facet_band_float64(xin.to(torch.float32), 0, (0, yN), out=out)
    with pytest.raises(ValueError, match="complex128"):
        core.prepare_facet_band_float64(xin, 0, (0, yN), out=torch.empty((ROWS, yN), dtype=torch.complex64, device="cuda"))
    with pytest.raises(ValueError, match="complex128"):
        core.finish_facet_band_float64(acc.to(torch.complex64), (0, yN), 0, yB, out=rout[:, :yB])
    with pytest.raises(ValueError, match="float64"):
        core.finish_facet_band_float64(acc, (0, yN), 0, yB, out=torch.empty((ROWS, yB), dtype=torch.float32, device="cuda"))
    assert k1_untouched() and finish_untouched()
    # the doors that existed before keep refusing: float64 into prepare_facet_band, complex128 into the float32 forms
    with pytest.raises(ValueError, match="float64"):
        core.prepare_facet_band(xin, 0, (0, yN))
    with pytest.raises(NotImplementedError, match="complex128"):
        core.finish_facet_band(acc, (0, yN), 0, yB, real=True, out=torch.empty((ROWS, yB), dtype=torch.float32, device="cuda"))
    for name in ("swiftly_hip_prepare_facet_band_real", "swiftly_hip_prepare_facet_band_rfft"):
        assert _raw_k1(core, name, _lib.C128, xin, out, (0, yN)) == _lib.ERR_UNSUPPORTED and "complex128" in _lib.last_error()
    for name in ("swiftly_hip_finish_facet_band_real", "swiftly_hip_finish_facet_band_c2r"):
        assert _raw_finish(core, name, _lib.C128, acc, rout, (0, yN), yB) == _lib.ERR_UNSUPPORTED and "complex128" in _lib.last_error()
    assert k1_untouched() and finish_untouched()
    # yN = 3 * 2^10: the complex128 passes have no radix-Q form, so neither have these
    core3 = SwiftlyCoreHip(fs.W, 6144, 256, 3 << 10)
    assert not core3.supports_real_facets_f64() and _lib.last_error().startswith(IN_PREFIX)
    assert not core3.supports_real_facets_out_f64() and _lib.last_error().startswith(OUT_PREFIX)
    yN3, yB3 = 3 << 10, 2112
    x3 = torch.zeros((ROWS, yB3), dtype=torch.float64, device="cuda")
    out3 = torch.full((ROWS, yN3), SENTINEL, dtype=torch.complex128, device="cuda")
    with pytest.raises(NotImplementedError, match=IN_PREFIX):
        core3.prepare_facet_band_float64(x3, 0, (0, yN3), out=out3)
    assert _raw_k1(core3, "swiftly_hip_prepare_facet_band_real64", _lib.C128, x3, out3, (0, yN3)) == _lib.ERR_UNSUPPORTED
    rout3 = torch.full((ROWS, yB3), SENTINEL_R, dtype=torch.float64, device="cuda")
    acc3 = torch.zeros((ROWS, yN3), dtype=torch.complex128, device="cuda")
    with pytest.raises(NotImplementedError, match=OUT_PREFIX):
        core3.finish_facet_band_float64(acc3, (0, yN3), 0, yB3, out=rout3)
    assert _raw_finish(core3, "swiftly_hip_finish_facet_band_real64", _lib.C128, acc3, rout3, (0, yN3), yB3) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out3 == SENTINEL).all()) and bool((rout3 == SENTINEL_R).all())


# ------------------------------------------------------------------------------------------------------- forward passes
def real_vectors(vec):
    """separable vectors with their imaginary parts dropped (still complex128 arrays: the oracle's type)"""
    a, b = vec
    return a.real + 0j, b.real + 0j


def real_facet(vec, cfg):
    """float64 device facet ``sum_r a_r (x) b_r`` times the cover masks, from real vectors"""
    import torch

    a, b = vec
    yB = cfg.size
    m0 = cfg.mask0 if cfg.mask0 is not None else numpy.ones(yB)
    m1 = cfg.mask1 if cfg.mask1 is not None else numpy.ones(yB)
    out = torch.zeros((yB, yB), dtype=torch.float64, device="cuda")
    for r in range(a.shape[0]):
        out.add_(torch.outer(torch.from_numpy(a[r].real * m0).cuda(), torch.from_numpy(b[r].real * m1).cuda()))
    return out


def forward(cfg, facet_cfgs, facets, plan, order, wave_axis, **kw):
    """``(subgrids as host arrays, facet_dtype, dtypes of the resident facets, did device facets stay in place)``"""
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    fwd = sw.SwiftlyForward(cfg, list(zip(facet_cfgs, facets)), subgrid_configs=plan, wave_axis=wave_axis, **kw)
    assert fwd.wave_axis == wave_axis and fwd.dtype == torch.complex128
    got = [t.cpu().numpy() for t in fwd.get_subgrid_tasks(order)]
    resident = fwd._ingest.tensors  # pylint: disable=protected-access
    in_place = all(not isinstance(f, torch.Tensor) or f.data_ptr() == t.data_ptr() for f, t in zip(facets, resident))
    return got, fwd.facet_dtype, {t.dtype for t in resident}, in_place


def test_forward_small_full_cover_float64():
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    p = SMALL
    cfg = sw.SwiftlyConfig(backend="hip", **p)
    facet_cfgs = sw.api.make_full_cover_config(p["N"], p["yB_size"], sw.FacetConfig)
    sg_cfgs = sw.api.make_full_cover_config(p["N"], p["xA_size"], sw.SubgridConfig)
    vectors = [real_vectors(sep.facet_vectors(700 + j, p["yB_size"], rank=2)) for j in range(len(facet_cfgs))]
    reals = [real_facet(v, c) for v, c in zip(vectors, facet_cfgs)]
    promoted = [f.to(torch.complex128) for f in reals]
    n = len(facet_cfgs)
    assert cfg.core.supports_band_pipeline(torch.complex128, n, explicit=True) and cfg.core.supports_real_facets_f64()
    order = sorted(sg_cfgs, key=lambda c: (c.off1, c.off0))
    want, dt, resident, _ = forward(cfg, facet_cfgs, promoted, sg_cfgs, order, 1)
    assert dt == torch.complex128 and resident == {torch.complex128}
    # device tensors: float64 resident, in place, the subgrids of the promoted run bit for bit
    got, dt, resident, in_place = forward(cfg, facet_cfgs, reals, sg_cfgs, order, 1, facet_dtype=torch.float64)
    assert dt == torch.float64 and resident == {torch.float64} and in_place
    assert all(g.dtype == numpy.complex128 and numpy.array_equal(g, w) for g, w in zip(got, want))
    par = bench.verify_subgrids(p, facet_cfgs, vectors, order, dict(enumerate(got)), tol=PASS_TOL)
    print(f"REALF64 forward SMALL full cover, float64 facets: relRMSE {par['rel_rmse']:.3e} (bound {PASS_TOL:.1e})")
    assert par["rel_rmse"] <= PASS_TOL, par
    # host arrays through the staging ring: uploaded as float64
    host = [f.cpu().numpy() for f in reals]
    assert all(h.dtype == numpy.float64 for h in host)
    got, dt, resident, _ = forward(cfg, facet_cfgs, host, sg_cfgs, order, 1, facet_dtype="float64")
    assert dt == torch.float64 and resident == {torch.float64}
    assert all(numpy.array_equal(g, w) for g, w in zip(got, want))
    # without the keyword float64 facets are promoted as ever (device and host)
    for data in (reals, host):
        got, dt, resident, _ = forward(cfg, facet_cfgs, data, sg_cfgs, order, 1)
        assert dt == torch.complex128 and resident == {torch.complex128}
        assert all(numpy.array_equal(g, w) for g, w in zip(got, want))
    # wave_axis=0 has no float64 K1: promoted with the keyword too, and the results are those of the promoted facets
    want0, _, _, _ = forward(cfg, facet_cfgs, promoted, sg_cfgs, order, 0)
    got, dt, resident, _ = forward(cfg, facet_cfgs, reals, sg_cfgs, order, 0, facet_dtype=torch.float64)
    assert dt == torch.complex128 and resident == {torch.complex128}
    assert all(numpy.array_equal(g, w) for g, w in zip(got, want0))
    # the keyword is a statement about the data: float32 or complex facets with it are refused at construction
    for bad in ([f.to(torch.float32) for f in reals], promoted, reals[:1] + promoted[1:]):
        with pytest.raises(ValueError, match="facet_dtype"):
            sw.SwiftlyForward(cfg, list(zip(facet_cfgs, bad)), subgrid_configs=sg_cfgs, wave_axis=1, facet_dtype=torch.float64)
    with pytest.raises(ValueError, match="half_length_k1=True needs facet_dtype=float32"):
        sw.SwiftlyForward(cfg, list(zip(facet_cfgs, reals)), wave_axis=1, facet_dtype=torch.float64, half_length_k1=True)


def test_forward_64k_n16k_1k_float64_peak_memory():
    """the first facet and three subgrids of ``_large_problem`` (one long-row K1 in a real pass): the subgrids of the promoted
    run bit for bit, within the oracle bound, and a peak lower by at least ``yB^2 * 8`` bytes"""
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    p, facet_cfgs, vectors, sg_cfgs = fwd128._large_problem("64k[1]-n16k-1k", 3)  # pylint: disable=protected-access
    facet_cfgs, vectors = facet_cfgs[:1], [real_vectors(vectors[0])]
    yB = p["yB_size"]
    cfg = sw.SwiftlyConfig(backend="hip", **p)
    assert cfg.core.supports_band_pipeline(torch.complex128, 1, explicit=True) and cfg.core.supports_real_facets_f64()
    order = sorted(sg_cfgs, key=lambda c: (c.off1, c.off0))

    def measured(facets, **kw):
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        got, dt, resident, _ = forward(cfg, facet_cfgs, facets, sg_cfgs, order, 1, **kw)
        torch.cuda.synchronize()
        return got, dt, resident, torch.cuda.max_memory_allocated()

    real = real_facet(vectors[0], facet_cfgs[0])
    got, dt, resident, peak_real = measured([real], facet_dtype=torch.float64)
    assert dt == torch.float64 and resident == {torch.float64}
    promoted = real.to(torch.complex128)
    del real
    want, dt, resident, peak_promoted = measured([promoted])
    assert dt == torch.complex128 and resident == {torch.complex128}
    del promoted
    assert all(g.dtype == numpy.complex128 and numpy.array_equal(g, w) for g, w in zip(got, want))
    par = bench.verify_subgrids(p, facet_cfgs, vectors, order, dict(enumerate(got)), tol=PASS_TOL)
    print(f"REALF64 forward 64k[1]-n16k-1k, one float64 facet: relRMSE {par['rel_rmse']:.3e} (bound {PASS_TOL:.1e}); peak "
          f"{peak_real / 2**30:.3f} GiB against {peak_promoted / 2**30:.3f} GiB promoted (yB^2 * 8 = {yB * yB * 8 / 2**30:.3f} GiB)")
    assert par["rel_rmse"] <= PASS_TOL, par
    assert peak_promoted - peak_real >= yB * yB * 8, (peak_promoted, peak_real)


# ------------------------------------------------------------------------------------------------------ backward passes
def test_backward_small_float64():
    """the small full-cover problem of the complex128 backward module: float64 facets straight from the row kernels"""
    import torch

    P = bwd128.small_problem()
    sw, cfg, sg, data, by1 = P["sw"], P["cfg"], P["sg_cfgs"], P["data"], P["by1"]
    assert cfg.core.supports_real_facets_out_f64()
    complex_run = bwd128.whole_waves_result(P)
    bwd = bwd128.band_backward(P, subgrid_configs=sg, facet_dtype=torch.float64)
    assert bwd.real_finish_native is True and bwd.facet_dtype == torch.float64 and bwd.half_length_finish is False
    calls = []
    inner = cfg.core.finish_facet_band_float64
    cfg.core.finish_facet_band_float64 = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    try:
        bwd.add_new_subgrid_tasks([sg[i] for i in by1], [data[i] for i in by1])
        assert bwd.bands.bands.dtype == torch.complex128
        out = bwd.finish()
    finally:
        del cfg.core.finish_facet_band_float64
    assert len(calls) == len(P["facet_cfgs"])  # every facet through the float64 store
    assert all(t.dtype == torch.float64 and tuple(t.shape) == (SMALL["yB_size"],) * 2 for t in out)
    got = numpy.array([t.cpu().numpy() for t in out])
    assert numpy.array_equal(got, complex_run.real), "float64 facets differ from the real parts of the complex128 run"
    # the bound of that module (``pass_rule``), with the error of the real parts over the norm it uses: the oracle's
    # imaginary parts stand in for the ones this pass does not return, so the figure is at most the complex run's
    bwd128.pass_rule("float64 facets, off1-major waves", got + 1j * P["want"].imag, P["want"], P["e_ref"])
    # complex64 data with float64 facets: refused at the first data
    xA = SMALL["xA_size"]
    other = sw.SwiftlyBackward(cfg, P["facet_cfgs"], wave_axis=1, facet_dtype=torch.float64)
    with pytest.raises(ValueError, match="does not match"):
        other.wave_contributions([sg[0]], [torch.zeros((xA, xA), dtype=torch.complex64, device="cuda")])


def test_backward_small_float64_wave_axis_0():
    import torch

    P = bwd128.small_problem()
    sw, cfg, facet_cfgs, sg, data = P["sw"], P["cfg"], P["facet_cfgs"], P["sg_cfgs"], P["data"]
    runs = {}
    for name, kw in (("complex", {}), ("float64", dict(facet_dtype=torch.float64))):
        bwd = sw.SwiftlyBackward(cfg, facet_cfgs, wave_axis=0, dtype=torch.complex128, **kw)
        assert bwd.real_finish_native is False
        bwd.add_new_subgrid_tasks(sg, data)
        runs[name] = bwd.finish()
    assert all(t.dtype == torch.float64 for t in runs["float64"]) and all(t.dtype == torch.complex128 for t in runs["complex"])
    assert all(torch.equal(r, c.real) for r, c in zip(runs["float64"], runs["complex"]))


def test_backward_64k_n16k_1k_float64_peak_memory():
    """one facet of ``64k[1]-n16k-1k``, four subgrids in two waves (the long-row finish): ``finish()`` returns the real part
    of the complex128 run bit for bit and peaks at least ``yB^2 * 8`` bytes lower -- no complex128 facet is allocated"""
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    p, facet_cfgs, _, _ = fwd128._large_problem("64k[1]-n16k-1k", 2)  # pylint: disable=protected-access
    facet_cfgs = facet_cfgs[:1]
    xA, yB = p["xA_size"], p["yB_size"]
    sg_cfgs = [sw.SubgridConfig(o0, o1, xA) for o0, o1 in ((0, 0), (3 * xA, 0), (10 * xA, xA), (-7 * xA, xA))]
    data = [bwd128.subgrid128(sep.subgrid_vectors(1500 + i, xA, rank=2), c) for i, c in enumerate(sg_cfgs)]
    cfg = sw.SwiftlyConfig(backend="hip", **p)
    assert cfg.core.supports_real_facets_out_f64()

    def finished(**kw):
        bwd = sw.SwiftlyBackward(cfg, facet_cfgs, wave_axis=1, subgrid_configs=sg_cfgs, dtype=torch.complex128, **kw)
        bwd.add_new_subgrid_tasks(sg_cfgs, data)
        native = bwd.real_finish_native
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        out = bwd.finish()
        torch.cuda.synchronize()
        return out[0], native, torch.cuda.max_memory_allocated()

    real, native, peak_real = finished(facet_dtype=torch.float64)
    assert native is True and real.dtype == torch.float64 and tuple(real.shape) == (yB, yB)
    real = real.cpu()
    cplx, native, peak_complex = finished()
    assert native is False and cplx.dtype == torch.complex128
    assert torch.equal(real, cplx.real.cpu())
    print(f"REALF64 backward 64k[1]-n16k-1k finish(): peak {peak_real / 2**30:.3f} GiB against {peak_complex / 2**30:.3f} GiB "
          f"complex (yB^2 * 8 = {yB * yB * 8 / 2**30:.3f} GiB)")
    assert peak_complex - peak_real >= yB * yB * 8, (peak_complex, peak_real)
