"""
GPU tests of ``DeviceSources`` on real-valued images (``swiftly_hip_facet_from_sources_real`` /
``swiftly_hip_check_facet_from_sources_real``, csrc/swiftly_sources.h): facets built as float32 / float64 and facets checked
without ever being complex.

The problem is the ``n1024`` case of tests/test_hip_sources_gpu.py with the real parts of its intensities, on 64-pixel
facets; because 37 random sources leave such facets almost empty, every facet also gets sources of its own (its first and
last pixel among them).  Every expectation is the complex twin on the same table: the real store is the real part of the
complex store (one rounding of the same float64 product), and the real check adds, in the complex check's order, the same
squares minus exact zeros -- so both comparisons are ``torch.equal``.  The figures themselves are held to a formula of this
file: the RMS of the float64 difference to the device truth, whose sum of 4096 squares in another order agrees to
``4096 * 2^-52 < 1e-12`` relative (bound used: 1e-10).
"""
import functools

import numpy
import pytest

from test_hip_sources_gpu import case, holes

pytestmark = pytest.mark.gpu

N, SIZE = 1024, 64
#: (off0, off1, masked): the centre, a masked facet, one that wraps around the edge of the image on both axes
FACETS = [(0, 0, False), (64, -128, True), (500, -500, False)]


@functools.lru_cache(maxsize=None)
def real_sources():
    out = [(float(numpy.real(i)), c0, c1) for i, c0, c1 in case("n1024")[2]]
    rng = numpy.random.default_rng(77)
    for off0, off1, _ in FACETS:
        lo0, lo1 = off0 - SIZE // 2, off1 - SIZE // 2
        pixels = {(0, 0), (SIZE - 1, SIZE - 1), (0, SIZE - 1), (17, 17), (17, 18), (17, 40)}
        while len(pixels) < 20:
            pixels.add(tuple(int(v) for v in rng.integers(0, SIZE, size=2)))
        out += [(float(rng.standard_normal()), lo0 + p0, lo1 + p1) for p0, p1 in sorted(pixels)]
    return out


def facet_configs(masked=None):
    import ska_sdp_exec_swiftly_amd as sw

    return [sw.FacetConfig(o0, o1, SIZE, holes(SIZE, 31) if m else None, holes(SIZE, 32) if m else None)
            for o0, o1, m in FACETS if masked is None or m == masked]


@functools.lru_cache(maxsize=None)
def device_sources():
    import ska_sdp_exec_swiftly_amd as sw

    return sw.DeviceSources(real_sources(), N)


@functools.lru_cache(maxsize=None)
def truths():
    """complex128 device facets of FACETS, computed once and left unchanged"""
    out = [device_sources().facet(cfg) for cfg in facet_configs()]
    assert all(int((t != 0).sum()) >= 5 for t in out) and all(float(t.imag.abs().max()) == 0 for t in out)
    return out


@pytest.mark.parametrize("masked", [False, True])
def test_real_facet_is_the_real_part_of_the_complex_facet(masked):
    import torch

    dsrc = device_sources()
    for cfg in facet_configs(masked):
        for real, cplx in ((torch.float32, torch.complex64), (torch.float64, torch.complex128)):
            want = dsrc.facet(cfg, dtype=cplx)
            got = dsrc.facet(cfg, dtype=real)
            assert got.dtype == real and tuple(got.shape) == (SIZE, SIZE) and got.is_contiguous()
            assert int((want != 0).sum()) >= 5
            assert torch.equal(got, want.real)
        # numpy names of the dtype; a dirty caller's view with a larger row stride: zeroed first, the gap keeps its sentinel
        assert torch.equal(dsrc.facet(cfg, dtype="float32"), dsrc.facet(cfg, dtype=torch.complex64).real)
        wide = torch.full((SIZE, SIZE + 5), 7.0, dtype=torch.float32, device=dsrc.device)
        ret = dsrc.facet(cfg, out=wide[:, :SIZE])
        assert ret.data_ptr() == wide.data_ptr() and ret.dtype == torch.float32
        assert torch.equal(wide[:, :SIZE], dsrc.facet(cfg, dtype=torch.complex64).real)
        assert bool((wide[:, SIZE:] == 7.0).all())


def test_a_complex_intensity_is_refused_and_nothing_is_written():
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    cfg = facet_configs()[0]
    sources = real_sources()
    dsrc = sw.DeviceSources(sources[:5] + [(1.0 + 0.25j, 3, 4)] + sources[5:], N)
    out = torch.full((SIZE, SIZE), 7.0, dtype=torch.float32, device=dsrc.device)
    for kw in (dict(out=out), dict(dtype=torch.float32), dict(dtype=torch.float64)):
        with pytest.raises(ValueError, match="imaginary"):
            dsrc.facet(cfg, **kw)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert dsrc.facet(cfg, dtype=torch.complex64)[SIZE // 2 + 3, SIZE // 2 + 4] == 1.0 + 0.25j  # the complex form takes it
    # imaginary parts that cancel on one pixel leave a real table
    both = sw.DeviceSources([(1.0 + 2j, 3, 4), (0.5 - 2j, 3, 4)], N)
    assert float(both.facet(cfg, dtype=torch.float32)[SIZE // 2 + 3, SIZE // 2 + 4]) == 1.5


def _noisy(dtype, rel=1e-3, seed=5):
    """truth + noise of about ``rel`` of the brightest pixel, rounded to ``dtype``: shared inputs, one per facet"""
    import torch

    gen = torch.Generator(device="cpu").manual_seed(seed)
    out = []
    for t in truths():
        noise = torch.randn((SIZE, SIZE), dtype=torch.float64, generator=gen).to(t.device) * (rel * float(t.real.abs().max()))
        out.append((t.real + noise).to(dtype))
    return out


@pytest.mark.parametrize("real,cplx", [("float32", "complex64"), ("float64", "complex128")])
def test_check_facets_on_reals_gives_the_bits_of_the_promoted_facets(real, cplx):
    import torch

    dsrc, cfgs = device_sources(), facet_configs()
    approx = _noisy(getattr(torch, real))
    got = dsrc.check_facets(cfgs, approx)
    assert isinstance(got, torch.Tensor) and got.device == dsrc.device
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(cfgs), 2)
    promoted = [a.to(getattr(torch, cplx)) for a in approx]
    assert torch.equal(got, dsrc.check_facets(cfgs, promoted))
    assert torch.equal(got, dsrc.check_facets(cfgs, approx))  # fixed-order sums: the same bits again
    # the figures: RMS of the difference to the (masked) truth and RMS of the truth, from this file's formula
    for k, (cfg, a, t) in enumerate(zip(cfgs, approx, truths())):
        want = float((a.to(torch.float64) - t.real).pow(2).mean().sqrt())
        rms = float(t.real.pow(2).mean().sqrt())
        print(f"check_facets {real} facet {k}: RMSE {float(got[k, 0]):.6e} (formula {want:.6e}), truth RMS {float(got[k, 1]):.6e}")
        assert want > 0 and abs(float(got[k, 0]) - want) <= 1e-10 * want
        assert abs(float(got[k, 1]) - rms) <= 1e-10 * rms
    # a mixed list, and views with a larger row stride read in place (NaN in the gap)
    mixed = [approx[0], promoted[1], approx[2]]
    assert torch.equal(dsrc.check_facets(cfgs, mixed), got)
    wide = torch.full((len(cfgs), SIZE + 2, SIZE + 3), float("nan"), dtype=approx[0].dtype, device=dsrc.device)
    views = [wide[k, 1 : 1 + SIZE, 2 : 2 + SIZE] for k in range(len(cfgs))]
    for v, a in zip(views, approx):
        v.copy_(a)
    assert dsrc._approx(views[1], 2, real_ok=True).data_ptr() == views[1].data_ptr()  # pylint: disable=protected-access
    assert torch.equal(dsrc.check_facets(cfgs, views), got)


@pytest.mark.parametrize("cplx", ["complex64", "complex128"])
def test_check_facets_on_complex_input_is_check_facet_per_facet(cplx):
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    # complex intensities and complex noise: the existing check, one row per facet
    sources = case("n1024")[2] + [(complex(i, -0.5 * i), c0, c1) for i, c0, c1 in real_sources()[37:]]
    dsrc, cfgs = sw.DeviceSources(sources, N), facet_configs()
    gen = torch.Generator(device="cpu").manual_seed(6)
    approx = []
    for cfg in cfgs:
        t = dsrc.facet(cfg)
        approx.append((t + 1e-3 * torch.randn((SIZE, SIZE), dtype=torch.complex128, generator=gen).to(t.device)).to(getattr(torch, cplx)))
    got = dsrc.check_facets(cfgs, approx)
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(cfgs), 2) and got.device == dsrc.device
    for k, (cfg, a) in enumerate(zip(cfgs, approx)):
        assert float(got[k, 0]) == dsrc.check_facet(cfg, a) > 0
    assert torch.equal(dsrc.check_facets(cfgs, torch.stack(approx)), got)  # one [n, size, size] tensor: its slices
    assert tuple(dsrc.check_facets([], []).shape) == (0, 2)


def test_check_facets_parameter_errors():
    import torch

    dsrc, cfgs = device_sources(), facet_configs()
    ok = _noisy(torch.float32)
    with pytest.raises(ValueError):  # not square
        dsrc.check_facets(cfgs, [ok[0], ok[1][:, : SIZE - 1], ok[2]])
    with pytest.raises(ValueError):  # not 2-D
        dsrc.check_facets(cfgs[:1], [ok[0][None]])
    with pytest.raises(ValueError):  # non-unit inner stride: never gathered behind the caller's back
        dsrc.check_facets(cfgs[:1], [ok[0].t()])
    with pytest.raises(ValueError):
        dsrc.check_facets(cfgs[:1], [torch.zeros((SIZE, 2 * SIZE), dtype=torch.float32, device=dsrc.device)[:, ::2]])
    with pytest.raises(ValueError):  # one facet short
        dsrc.check_facets(cfgs, ok[:2])
    with pytest.raises(ValueError):
        dsrc.check_facets(cfgs[:1], [ok[0].to(torch.float16)])
    with pytest.raises(ValueError):  # a mask of another length than the facet
        dsrc.check_facets(cfgs[1:2], [ok[1][:60, :60]])


def test_check_facet_still_refuses_real_input():
    import torch

    dsrc, cfg = device_sources(), facet_configs()[0]
    for dtype in (torch.float32, torch.float64):
        with pytest.raises(ValueError, match="complex"):
            dsrc.check_facet(cfg, torch.zeros((SIZE, SIZE), dtype=dtype, device=dsrc.device))
    with pytest.raises(ValueError):
        dsrc.subgrids([], dtype=torch.float32)
