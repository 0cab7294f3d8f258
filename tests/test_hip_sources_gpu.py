"""
GPU tests of the device point-source truths (``DeviceSources``: csrc/swiftly_sources.h behind four handle-free entry
points).  Every expectation comes from ``oracle/swiftly_oracle.py`` or from a formula in this file:

* ``exact_subgrid``: the direct Fourier sum with the phase reduced in integers, ``(c * u) % N`` in int64, then
  ``exp(2 pi i r / N)`` -- the form the kernels implement.  A double evaluation of it is within 1.2 .. 3.5 eps * scale of
  a long-double evaluation on the cases below, the reference's unreduced formula is off by 20 .. 178 000 eps * scale.
* the oracle's ``make_subgrid_from_sources`` / ``make_facet_from_sources`` (the reference's own formulas).

``eps = 2^-52``, ``scale = sum |I_s| / N^2``.  Bound of the exact-phase comparison: ``(2 S + 32) eps scale`` -- about
10 eps per term for two sincos results, two complex products and the scaling, plus (S - 1) eps for the sum, doubled.
Bound of the comparison with the reference formula: ``8 eps (pi N / 2) scale``, that formula's own phase rounding.
"""
import functools

import numpy
import pytest

from oracle import swiftly_oracle as orc

pytestmark = pytest.mark.gpu

EPS = 2.0**-52
TEST_PARAMS = dict(W=13.5625, fov=1.0, N=1024, yB_size=416, yN_size=512, xA_size=228, xM_size=256)


def random_sources(seed, count, N, extra=()):
    rng = numpy.random.default_rng(seed)
    out = list(extra)
    while len(out) < count:
        c0, c1 = (int(v) for v in rng.integers(-N // 2, N // 2, size=2))
        out.append((complex(rng.standard_normal(), rng.standard_normal()), c0, c1))
    return out


def holes(size, seed):
    mask = numpy.ones(size)
    mask[numpy.random.default_rng(seed).choice(size, size // 5, replace=False)] = 0
    mask[0] = mask[size // 2] = 0
    return mask


# name -> (N, size, sources, [(off0, off1, mask0, mask1), ...])
@functools.lru_cache(maxsize=None)
def case(name):
    if name == "n1024":
        return 1024, 100, random_sources(1, 37, 1024), [(0, 0, None, None)]
    if name == "n1024-odd-masked":
        return 1024, 93, random_sources(2, 5, 1024), [(-5 * 93, 1024 + 3 * 93, holes(93, 5), holes(93, 6))]
    if name == "n131072":
        N = 131072
        return N, 64, random_sources(3, 37, N, [(1.25 - 0.5j, -N // 2, N // 2 - 1)]), [(65504, -65504, None, None)]
    if name == "n131072-one":
        N = 131072
        return N, 64, [(1.25 - 0.5j, -N // 2, N // 2 - 1)], [(65504, -65504, None, None)]
    if name == "no-sources":
        return 1024, 100, [], [(100, -200, None, None)]
    if name == "batch":  # 7 subgrids, two off0 values, ragged tiles; one masked
        offs = [(70, 0), (70, 140), (-210, 140), (70, -70), (-210, 0), (-210, 1024 + 70), (70, 70)]
        return 1024, 70, random_sources(4, 21, 1024), [
            (o0, o1, holes(70, 7) if k == 2 else None, holes(70, 8) if k == 2 else None) for k, (o0, o1) in enumerate(offs)]
    if name == "xA928":  # 14.5 tiles of 64: the 64k catalogue's own subgrid size
        return 65536, 928, random_sources(5, 3, 65536), [(928 * 3, 928 * 70, None, None)]
    raise KeyError(name)


def scale_of(name):
    N, _, sources, _ = case(name)
    return sum(abs(s[0]) for s in sources) / N**2


def configs(name):
    import ska_sdp_exec_swiftly_amd as sw

    _, size, _, subs = case(name)
    return [sw.SubgridConfig(o0, o1, size, m0, m1) for o0, o1, m0, m1 in subs]


@functools.lru_cache(maxsize=None)
def exact_subgrids(name):
    """[n, size, size]: the direct Fourier sum with integer-reduced phases (this file's own formula)"""
    N, size, sources, subs = case(name)
    out = numpy.zeros((len(subs), size, size), dtype=complex)
    for k, (o0, o1, m0, m1) in enumerate(subs):
        u0 = numpy.arange(size, dtype=numpy.int64) + (o0 - size // 2)
        u1 = numpy.arange(size, dtype=numpy.int64) + (o1 - size // 2)
        for intensity, c0, c1 in sources:
            p0 = numpy.exp(2j * numpy.pi * ((c0 * u0) % N) / N)
            p1 = numpy.exp(2j * numpy.pi * ((c1 * u1) % N) / N)
            out[k] += (intensity / N**2) * p0[:, None] * p1[None, :]
        if m0 is not None:
            out[k] *= m0[:, None]
        if m1 is not None:
            out[k] *= m1[None, :]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_subgrids(name):
    """the same subgrids by the reference's formula (oracle)"""
    N, size, sources, subs = case(name)
    out = numpy.array([orc.make_subgrid_from_sources(sources, N, size, [o0, o1], [m0, m1]) for o0, o1, m0, m1 in subs])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def device_sources(name):
    import ska_sdp_exec_swiftly_amd as sw

    N, _, sources, _ = case(name)
    return sw.DeviceSources(sources, N)


@functools.lru_cache(maxsize=None)
def device_subgrids(name):
    """complex128 device truth of a case, computed once and left unchanged"""
    return device_sources(name).subgrids(configs(name))


ALL_CASES = ["n1024", "n1024-odd-masked", "n131072", "n131072-one", "no-sources", "batch", "xA928"]


# ---------------------------------------------------------------------------------------------- 1. exact-phase truth
@pytest.mark.parametrize("name", ALL_CASES)
def test_subgrids_match_exact_phase_truth(name):
    import torch

    _, size, sources, subs = case(name)
    want = exact_subgrids(name)
    got = device_subgrids(name)
    assert got.dtype == torch.complex128 and tuple(got.shape) == (len(subs), size, size)
    err = float(numpy.abs(got.cpu().numpy() - want).max())
    bound = (2 * len(sources) + 32) * EPS * scale_of(name)
    print(f"{name}: max|err| = {err / (EPS * scale_of(name)) if sources else err:.2f} eps*scale, bound {2 * len(sources) + 32}")
    assert err <= bound, (err, bound)
    # one at a time (subgrid) gives what the batch gives, bit for bit
    one = device_sources(name).subgrid(configs(name)[-1])
    assert torch.equal(one, got[-1])


@pytest.mark.parametrize("name", ALL_CASES)
def test_subgrids_complex64_rounds_once(name):
    import torch

    _, size, sources, subs = case(name)
    want = exact_subgrids(name)
    got = device_sources(name).subgrids(configs(name), dtype=torch.complex64)
    assert got.dtype == torch.complex64
    err = float(numpy.abs(got.cpu().numpy().astype(complex) - want).max())
    bound = (2 * len(sources) + 32) * EPS * scale_of(name) + 2.0**-24 * float(numpy.abs(want).max())
    assert err <= bound, (err, bound)
    # and it IS the complex128 result rounded once
    assert torch.equal(got, device_subgrids(name).to(torch.complex64))
    # into a caller's row-strided buffer
    wide = torch.full((len(subs), size, size + 5), 7.0, dtype=torch.complex64, device=got.device)
    ret = device_sources(name).subgrids(configs(name), out=wide[:, :, :size])
    assert ret.data_ptr() == wide.data_ptr() and torch.equal(wide[:, :, :size], got)
    assert bool((wide[:, :, size:] == 7.0).all())


# ------------------------------------------------------------------ 2. agreement with the reference-pinned host formula
@pytest.mark.parametrize("name", ["n1024", "n1024-odd-masked", "n131072", "n131072-one"])
def test_subgrids_agree_with_reference_formula(name):
    N = case(name)[0]
    err = float(numpy.abs(device_subgrids(name).cpu().numpy() - reference_subgrids(name)).max())
    bound = 8 * EPS * (numpy.pi * N / 2) * scale_of(name)
    print(f"{name}: device vs reference formula {err / (EPS * scale_of(name)):.0f} eps*scale, bound {bound / (EPS * scale_of(name)):.0f}")
    assert err <= bound, (err, bound)


# ------------------------------------------------------------------------------------------------------- 3. facets
FACET_N, FACET_SIZE, FACET_OFF = 1024, 93, (-200, 1024 + 300)


def facet_problem():
    N, size, (off0, off1) = FACET_N, FACET_SIZE, FACET_OFF
    lo0, lo1 = off0 - size // 2, off1 - size // 2
    mask0, mask1 = holes(size, 11), holes(size, 12)
    mask0[size - 1] = mask1[size - 1] = 1  # the last pixel stays open
    open0 = int(numpy.flatnonzero(mask0)[3]), int(numpy.flatnonzero(mask1)[4])
    sources = [
        (1.0, lo0 + open0[0], lo1 + open0[1] - N),          # inside, given one period off
        (2.5 - 1j, lo0 + size - 1, lo1 + size - 1 - N),      # on the last pixel
        (3.0, lo0 + size, lo1 + 5 - N),                      # just outside along axis 0
        (0.5j, lo0 + 7 + N, lo1 + 9 - 2 * N),                # wraps modulo N on both axes
        (0.25, lo0 + 7, lo1 + 9 - N),                        # ... onto a pixel that is already taken: duplicates
        (4.0, lo0 + 7 - N, lo1 + 9 - N),
        (5.0, lo0 + 0, lo1 + 20 - N),                        # row 0 is masked: zeroed
        (6.0, lo0 + 40, lo1 + size // 2 - N),                # column size // 2 is masked
        (7.0, 400, 400),                                     # far outside
    ]
    sources += [(complex(k, -k), lo0 + 10 + k, lo1 + 3 * k - N) for k in range(1, 25)]  # several per row region
    return N, size, off0, off1, mask0, mask1, sources


@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
@pytest.mark.parametrize("masked", [True, False])
def test_facet_equals_oracle_bit_for_bit(dtype, masked):
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    N, size, off0, off1, mask0, mask1, sources = facet_problem()
    if not masked:
        mask0 = mask1 = None
    want = orc.make_facet_from_sources(sources, N, size, [off0, off1], [mask0, mask1])
    assert numpy.count_nonzero(want) >= 20 and want[size - 1, size - 1] != 0
    dsrc = sw.DeviceSources(sources, N)
    got = dsrc.facet(sw.FacetConfig(off0, off1, size, mask0, mask1), dtype=getattr(torch, dtype))
    assert got.dtype == getattr(torch, dtype)
    assert numpy.array_equal(got.cpu().numpy(), want.astype(dtype))
    # a second call into the same (dirty) buffer zeroes it first
    got.fill_(3.0)
    dsrc.facet(sw.FacetConfig(off0, off1, size, mask0, mask1), out=got)
    assert numpy.array_equal(got.cpu().numpy(), want.astype(dtype))


# ------------------------------------------------------------------------------------------------------- 4. checks
def delta_like(t, rms, seed):
    """a fixed random complex128 perturbation of RMS exactly ``rms``"""
    import torch

    gen = torch.Generator(device="cpu").manual_seed(seed)
    d = torch.randn(tuple(t.shape), dtype=torch.complex128, generator=gen)
    d *= rms / float(d.abs().pow(2).mean().sqrt())
    return d.to(t.device)


@pytest.mark.parametrize("name", ["n1024", "n131072", "n1024-odd-masked"])
def test_check_subgrid_of_own_truth(name):
    dsrc, cfg = device_sources(name), configs(name)[0]
    err = dsrc.check_subgrid(cfg, device_subgrids(name)[0])
    assert isinstance(err, float)
    assert err <= (2 * len(case(name)[2]) + 32) * EPS * scale_of(name), err


@pytest.mark.parametrize("dtype,rel", [("complex128", 1e-12), ("complex64", 1e-5)])
@pytest.mark.parametrize("name", ["n1024", "batch"])
def test_check_subgrids_measures_a_known_perturbation(name, dtype, rel):
    import torch

    truth = device_subgrids(name)
    rms_t = truth.abs().pow(2).mean(dim=(1, 2)).sqrt()
    delta = delta_like(truth, 1.0, 21) * (rel * rms_t)[:, None, None]
    approx = (truth + delta).to(getattr(torch, dtype))
    got = device_sources(name).check_subgrids(configs(name), approx)
    assert got.dtype == torch.float64 and tuple(got.shape) == (truth.shape[0], 2)
    want = delta.abs().pow(2).mean(dim=(1, 2)).sqrt()
    print(f"{name} {dtype}: RMSE / rms(delta) - 1 = {(got[:, 0] / want - 1).cpu().numpy()}")
    assert bool(((got[:, 0] - want).abs() <= 1e-3 * want).all()), (got, want)
    assert bool(((got[:, 1] - rms_t).abs() <= 1e-12 * rms_t).all()), (got, rms_t)
    # one subgrid through check_subgrid: the same number
    assert device_sources(name).check_subgrid(configs(name)[0], approx[0]) == float(got[0, 0])


def test_check_facet_is_not_a_difference_of_sums():
    """delta of RMS 1e-12 on a 512^2 facet whose sources are O(1): sum |approx|^2 - sum |truth|^2 would cancel
    completely in double; the pixel-by-pixel residual does not"""
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    N, size = 2048, 512
    sources = random_sources(9, 40, size) + [(2.0, -256, 255), (1.5, 255, -256), (3.0, 700, 700)]
    mask0 = holes(size, 13)
    cfg = sw.FacetConfig(0, N, size, mask0, None)
    dsrc = sw.DeviceSources(sources, N)
    truth = dsrc.facet(cfg)
    assert numpy.array_equal(truth.cpu().numpy(), orc.make_facet_from_sources(sources, N, size, [0, N], [mask0, None]))
    assert dsrc.check_facet(cfg, truth) == 0.0
    for dtype, rms in ((torch.complex128, 1e-12), (torch.complex64, 1e-5)):
        delta = delta_like(truth, rms, 22)
        got = dsrc.check_facet(cfg, (truth + delta).to(dtype))
        print(f"check_facet {dtype}: {got:.6e} for rms(delta) = {rms:.0e}")
        assert abs(got - rms) <= 1e-3 * rms, (got, rms)
    # the numpy form of the package on the same input
    approx = truth + delta_like(truth, 1e-12, 22)
    host = sw.check_facet(N, cfg, approx, sources)
    assert abs(dsrc.check_facet(cfg, approx) - host) <= 1e-3 * host


@pytest.mark.parametrize("name", ["n1024", "n1024-odd-masked", "n131072"])
def test_check_subgrid_agrees_with_host_check(name):
    import ska_sdp_exec_swiftly_amd as sw

    N, _, sources, _ = case(name)
    truth = device_subgrids(name)[0]
    approx = truth + delta_like(truth, 1e-12 * float(truth.abs().pow(2).mean().sqrt()), 23)
    dev = device_sources(name).check_subgrid(configs(name)[0], approx)
    host = sw.check_subgrid(N, configs(name)[0], approx, sources)
    assert abs(dev - host) <= 8 * EPS * (numpy.pi * N / 2) * scale_of(name), (dev, host)


def test_check_subgrids_is_reproducible_and_reads_strided_input_in_place():
    import torch

    name = "batch"
    truth = device_subgrids(name)
    n, size = truth.shape[0], truth.shape[-1]
    approx = truth + delta_like(truth, 1e-9 * float(truth.abs().pow(2).mean().sqrt()), 24)
    dsrc = device_sources(name)
    first = dsrc.check_subgrids(configs(name), approx)
    again = dsrc.check_subgrids(configs(name), approx)
    assert torch.equal(first, again)  # bit-identical: fixed-order sums, no atomics
    for dtype in (torch.complex128, torch.complex64):
        wide = torch.full((n + 1, size + 3, size + 7), 1e3, dtype=dtype, device=truth.device)
        view = wide[1:, 2 : 2 + size, 4 : 4 + size]
        view.copy_(approx)
        assert not view.is_contiguous()
        assert dsrc._approx(view, 3).data_ptr() == view.data_ptr()  # pylint: disable=protected-access
        assert torch.equal(dsrc.check_subgrids(configs(name), view), dsrc.check_subgrids(configs(name), view.contiguous()))
    # a host array is uploaded
    assert torch.equal(dsrc.check_subgrids(configs(name), approx.cpu().numpy()), first)


# --------------------------------------------------------------------------------------------------- 5. end to end
def test_roundtrip_checked_on_the_device():
    """the reference round trip (tests/test_api.py:42-125, as tests/test_hip_api_gpu.py::test_swiftly_api_roundtrip: its
    TEST_PARAMS, full covers, complex128, its bounds) with six sources, the facets built and every subgrid and finished
    facet checked on the device.

    The bounds of that test are absolute and belong to its input, one source of intensity 1: the transform is linear,
    so the window error of the algorithm itself scales with the flux.  The six sources therefore carry unit flux in
    all, sum |I_s| = 1.  What the algorithm (not this implementation) delivers for them was taken from the CPU oracle's
    replica of the reference round trip (``orc.forward_all`` / ``orc.backward_all`` in double, numpy checks): subgrid
    RMSE 1.4e-16, facet RMSE 1.7e-11 .. 1.46e-10 over the nine facets -- inside both bounds.  (The same six positions with
    the intensities 1, 0.5, 2, 1.5, 0.75, 1 as they stand, flux 6.75, give 1.1e-10 .. 9.8e-10 in the oracle itself, and
    the first facet's 4.2073e-10 is also what the device round trip gave for them: the bound is then missed by the
    algorithm, whatever computes it.)"""
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    weights, places = [1, 0.5, 2, 1.5, 0.75, 1], [(1, 0), (-300, 200), (17, -45), (-500, 480), (400, -505), (-250, 300)]
    sources = [(w / sum(weights), c0, c1) for w, (c0, c1) in zip(weights, places)]
    cfg = sw.SwiftlyConfig(backend="hip", **TEST_PARAMS)
    sg_cfgs = sw.make_full_subgrid_cover(cfg)
    facet_cfgs = sw.make_full_facet_cover(cfg)
    dsrc = sw.DeviceSources(sources, cfg.image_size)
    facets = [dsrc.facet(fc) for fc in facet_cfgs]
    # every source is in exactly one facet; three of them lie in the outermost (corner) facets, away from the centre on both axes
    host = [orc.make_facet_from_sources(sources, cfg.image_size, fc.size, [fc.off0, fc.off1], [fc.mask0, fc.mask1])
            for fc in facet_cfgs]
    outer = [numpy.count_nonzero(h) for h, fc in zip(host, facet_cfgs) if fc.off0 != 0 and fc.off1 != 0]
    assert sum(outer) >= 2 and sum(numpy.count_nonzero(h) for h in host) == 6
    fwd = sw.SwiftlyForward(cfg, list(zip(facet_cfgs, facets)), 1, 100)
    bwd = sw.SwiftlyBackward(cfg, facet_cfgs, 1, 100)
    columns = {}
    for c in sg_cfgs:
        columns.setdefault(c.off0, []).append(c)
    worst = torch.zeros((), dtype=torch.float64, device=facets[0].device)
    for column in columns.values():
        sgs = fwd.get_subgrid_tasks(column)
        errs = dsrc.check_subgrids(column, torch.stack(list(sgs)))
        worst = torch.maximum(worst, errs[:, 0].max())
        bwd.add_new_subgrid_tasks(column, sgs)
    assert float(worst) < 1e-9, float(worst)
    for fc, facet in zip(facet_cfgs, bwd.finish()):
        assert dsrc.check_facet(fc, facet) < 3e-10


# ------------------------------------------------------------------------------------------------ 6. parameter errors
def test_parameter_errors():
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    dsrc = device_sources("n1024")
    with pytest.raises(ValueError):
        dsrc.subgrids([sw.SubgridConfig(0, 0, 64), sw.SubgridConfig(64, 0, 65)])
    with pytest.raises(ValueError):
        dsrc.check_subgrid(sw.SubgridConfig(0, 0, 64), torch.zeros((64, 64), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        dsrc.check_subgrids([sw.SubgridConfig(0, 0, 64)], numpy.zeros((1, 64, 64)))
    with pytest.raises(ValueError):
        dsrc.check_facet(sw.FacetConfig(0, 0, 64), torch.zeros((64, 64), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        sw.DeviceSources([(1, 0, 0)], 2**31 + 2)
    with pytest.raises(ValueError):
        dsrc.check_subgrids([sw.SubgridConfig(0, 0, 64)], torch.zeros((1, 64, 63), dtype=torch.complex64, device="cuda"))
    with pytest.raises(ValueError):  # a mask of another length than the approximation
        dsrc.check_subgrid(sw.SubgridConfig(0, 0, 64, numpy.ones(64), None), torch.zeros((60, 60), dtype=torch.complex64, device="cuda"))
