"""
complex128 at padded facet sizes yN = 16384 and 32768 (catalogue entries 64k[1]-n16k-1k and 128k[1]-n32k-1k, and the
headline configuration 64k[1]-n32k-1k).

* primitives against oracle/swiftly_oracle.py on a few rows: prepare_facet / finish_facet (with and without mask) along
  both axes, extract_column with and without a row map; bound 5e-12 * max|expected| (tests/test_hip_core_gpu.py).
* whole facets (separable ``outer(a, b)`` built on the device, components on the 1/8 grid: exact in any precision):
  every row of a full-size prepare_facet / finish_facet against two 1-D oracle calls, with row counts that span several
  scratch chunks of the contiguous-axis four-step and are not a multiple of the chunk.
* SwiftlyForward / SwiftlyBackward in complex128 against oracle/separable.py: relative RMSE <= 1e-10.
* the complex64 headline pipeline against the complex128 HIP result (bench.py's parity bound).
* ``SwiftlyCoreHip.supports_dtype`` and the refusals that stay (yN = 65536, yN = 49152 = 3 * 16384).

Peak device memory stays under ~40 GB per test (one 128k[1]-n32k-1k facet: 11.3 GB, its prepared form 14 GB).
"""
import gc

import numpy
import pytest

import bench
from oracle import separable as sep
from oracle import swiftly_oracle as orc

pytestmark = pytest.mark.gpu

C128_TOL = 5e-12  # max|err| / max|expected|, single primitives (tests/test_hip_core_gpu.py)
PASS_TOL = 1e-10  # relative RMSE of whole passes

# name -> SwiftlyConfig parameters (ska_sdp_exec_swiftly_amd/swift_configs.py)
ENTRIES = {
    "64k[1]-n16k-1k": dict(W=13.5625, fov=1.0, N=65536, yB_size=13312, yN_size=16384, xA_size=896, xM_size=1024),
    "128k[1]-n32k-1k": dict(W=13.5625, fov=1.0, N=131072, yB_size=26624, yN_size=32768, xA_size=896, xM_size=1024),
}
HEADLINE = dict(W=10.875, fov=1.0, N=65536, yB_size=22528, yN_size=32768, xA_size=928, xM_size=1024)


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    import torch

    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _cores(p):
    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    return (SwiftlyCoreHip(p["W"], p["N"], p["xM_size"], p["yN_size"]),
            orc.OracleCore(p["W"], p["N"], p["xM_size"], p["yN_size"]))


def _maxrel(got, want):
    got = numpy.asarray(got)
    assert got.shape == want.shape and got.dtype == numpy.complex128, (got.shape, want.shape, got.dtype)
    return float(numpy.max(numpy.abs(got - want)) / numpy.max(numpy.abs(want)))


def _relrms(got, want):
    return float(numpy.sqrt(numpy.mean(numpy.abs(got - want) ** 2) / numpy.mean(numpy.abs(want) ** 2)))


def _crandn(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _grid_vec(rng, n):
    """complex128 vector on the 1/8 grid (oracle/separable.py): its outer products are exact"""
    re = numpy.clip(numpy.round(rng.standard_normal(n) * 8) / 8, -3, 3)
    im = numpy.clip(numpy.round(rng.standard_normal(n) * 8) / 8, -3, 3)
    return re + 1j * im


def _offsets(p):
    """facet offsets: 0, positive, negative, >= N (all multiples of the facet offset step)"""
    step = p["N"] // p["xM_size"]
    return (0, 37 * step, -p["yB_size"], p["N"] + 11 * step)


@pytest.mark.parametrize("name", list(ENTRIES))
def test_primitives_match_oracle(name):
    p = ENTRIES[name]
    core, ref = _cores(p)
    yB, yN = p["yB_size"], p["yN_size"]
    rng = numpy.random.default_rng(2024)
    rows = _crandn(rng, (3, yB))
    cols = numpy.ascontiguousarray(rows.T)
    acc = _crandn(rng, (3, yN))
    accT = numpy.ascontiguousarray(acc.T)
    mask = (rng.random(yB) > 0.3).astype(float)
    errs = {}
    for off in _offsets(p):
        errs[f"prepare ax1 off={off}"] = _maxrel(core.prepare_facet(rows, off, axis=1), ref.prepare_facet(rows, off, 1))
        errs[f"prepare ax0 off={off}"] = _maxrel(core.prepare_facet(cols, off, axis=0), ref.prepare_facet(cols, off, 0))
        errs[f"finish ax1 off={off}"] = _maxrel(core.finish_facet(acc, off, yB, axis=1), ref.finish_facet(acc, off, yB, 1))
        errs[f"finish ax0 off={off}"] = _maxrel(core.finish_facet(accT, off, yB, axis=0), ref.finish_facet(accT, off, yB, 0))
        got = core.finish_facet(acc, off, yB, axis=1, mask=mask)
        errs[f"finish ax1 mask off={off}"] = _maxrel(got, ref.finish_facet(acc, off, yB, 1) * mask[None, :])
        assert not got[:, mask == 0].any()
        got = core.finish_facet(accT, off, yB, axis=0, mask=mask)
        errs[f"finish ax0 mask off={off}"] = _maxrel(got, ref.finish_facet(accT, off, yB, 0) * mask[:, None])
    print(name, {k: float(f"{v:.3g}") for k, v in errs.items()})
    assert max(errs.values()) <= C128_TOL, errs


@pytest.mark.parametrize("name", list(ENTRIES))
def test_extract_column_matches_oracle(name):
    """extract_column on a full BF_F [yN, yB] (modular row gather fused into the contiguous-axis load) and on the
    row-compacted form (prepare_facet_rows along the strided axis + subgrid_column_rows)"""
    import torch

    p = ENTRIES[name]
    core, ref = _cores(p)
    yB, yN, xA = p["yB_size"], p["yN_size"], p["xA_size"]
    step = p["N"] // p["xM_size"]
    errs = {}
    gen = torch.Generator(device="cuda").manual_seed(5)
    BF_F = torch.randn((yN, yB), dtype=torch.complex128, device="cuda", generator=gen)
    for sg_off0, f_off1 in ((0, 0), (xA * 9, 53 * step), (-xA * 13, -yB)):
        got = core.extract_column(BF_F, sg_off0, f_off1).cpu().numpy()
        gathered = core.extract_from_facet(BF_F, sg_off0, axis=0).cpu().numpy()  # bit-exact gather
        errs[f"plain sg={sg_off0} f={f_off1}"] = _maxrel(got, ref.prepare_facet(gathered, f_off1, 1))
    del BF_F, gathered
    # row map: two subgrid columns kept, the facet is [yB, C] with a narrow axis 1 (C = facet size along axis 1)
    C = 1500
    rng = numpy.random.default_rng(6)
    facet = _crandn(rng, (yB, C))
    f_off0, sg_off0s = 29 * step, (xA * 4, -xA * 21)
    rowmap, n_rows = core.subgrid_column_rows(sg_off0s)
    BF_c = core.prepare_facet_rows(torch.from_numpy(facet).cuda(), f_off0, rowmap, n_rows)
    BF_ref = ref.prepare_facet(facet, f_off0, 0)
    for sg_off0 in sg_off0s:
        got = core.extract_column(BF_c, sg_off0, 7 * step, rowmap=rowmap).cpu().numpy()
        want = ref.prepare_facet(ref.extract_from_facet(BF_ref, sg_off0, 0), 7 * step, 1)
        errs[f"rowmap sg={sg_off0}"] = _maxrel(got, want)
    print(name, {k: float(f"{v:.3g}") for k, v in errs.items()})
    assert max(errs.values()) <= C128_TOL, errs


def _outer_maxrel(got, a, w, block=2048):
    """max |got - outer(a, w)| / max |outer(a, w)| on the device, in row blocks"""
    import torch

    A = torch.from_numpy(a).cuda()
    Wv = torch.from_numpy(w).cuda()
    assert tuple(got.shape) == (a.size, w.size) and got.dtype == torch.complex128
    err = 0.0
    for i in range(0, a.size, block):
        err = max(err, float((got[i:i + block] - torch.outer(A[i:i + block], Wv)).abs().max()))
    return err / (float(numpy.abs(a).max()) * float(numpy.abs(w).max()))


# scratch chunk of the contiguous-axis four-step: default 1 GiB = 4096 rows at 16384 points (13312 rows = 3.25 chunks);
# at 32768 points 700 MiB = 1400 rows (26624 rows = 19.02 chunks)
CHUNK_MB = {"64k[1]-n16k-1k": None, "128k[1]-n32k-1k": "700"}


@pytest.mark.parametrize("name", list(ENTRIES))
def test_full_facet_separable(name, monkeypatch):
    import torch

    if CHUNK_MB[name]:
        monkeypatch.setenv("SWIFTLY_LONG_ROWS_CHUNK_MB", CHUNK_MB[name])
    p = ENTRIES[name]
    core, ref = _cores(p)
    yB, yN = p["yB_size"], p["yN_size"]
    step = p["N"] // p["xM_size"]
    rng = numpy.random.default_rng(77)
    a, b, c = _grid_vec(rng, yB), _grid_vec(rng, yB), _grid_vec(rng, yN)
    mask = (rng.random(yB) > 0.2).astype(float)
    off = -61 * step
    errs = {}
    facet = torch.outer(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    out = core.prepare_facet(facet, off, axis=1)
    errs["prepare ax1"] = _outer_maxrel(out, a, ref.prepare_facet(b, off, 0))
    del out
    out = core.prepare_facet(facet, off, axis=0)  # strided axis: [yN, yB] = outer(P(a), b)
    errs["prepare ax0"] = _outer_maxrel(out, ref.prepare_facet(a, off, 0), b)
    del out, facet
    acc = torch.outer(torch.from_numpy(a).cuda(), torch.from_numpy(c).cuda())  # [yB, yN]
    out = core.finish_facet(acc, off, yB, axis=1, mask=mask)
    errs["finish ax1 mask"] = _outer_maxrel(out, a, ref.finish_facet(c, off, yB, 0) * mask)
    del out, acc
    torch.cuda.synchronize()
    print(name, {k: float(f"{v:.3g}") for k, v in errs.items()})
    assert max(errs.values()) <= C128_TOL, errs


def _facet128(vec, size):
    import torch

    a, b = vec
    out = torch.zeros((size, size), dtype=torch.complex128, device="cuda")
    for r in range(a.shape[0]):
        out.add_(torch.outer(torch.from_numpy(a[r]).cuda(), torch.from_numpy(b[r]).cuda()))
    return out


def _subgrids(p):
    xA = p["xA_size"]
    import ska_sdp_exec_swiftly_amd as sw

    offs = [(0, 0), (3 * xA, 0), (10 * xA, 2 * xA), (-7 * xA, 5 * xA), (20 * xA, -4 * xA), (40 * xA, 30 * xA)]
    return [sw.SubgridConfig(o0, o1, xA) for o0, o1 in offs]


def _forward_c128(p, facet_cfgs, vectors, sg_cfgs, plan):
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    cfg = sw.SwiftlyConfig(backend="hip", **p)
    facets = [_facet128(v, c.size) for v, c in zip(vectors, facet_cfgs)]
    fwd = sw.SwiftlyForward(cfg, list(zip(facet_cfgs, facets)), subgrid_configs=sg_cfgs if plan else None)
    assert fwd.wave_axis == 0 and fwd.dtype == torch.complex128
    ordered = sorted(sg_cfgs, key=lambda c: c.off0)
    got = [t.cpu().numpy() for t in fwd.get_subgrid_tasks(ordered)]
    assert all(g.dtype == numpy.complex128 for g in got)
    del fwd, facets
    return ordered, got


@pytest.mark.parametrize("name", list(ENTRIES))
def test_forward_matches_separable_oracle(name):
    import ska_sdp_exec_swiftly_amd as sw

    p = ENTRIES[name]
    yB = p["yB_size"]
    facet_cfgs = [sw.FacetConfig(0, 0, yB), sw.FacetConfig(yB, -yB, yB)]
    if p["yN_size"] >= 32768:
        facet_cfgs = facet_cfgs[1:]  # one facet + its prepared form + the four-step scratch: ~40 GB
    vectors = [sep.facet_vectors(300 + j, yB) for j in range(len(facet_cfgs))]
    sg_cfgs = _subgrids(p)
    for plan in (False, True):
        ordered, got = _forward_c128(p, facet_cfgs, vectors, sg_cfgs, plan)
        par = bench.verify_subgrids(p, facet_cfgs, vectors, ordered, dict(enumerate(got)), tol=PASS_TOL)
        print(f"{name} forward complex128 plan={plan}: relRMSE {par['rel_rmse']:.3e} each {par['rel_rmse_each']}")
        assert par["rel_rmse"] <= PASS_TOL, par


def test_backward_matches_separable_oracle():
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    p = ENTRIES["64k[1]-n16k-1k"]
    yB, xA = p["yB_size"], p["xA_size"]
    cfg = sw.SwiftlyConfig(backend="hip", **p)
    facet_cfgs = [sw.FacetConfig(0, 0, yB), sw.FacetConfig(yB, -yB, yB)]
    sg_cfgs = sorted(_subgrids(p), key=lambda c: c.off0)
    vectors = [sep.subgrid_vectors(500 + i, xA, rank=2) for i in range(len(sg_cfgs))]
    data = [_facet128(v, xA) for v in vectors]
    bwd = sw.SwiftlyBackward(cfg, facet_cfgs, wave_axis=0)
    bwd.add_new_subgrid_tasks(sg_cfgs, data)
    out = bwd.finish()
    torch.cuda.synchronize()
    assert all(t.dtype == torch.complex128 for t in out)
    par = bench.verify_facets(p, facet_cfgs, sg_cfgs, vectors, out, rows_per_facet=16, tol=PASS_TOL)
    print(f"backward complex128: relRMSE per facet {par['rel_rmse_each']}")
    assert par["rel_rmse"] <= PASS_TOL, par


def test_headline_complex64_against_complex128():
    """64k[1]-n32k-1k: complex128 HIP against the separable oracle, then the default complex64 pipeline against the
    complex128 HIP result"""
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    p = HEADLINE
    yB = p["yB_size"]
    facet_cfgs = [sw.FacetConfig(0, 0, yB), sw.FacetConfig(yB, -yB, yB)]
    vectors = [sep.facet_vectors(40 + j, yB) for j in range(2)]
    sg_cfgs = _subgrids(p)
    ordered, got128 = _forward_c128(p, facet_cfgs, vectors, sg_cfgs, plan=True)
    par = bench.verify_subgrids(p, facet_cfgs, vectors, ordered, dict(enumerate(got128)), tol=PASS_TOL)
    print(f"headline complex128 vs oracle: relRMSE {par['rel_rmse']:.3e}")
    assert par["rel_rmse"] <= PASS_TOL, par

    cfg = sw.SwiftlyConfig(backend="hip", **p)
    facets = [bench.separable_facet(torch, v, c) for v, c in zip(vectors, facet_cfgs)]
    fwd = sw.SwiftlyForward(cfg, list(zip(facet_cfgs, facets)), subgrid_configs=sg_cfgs)
    got64 = [t.cpu().numpy() for t in fwd.get_subgrid_tasks(ordered)]
    rel = max(_relrms(g64, g128) for g64, g128 in zip(got64, got128))
    print(f"headline complex64 (wave_axis={fwd.wave_axis}) vs complex128 HIP: relRMSE {rel:.3e}")
    assert rel <= bench.PARITY_TOL, rel


def test_supports_dtype():
    import torch

    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    cases = [  # (W, N, xM, yN), complex128 expected
        ((13.5625, 65536, 1024, 16384), True),
        ((13.5625, 131072, 1024, 32768), True),
        ((13.5625, 512, 128, 256), True),
        ((10.875, 131072, 1024, 65536), False),
        ((11.0, 98304, 512, 49152), False),  # 96k[1]-n48k-512: 3 * 16384
    ]
    for (W, N, xM, yN), want in cases:
        core = SwiftlyCoreHip(W, N, xM, yN)
        assert core.supports_dtype(numpy.complex128) is want, (yN, "complex128")
        assert core.supports_dtype(torch.complex128) is want
        assert core.supports_dtype(numpy.complex64) is True and core.supports_dtype(torch.complex64) is True
        if not want:
            with pytest.raises(NotImplementedError):
                core.prepare_facet(numpy.zeros(500, dtype=complex), 0, axis=1)
            with pytest.raises(NotImplementedError):
                core.prepare_facet(numpy.zeros((500, 2), dtype=complex), 0, axis=0)
        del core
    with pytest.raises(ValueError):
        SwiftlyCoreHip(13.5625, 512, 128, 256).supports_dtype(numpy.float32)
