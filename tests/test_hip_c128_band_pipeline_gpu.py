"""
The contiguous-axis-first forward pipeline (``wave_axis=1``) on complex128 facets.

* each C ABI entry point with complex128 data against compositions of the 1-D oracle primitives
  (oracle/swiftly_oracle.py): prepare_facet_band (plain band), prepare_facet_columns (single pass and four-step),
  transform_contributions (layouts 1 and 2), sum_finish_facets, wave_subgrid_side; bound 5e-12 * max|expected|
* whole passes against oracle/separable.py (relative RMSE <= 1e-10) and against the complex128 reference schedule
  (``wave_axis=0``: <= 1e-12 on a small configuration with a full cover; <= 1e-10 on 64k[1]-n16k-1k and
  128k[1]-n32k-1k, where each schedule's own rounding error is ~3e-11)
* schedule behaviour: shuffled requests, a partial wave, masks, prefetch on / off and the chunked four-step of K2 on / off
  (bit-identical), host-resident facets, ``delayed=True``
* defaults stay: ``preferred_wave_axis`` and the automatic choice are 0 for complex128; unsupported requests raise
"""
import gc
import os
import subprocess
import sys

import numpy
import pytest

import bench
from oracle import separable as sep
from oracle import swiftly_oracle as orc

pytestmark = pytest.mark.gpu

C128_TOL = 5e-12  # max|err| / max|expected|, single entry points
PASS_TOL = 1e-10  # relative RMSE against the separable oracle
SCHEDULE_TOL = 1e-12  # relative RMSE against the complex128 wave_axis=0 pass (small configuration)
# W = 13.5625 (1/pswf ~ 4.9e3 per axis): each schedule sits ~3e-11 from the exact result on its own rounding path, so two
# correct complex128 passes differ by up to the sum of their errors (measured 4.1e-11 at 64k[1]-n16k-1k)
SCHEDULE_TOL_W13 = 1e-10

# m = 128, xM = 256: complex128 sum_finish instance (7, 8); yN = 512: K2 in one column pass
SMALL = dict(W=11.0, fov=1.0, N=1024, yB_size=352, yN_size=512, xA_size=192, xM_size=256)
ENTRIES = {
    "64k[1]-n16k-1k": dict(W=13.5625, fov=1.0, N=65536, yB_size=13312, yN_size=16384, xA_size=896, xM_size=1024),
    "128k[1]-n32k-1k": dict(W=13.5625, fov=1.0, N=131072, yB_size=26624, yN_size=32768, xA_size=896, xM_size=1024),
}


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    import torch

    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _relrms(got, want):
    return float(numpy.sqrt(numpy.mean(numpy.abs(got - want) ** 2) / numpy.mean(numpy.abs(want) ** 2)))


def _maxrel(got, want):
    got = numpy.asarray(got)
    assert got.shape == want.shape and got.dtype == numpy.complex128, (got.shape, want.shape, got.dtype)
    return float(numpy.max(numpy.abs(got - want)) / numpy.max(numpy.abs(want)))


def _crandn(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _cores(p):
    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    return (SwiftlyCoreHip(p["W"], p["N"], p["xM_size"], p["yN_size"]),
            orc.OracleCore(p["W"], p["N"], p["xM_size"], p["yN_size"]))


def _facet128(vec, cfg, device="cuda"):
    """complex128 device facet ``sum_r a_r (x) b_r`` times the cover masks (bench.separable_facet in complex128)"""
    import torch

    a, b = vec
    yB = cfg.size
    m0 = cfg.mask0 if cfg.mask0 is not None else numpy.ones(yB)
    m1 = cfg.mask1 if cfg.mask1 is not None else numpy.ones(yB)
    out = torch.zeros((yB, yB), dtype=torch.complex128, device=device)
    for r in range(a.shape[0]):
        out.add_(torch.outer(torch.from_numpy(a[r] * m0).to(device), torch.from_numpy(b[r] * m1).to(device)))
    return out


# ------------------------------------------------------------------------------------------- entry points one by one
def test_prepare_facet_band_c128():
    import torch

    for p in (SMALL, ENTRIES["64k[1]-n16k-1k"]):
        core, ref = _cores(p)
        yN, step = p["yN_size"], p["N"] // p["xM_size"]
        rng = numpy.random.default_rng(31)
        rows, yB = 3, p["yB_size"]
        x = _crandn(rng, (rows, yB))
        for off in (0, 37 * step, -yB):
            got = core.prepare_facet_band(torch.from_numpy(x).cuda(), off, (0, yN), fold_other_axis_window=False)
            assert got.dtype == torch.complex128 and tuple(got.shape) == (rows, yN)
            assert _maxrel(got.cpu().numpy(), ref.prepare_facet(x, off, 1)) <= C128_TOL
        # a pruned band stays complex64-only
        with pytest.raises(NotImplementedError):
            core.prepare_facet_band(torch.from_numpy(x).cuda(), 0, (0, yN // 2), fold_other_axis_window=False)


@pytest.mark.parametrize("p", [SMALL, ENTRIES["64k[1]-n16k-1k"]], ids=["small", "64k"])
def test_prepare_facet_columns_c128(p):
    """K2 (one pass at yN = 512, four-step at 16384) with and without a row map"""
    import torch

    core, ref = _cores(p)
    m, yN, xA = core.xM_yN_size, core.yN_size, p["xA_size"]
    rng = numpy.random.default_rng(32)
    yB0, F = 96, 2
    logical = _crandn(rng, (F, yB0, yN))
    bands = torch.from_numpy(logical).cuda()
    off0s = [0, -3 * core.facet_off_step * 8]
    for use_rowmap in (False, True):
        rowmap, n_rows = core.subgrid_column_rows([0, 3 * xA]) if use_rowmap else (None, yN)
        rm = rowmap.cpu().numpy() if rowmap is not None else numpy.arange(yN)
        off1 = -5 * xA
        got = core.prepare_facet_columns(bands, off0s, (0, yN), off1, rowmap, n_rows)
        assert got.dtype == torch.complex128 and tuple(got.shape) == (F, n_rows, m)
        got = got.cpu().numpy()
        for f in range(F):
            win = ref.extract_from_facet(logical[f], off1, axis=1)  # [yB0, m]
            want = ref.prepare_facet(win / ref.facet_window(yB0)[:, None], off0s[f], axis=0)  # window NOT applied
            keep = rm >= 0
            assert _maxrel(got[f][rm[keep]], want[keep]) <= C128_TOL, (use_rowmap, f)


def _G_want(ref, C, off0):
    """Fn * cfft_m(C, axis 0) rotated by the facet offset, without placement: rows of add_to_subgrid(axis 0)."""
    m, xM = ref.xM_yN_size, ref.xM_size
    placed = ref.add_to_subgrid(C, off0, axis=0)
    sp = off0 * xM // ref.N
    return placed[(numpy.arange(m) + xM // 2 - m // 2 + sp) % xM]


def test_transform_contributions_c128():
    import torch

    core, ref = _cores(SMALL)
    m, yN, N = core.xM_yN_size, SMALL["yN_size"], SMALL["N"]
    rng = numpy.random.default_rng(33)
    fstep, sstep = core.facet_off_step, core.subgrid_off_step
    foffs = [0, 88 * fstep, -40 * fstep]
    soffs = [0, 96 * sstep, -17 * sstep, N // 2 + 10 * sstep]
    F, S = len(foffs), len(soffs)
    rowmap, n_rows = core.subgrid_column_rows(soffs)
    rm = rowmap.cpu().numpy()
    full = _crandn(rng, (F, yN, m))
    compact = numpy.zeros((F, n_rows, m), dtype=complex)
    compact[:, rm[rm >= 0]] = full[:, rm >= 0]
    G1 = core.transform_contributions(torch.from_numpy(compact).cuda(), 1, foffs, soffs, rowmap=rowmap)
    assert G1.dtype == torch.complex128
    G1 = G1.cpu().numpy()
    for f in range(F):
        for b in range(S):
            want = _G_want(ref, ref.extract_from_facet(full[f], soffs[b], axis=0), foffs[f])
            assert _maxrel(G1[f, b], want) <= C128_TOL, (f, b)
    contrib = _crandn(rng, (F, S, m, m))
    G2 = core.transform_contributions(torch.from_numpy(contrib).cuda(), 2, foffs, None, nsub=S).cpu().numpy()
    for f in range(F):
        for b in range(S):
            assert _maxrel(G2[f, b], _G_want(ref, contrib[f, b], foffs[f])) <= C128_TOL, (f, b)
    # layout 0 reads the complex64 column buffers of the reference schedule: refused in complex128
    with pytest.raises(NotImplementedError):
        core.transform_contributions(torch.zeros((1, m, yN), dtype=torch.complex128, device="cuda"), 0, [0], [0])


def test_sum_finish_facets_and_subgrid_side_c128():
    import torch

    core, ref = _cores(SMALL)
    m, xM, xA = core.xM_yN_size, SMALL["xM_size"], SMALL["xA_size"]
    rng = numpy.random.default_rng(34)
    fstep, sstep = core.facet_off_step, core.subgrid_off_step
    f_offs = [(0, 0), (0, 88 * fstep), (88 * fstep, 0), (88 * fstep, 88 * fstep), (-44 * fstep, 20 * fstep)]
    s_offs = [(0, 0), (40 * sstep, 96 * sstep), (-12 * sstep, -33 * sstep)]
    F, S = len(f_offs), len(s_offs)
    contrib = _crandn(rng, (F, S, m, m))
    G = core.transform_contributions(torch.from_numpy(contrib).cuda(), 2, [o[0] for o in f_offs], None, nsub=S)
    mask1 = (rng.random((S, xA)) > 0.2).astype(float)
    mask0 = (rng.random((S, xA)) > 0.2).astype(float)
    out = torch.empty((S, xM, xA), dtype=torch.complex128, device="cuda")
    core.sum_finish_facets(G, [o[0] for o in f_offs], [o[1] for o in f_offs], out, [s[1] for s in s_offs], xA,
                           mask=torch.from_numpy(mask1).cuda())
    got = out.cpu().numpy()
    tmp = torch.empty((S, xM, xA), dtype=torch.complex128, device="cuda")
    res = torch.empty((S, xA, xA), dtype=torch.complex128, device="cuda")
    core.wave_subgrid_side(G, [o[0] for o in f_offs], [o[1] for o in f_offs], [s[0] for s in s_offs],
                           [s[1] for s in s_offs], xA, torch.from_numpy(mask0).cuda(), torch.from_numpy(mask1).cuda(), tmp,
                           res)
    res = res.cpu().numpy()
    for b in range(S):
        acc = numpy.zeros((xM, xM), dtype=complex)
        for f, (o0, o1) in enumerate(f_offs):
            acc += ref.add_to_subgrid(ref.add_to_subgrid(contrib[f, b], o0, 0), o1, 1)
        want1 = numpy.array([ref.finish_subgrid(acc[r], s_offs[b][1], xA) for r in range(xM)]) * mask1[b][None, :]
        assert _maxrel(got[b], want1) <= C128_TOL, b
        want = numpy.array([ref.finish_subgrid(want1[:, c], s_offs[b][0], xA) for c in range(xA)]).T * mask0[b][:, None]
        assert _maxrel(res[b], want) <= C128_TOL, b


# ----------------------------------------------------------------------------------------------------- whole passes
def _forward(cfg, facet_cfgs, facets, plan, order, wave_axis, **kw):
    import ska_sdp_exec_swiftly_amd as sw

    fwd = sw.SwiftlyForward(cfg, list(zip(facet_cfgs, facets)), subgrid_configs=plan, wave_axis=wave_axis, **kw)
    assert fwd.wave_axis == wave_axis
    tasks = fwd.get_subgrid_tasks(order)
    if kw.get("delayed"):  # DeviceTask handles: compute() waits and copies to the host
        got = [numpy.asarray(t.compute()) for t in tasks]
    else:
        got = [t.cpu().numpy() for t in tasks]
    del fwd
    return got


def test_forward_small_full_cover():
    """full facet and subgrid covers (masks on both sides) of a small power-of-two configuration"""
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    p = SMALL
    cfg = sw.SwiftlyConfig(backend="hip", **p)
    facet_cfgs = sw.api.make_full_cover_config(p["N"], p["yB_size"], sw.FacetConfig)
    sg_cfgs = sw.api.make_full_cover_config(p["N"], p["xA_size"], sw.SubgridConfig)
    assert any(c.mask0 is not None for c in facet_cfgs) and any(c.mask1 is not None for c in sg_cfgs)
    vectors = [sep.facet_vectors(700 + j, p["yB_size"], rank=2) for j in range(len(facet_cfgs))]
    facets = [_facet128(v, c) for v, c in zip(vectors, facet_cfgs)]
    assert cfg.core.supports_band_pipeline(torch.complex128, len(facet_cfgs), explicit=True)

    by_off1 = sorted(sg_cfgs, key=lambda c: (c.off1, c.off0))
    got1 = _forward(cfg, facet_cfgs, facets, sg_cfgs, by_off1, 1)
    assert all(g.dtype == numpy.complex128 and g.shape == (p["xA_size"],) * 2 for g in got1)
    par = bench.verify_subgrids(p, facet_cfgs, vectors, by_off1, dict(enumerate(got1)), tol=PASS_TOL)
    print(f"small full cover complex128 wave_axis=1: relRMSE {par['rel_rmse']:.3e}")
    assert par["rel_rmse"] <= PASS_TOL, par
    got0 = _forward(cfg, facet_cfgs, facets, sg_cfgs, by_off1, 0)
    sched = max(_relrms(a, b) for a, b in zip(got1, got0))
    print(f"small full cover complex128 wave_axis=1 vs 0: relRMSE {sched:.3e}")
    assert sched <= SCHEDULE_TOL

    # shuffled requests (partial waves served from the result cache), prefetch off: bit-identical
    rng = numpy.random.default_rng(35)
    perm = rng.permutation(len(by_off1))
    shuffled = [by_off1[i] for i in perm]
    old = sw.api._PREFETCH
    try:
        for prefetch in (True, False):
            sw.api._PREFETCH = prefetch
            got = _forward(cfg, facet_cfgs, facets, sg_cfgs, shuffled, 1)
            for k, i in enumerate(perm):
                assert numpy.array_equal(got[k], got1[i]), (prefetch, k)
    finally:
        sw.api._PREFETCH = old
    # a partial wave without a plan, host-resident facets through the staging ring, delayed task handles
    part = [c for c in by_off1 if c.off1 == by_off1[0].off1][:2]
    host = [f.cpu().numpy() for f in facets]
    got = _forward(cfg, facet_cfgs, host, None, part, 1, delayed=True)
    for g, c in zip(got, part):
        assert numpy.array_equal(g, got1[by_off1.index(c)])


def _large_problem(name, n_sub):
    import ska_sdp_exec_swiftly_amd as sw

    p = ENTRIES[name]
    yB, xA = p["yB_size"], p["xA_size"]
    facet_cfgs = [sw.FacetConfig(0, 0, yB), sw.FacetConfig(yB, -yB, yB)]
    vectors = [sep.facet_vectors(300 + j, yB) for j in range(len(facet_cfgs))]
    offs = [(0, 0), (3 * xA, 0), (10 * xA, 2 * xA), (-7 * xA, 2 * xA), (20 * xA, -4 * xA), (40 * xA, 30 * xA)][:n_sub]
    sg_cfgs = [sw.SubgridConfig(o0, o1, xA) for o0, o1 in offs]
    return p, facet_cfgs, vectors, sg_cfgs


@pytest.mark.parametrize("name", list(ENTRIES))
def test_forward_large_matches_oracle(name):
    """2 facets; complex128 wave_axis=1 against the separable oracle and against wave_axis=0 (peak ~55 GB at 128k)"""
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    p, facet_cfgs, vectors, sg_cfgs = _large_problem(name, 6)
    cfg = sw.SwiftlyConfig(backend="hip", **p)
    assert cfg.core.supports_band_pipeline(torch.complex128, 2, explicit=True)
    facets = [_facet128(v, c) for v, c in zip(vectors, facet_cfgs)]
    order = sorted(sg_cfgs, key=lambda c: (c.off1, c.off0))
    got1 = _forward(cfg, facet_cfgs, facets, sg_cfgs, order, 1)
    assert all(g.dtype == numpy.complex128 for g in got1)
    par = bench.verify_subgrids(p, facet_cfgs, vectors, order, dict(enumerate(got1)), tol=PASS_TOL)
    print(f"{name} complex128 wave_axis=1: relRMSE {par['rel_rmse']:.3e} each {par['rel_rmse_each']}")
    assert par["rel_rmse"] <= PASS_TOL, par
    gc.collect()
    torch.cuda.empty_cache()
    got0 = _forward(cfg, facet_cfgs, facets, sg_cfgs, order, 0)
    sched = max(_relrms(a, b) for a, b in zip(got1, got0))
    print(f"{name} complex128 wave_axis=1 vs 0: relRMSE {sched:.3e}")
    assert sched <= SCHEDULE_TOL_W13


_CHUNK_CHILD = r"""
import sys, numpy, torch
sys.path[:0] = [sys.argv[2] + "/tests", sys.argv[2], sys.argv[3]]
import test_hip_c128_band_pipeline_gpu as t
import ska_sdp_exec_swiftly_amd as sw
p, facet_cfgs, vectors, sg_cfgs = t._large_problem("64k[1]-n16k-1k", 4)
cfg = sw.SwiftlyConfig(backend="hip", **p)
facets = [t._facet128(v, c) for v, c in zip(vectors, facet_cfgs)]
order = sorted(sg_cfgs, key=lambda c: (c.off1, c.off0))
numpy.save(sys.argv[1], numpy.stack(t._forward(cfg, facet_cfgs, facets, sg_cfgs, order, 1)))
"""


def test_forward_k2_chunked_bit_identical(tmp_path):
    """the chunked two-stream four-step of K2 (SWIFTLY_K2_CHUNK, read once per process: one child process each) gives
    the same bits as the plain one"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "ska-sdp-distributed-fourier-transform_amd")
    outs = []
    for chunk in ("0", "64,1"):
        path = str(tmp_path / f"chunk_{chunk.replace(',', '_')}.npy")
        env = dict(os.environ, SWIFTLY_K2_CHUNK=chunk)
        res = subprocess.run([sys.executable, "-c", _CHUNK_CHILD, path, root, pkg], env=env, cwd=root, timeout=600,
                             capture_output=True, text=True)
        assert res.returncode == 0, (chunk, res.returncode, res.stderr[-3000:])
        outs.append(numpy.load(path))
    assert outs[0].dtype == numpy.complex128
    assert numpy.array_equal(outs[0], outs[1])


# -------------------------------------------------------------------------------------------------------- defaults
def test_defaults_and_refusals():
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    for p in (SMALL, ENTRIES["64k[1]-n16k-1k"]):
        cfg = sw.SwiftlyConfig(backend="hip", **p)
        core = cfg.core
        assert sw.api.preferred_wave_axis(cfg, torch.complex128) == 0
        assert not core.supports_band_pipeline(torch.complex128)
        assert core.supports_band_pipeline(torch.complex128, explicit=True)
        assert core.supports_band_pipeline(torch.complex64) == core.supports_band_pipeline(torch.complex64, explicit=True)
    p = SMALL
    cfg = sw.SwiftlyConfig(backend="hip", **p)
    yB = p["yB_size"]
    fc = [sw.FacetConfig(0, 0, yB)]
    facet = torch.zeros((yB, yB), dtype=torch.complex128, device="cuda")
    plan = [sw.SubgridConfig(0, 0, p["xA_size"])]
    assert sw.SwiftlyForward(cfg, [(fc[0], facet)], subgrid_configs=plan).wave_axis == 0
    # mixed dtypes
    with pytest.raises(ValueError):
        sw.SwiftlyForward(cfg, [(fc[0], facet), (sw.FacetConfig(yB, 0, yB), facet.to(torch.complex64))], wave_axis=1)
    # too many facets
    many = [(sw.FacetConfig(0, 0, yB), facet)] * 65
    fwd = sw.SwiftlyForward(cfg, many, wave_axis=1)
    with pytest.raises(ValueError):
        fwd.get_subgrid_task(plan[0])
    # unsupported sizes: yN = 65536, (m, xM) = (512, 2048) and m = 1024 have no complex128 band pipeline
    for W, N, xA, xM, yB, yN in ((10.875, 131072, 928, 1024, 1024, 65536), (11.0, 16384, 1024, 2048, 2048, 4096),
                                 (11.0, 8192, 1024, 2048, 2048, 4096)):
        cfg = sw.SwiftlyConfig(backend="hip", W=W, fov=1.0, N=N, yB_size=yB, yN_size=yN, xA_size=xA, xM_size=xM)
        assert not cfg.core.supports_band_pipeline(torch.complex128, explicit=True), (N, xM, yN)
        small = torch.zeros((yB, yB), dtype=torch.complex128, device="cuda")
        fwd = sw.SwiftlyForward(cfg, [(sw.FacetConfig(0, 0, yB), small)], wave_axis=1)
        with pytest.raises(ValueError, match="complex128"):
            fwd.get_subgrid_task(sw.SubgridConfig(0, 0, xA))
