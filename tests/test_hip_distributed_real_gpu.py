"""
Real-valued facets through the multi-GPU classes (``DistributedForward(facet_dtype=torch.float32, half_length_k1=...)``,
``DistributedBackward(facet_dtype=torch.float32, half_length_finish=...)``) as virtual ranks of one process, and the round
trip from ``DeviceSources.facet(float32)`` to ``DeviceSources.check_facets``.

The problem is the small-rows problem of tests/test_hip_band_pipeline_gpu.py (3 facets of 352^2, 12 subgrids in 4 waves, yN
32768) with the real separable facets of tests/test_hip_real_rfft_gpu.py; the exchange is that file's in-process
``_virtual_all_to_all``.  World 2: two whole facets and one cooperative facet; world 8: all three cooperative, in row blocks of
40 and 48 rows -- the smallest shapes at which the local K1, the cooperative K1 on a row block at a non-zero ``row0`` and the
cooperative finish all run.

Expected values and bounds:

* the real-load K1 and the real store give the bits of the promoted facets / of the real parts (the project's guarantee for
  these forms): ``torch.equal`` against the same-world pass without the keywords, no tolerance;
* the half-length K1: every subgrid against ``sep.SeparableOracle`` within the whole-pass bound of
  ``test_hip_real_rfft_gpu.py::test_forward_half_length_k1`` (relative RMSE < 2e-5);
* the half-length finish: every facet against the real-store pass on the same accumulators within the per-facet bound of
  ``test_hip_real_out_c2r_gpu.py::test_backward_half_length_finish`` (relative RMSE < 2 * f32_bound(15): each form is within
  one bound of the exact transform).

The passes without the keywords and the oracle's subgrids are computed once per world and shared, unchanged.
"""
import functools

import numpy
import pytest

from _band_sweep_worker import cores, f32_bound, last_instance, relrms
from oracle import separable as sep
from oracle import swiftly_oracle as orc
from test_hip_band_pipeline_gpu import _virtual_all_to_all
from test_hip_real_rfft_gpu import _real_problem

pytestmark = pytest.mark.gpu

WORLDS = [2, 8]
HALF_FINISH_BOUND = 2 * f32_bound(15)


@functools.lru_cache(maxsize=None)
def problem():
    """(torch, sw, cfg, facet_cfgs, vectors, float32 facets, promoted complex64 facets, sg_cfgs, waves by off1)"""
    torch, sw, cfg, facet_cfgs, vectors, reals, sg_cfgs, _ = _real_problem(47)
    assert cfg.core.supports_band_pipeline(torch.complex64) and cfg.core.supports_backward_band(torch.complex64)
    waves = {}
    for c in sg_cfgs:
        waves.setdefault(int(c.off1), []).append(c)
    return torch, sw, cfg, facet_cfgs, vectors, reals, [r.to(torch.complex64) for r in reals], sg_cfgs, waves


def forward_pass(world, facets, **kw):
    """one forward pass over virtual ranks: ``(objects, {cooperative facet: pack_coop send buffers by rank},
    {(off0, off1): subgrid})``"""
    from ska_sdp_exec_swiftly_amd.distributed import DistributedForward

    torch, _, cfg, facet_cfgs, _, _, _, sg_cfgs, waves = problem()
    fwds = [DistributedForward(cfg, facet_cfgs, facets, subgrid_configs=sg_cfgs, wave_axis=1, dtype=torch.complex64,
                               rank_world=(r, world), **kw) for r in range(world)]
    sh = fwds[0].sharding
    assert sh.coop == ([2] if world == 2 else [0, 1, 2])
    for f in fwds:
        f.prepare_all_facets()
    sends = {}
    for j in sh.coop:
        packed = [f.pack_coop(j) for f in fwds]
        sends[j] = [p[0] for p in packed]
        recvs = _virtual_all_to_all(sends[j], [p[1] for p in packed])
        for r, f in enumerate(fwds):
            assert recvs[r].numel() == sum(packed[r][2])
            f.unpack_coop(j, recvs[r])
    out = {}
    for wave in waves.values():
        packed = [f.pack_wave(wave) for f in fwds]
        recvs = _virtual_all_to_all([p[0] for p in packed], [p[1] for p in packed])
        for r, f in enumerate(fwds):
            mine, res = f.unpack_wave(wave, recvs[r])
            for k, i in enumerate(mine):
                out[(wave[i].off0, wave[i].off1)] = res[k].clone()
    assert len(out) == len(sg_cfgs)
    return fwds, sends, out


def backward_pass(world, subgrids, wave_axis=1, **kw):
    """one backward pass over virtual ranks: ``(objects, {facet: tensor, cooperative pieces concatenated}, all
    coop_pieces blocks)``"""
    from ska_sdp_exec_swiftly_amd.distributed import DistributedBackward

    torch, _, cfg, facet_cfgs, _, _, _, sg_cfgs, _ = problem()
    waves = {}
    for c in sg_cfgs:
        waves.setdefault(int(c.off1 if wave_axis == 1 else c.off0), []).append(c)
    plan = dict(subgrid_configs=sg_cfgs) if wave_axis == 1 else {}
    bwds = [DistributedBackward(cfg, facet_cfgs, wave_axis=wave_axis, dtype=torch.complex64, rank_world=(r, world), **plan, **kw)
            for r in range(world)]
    sh = bwds[0].sharding
    assert sh.coop == (([2] if world == 2 else [0, 1, 2]) if wave_axis == 1 else [])
    for wave in waves.values():
        data = [subgrids[(c.off0, c.off1)] for c in wave]
        packed = [b.pack_wave(wave, [data[i] for i in b.subgrids_of(wave)]) for b in bwds]
        recvs = _virtual_all_to_all([p[0] for p in packed], [p[1] for p in packed])
        for r, b in enumerate(bwds):
            assert recvs[r].numel() == sum(packed[r][2])
            b.unpack_wave(wave, recvs[r])
    done, pieces = {}, []
    for b in bwds:
        idx, out = b.finish()
        done.update(zip(idx, out))
    for j in sh.coop:
        packed = [b.pack_coop_finish(j) for b in bwds]
        recvs = _virtual_all_to_all([p[0] for p in packed], [p[1] for p in packed])
        rows = []
        for r, b in enumerate(bwds):
            jj, row0, piece = b.unpack_coop_finish(j, recvs[r])
            assert jj == j and row0 == sh.coop_rows(facet_cfgs[j].size, r)[0]
            rows.append(piece)
        pieces += rows
        done[j] = torch.cat(rows)
    assert sorted(done) == list(range(len(facet_cfgs)))
    return bwds, done, pieces


@functools.lru_cache(maxsize=None)
def forward_today(world):
    """the pass without the keywords on the promoted complex64 facets"""
    return forward_pass(world, problem()[6])


@functools.lru_cache(maxsize=None)
def forward_real_load(world):
    torch, reals = problem()[0], problem()[5]
    return forward_pass(world, reals, facet_dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def backward_today(world, wave_axis):
    return backward_pass(world, forward_today(2)[2], wave_axis)


@functools.lru_cache(maxsize=None)
def backward_real_store(world):
    return backward_pass(world, forward_today(2)[2], 1, facet_dtype=problem()[0].float32)


@functools.lru_cache(maxsize=None)
def oracle_subgrids():
    _, _, _, facet_cfgs, vectors, _, _, sg_cfgs, _ = problem()
    so = sep.SeparableOracle(cores("c15")[1], [orc.CoverItem(c.off0, c.off1, c.size) for c in facet_cfgs], vectors)
    return {(c.off0, c.off1): so.subgrid(orc.CoverItem(c.off0, c.off1, c.size)) for c in sg_cfgs}


def same(a, b):
    """two passes' buffers, key by key: bit-identical"""
    import torch

    assert sorted(a) == sorted(b)
    pairs = []
    for key in a:
        if isinstance(a[key], list):  # (send buffers by rank)
            assert len(a[key]) == len(b[key])
            pairs += list(zip(a[key], b[key]))
        else:
            pairs.append((a[key], b[key]))
    return all(x.shape == y.shape and torch.equal(x, y) for x, y in pairs)


# ------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("world", WORLDS)
def test_forward_real_load_gives_the_bits_of_the_promoted_facets(world):
    torch = problem()[0]
    fwds0, sends0, out0 = forward_today(world)
    fwds, sends, out = forward_real_load(world)
    assert all(f.facet_dtype == torch.complex64 and f.half_length_k1 is False for f in fwds0)
    # every rank holds data: rows of the cooperative facets, at world 2 a whole facet too
    assert all(f.facet_dtype == torch.float32 and f.half_length_k1 is False for f in fwds)
    if world == 2:
        assert all(f.local.facet_dtype == torch.float32 and type(f.local).__name__ == "SwiftlyForward" for f in fwds)
        assert all(type(f.local).__name__ == "_PromotingForward" for f in fwds0)
    assert all(s.dtype == torch.complex64 for ss in sends.values() for s in ss)
    assert same(sends, sends0), "a pack_coop send buffer differs from the promoted pass"
    assert same(out, out0), "a subgrid differs from the promoted pass"
    assert all(o.dtype == torch.complex64 and bool(o.abs().max() > 0) for o in out.values())


@pytest.mark.parametrize("world", WORLDS)
def test_forward_half_length_k1(world):
    torch, reals = problem()[0], problem()[5]
    _, sends_r, out_r = forward_real_load(world)
    want = oracle_subgrids()
    before, _ = last_instance()
    fwds, sends, out = forward_pass(world, reals, facet_dtype=torch.float32, half_length_k1=True)
    assert last_instance()[0] == before, "a K1 went through the band row kernel: the real-load form ran"
    assert all(f.half_length_k1 is True and f.facet_dtype == torch.float32 for f in fwds)
    worst = 0.0
    for key, g in out.items():
        assert g.dtype == torch.complex64
        worst = max(worst, relrms(g.cpu().numpy(), want[key]))
    print(f"distributed half-length K1, world {world}: worst subgrid relative RMSE {worst:.3e} (bound 2e-5)")
    assert worst < 2e-5, worst
    assert not same(out, out_r), "the half-length form rounds differently: did it run?"
    assert not same(sends, sends_r)


@pytest.mark.parametrize("world", WORLDS)
def test_forward_odd_pitch_runs_the_real_load_form(world):
    """facets (and with them every cooperative row block) at an odd pitch cannot be loaded as pairs: the objects say so and
    give the real-load bits"""
    torch, reals = problem()[0], problem()[5]
    views = []
    for r in reals:
        big = torch.zeros((r.shape[0], r.shape[1] + 3), dtype=torch.float32, device="cuda")
        big[:, : r.shape[1]] = r
        views.append(big[:, : r.shape[1]])
    assert all(v.stride(0) % 2 == 1 for v in views)
    _, sends_r, out_r = forward_real_load(world)
    fwds, sends, out = forward_pass(world, views, facet_dtype=torch.float32, half_length_k1=True)
    assert all(f.half_length_k1 is False and f.facet_dtype == torch.float32 for f in fwds)
    assert same(sends, sends_r) and same(out, out_r)


# ----------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("world", WORLDS)
def test_backward_real_store_is_the_real_part(world):
    torch = problem()[0]
    bwds0, done0, pieces0 = backward_today(world, 1)
    bwds, done, pieces = backward_real_store(world)
    assert all(b.facet_dtype == torch.complex64 and b.real_finish_native is False and b.half_length_finish is False for b in bwds0)
    assert all(b.facet_dtype == torch.float32 and b.real_finish_native is True and b.half_length_finish is False for b in bwds)
    assert len(pieces) == len(pieces0) == world * len(bwds[0].sharding.coop)
    assert all(p.dtype == torch.float32 for p in pieces) and all(d.dtype == torch.float32 for d in done.values())
    assert all(p.dtype == torch.complex64 for p in pieces0)
    for p, p0 in zip(pieces, pieces0):
        assert tuple(p.shape) == tuple(p0.shape) and torch.equal(p, p0.real)
    for j, d in done.items():
        assert tuple(d.shape) == (352, 352) and bool(d.abs().max() > 0)
        assert torch.equal(d, done0[j].real), j


def test_backward_reference_schedule_copies_the_real_part():
    """``wave_axis=0`` (the class's default; no cooperative facets): no native real store, the facets are float32 all the same"""
    torch = problem()[0]
    _, done0, _ = backward_today(2, 0)
    bwds, done, pieces = backward_pass(2, forward_today(2)[2], 0, facet_dtype=torch.float32)
    assert not pieces
    assert all(b.real_finish_native is False and b.half_length_finish is False and b.facet_dtype == torch.float32 for b in bwds)
    for j, d in done.items():
        assert d.dtype == torch.float32 and bool(d.abs().max() > 0)
        assert torch.equal(d, done0[j].real), j


@pytest.mark.parametrize("world", WORLDS)
def test_backward_half_length_finish(world):
    torch = problem()[0]
    _, done_r, pieces_r = backward_real_store(world)
    bwds, done, pieces = backward_pass(world, forward_today(2)[2], 1, facet_dtype=torch.float32, half_length_finish=True)
    assert all(b.half_length_finish is True and b.real_finish_native is True and b.facet_dtype == torch.float32 for b in bwds)
    assert all(p.dtype == torch.float32 for p in pieces)
    worst = 0.0
    for j, d in done.items():
        assert d.dtype == torch.float32 and tuple(d.shape) == tuple(done_r[j].shape)
        worst = max(worst, relrms(d.cpu().numpy().astype(float), done_r[j].cpu().numpy().astype(float)))
    print(f"distributed half-length finish, world {world}: worst facet relative RMSE against the real-store pass {worst:.3e} "
          f"(bound {HALF_FINISH_BOUND:.2e})")
    assert worst < HALF_FINISH_BOUND, worst
    assert not all(torch.equal(done[j], done_r[j]) for j in done), "the half-length form rounds differently: did it run?"
    assert not all(torch.equal(p, q) for p, q in zip(pieces, pieces_r))


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_with_a_real_config(monkeypatch):
    from ska_sdp_exec_swiftly_amd import api
    from ska_sdp_exec_swiftly_amd.distributed import DistributedBackward, DistributedForward

    torch, _, cfg, facet_cfgs, _, reals, promoted, sg_cfgs, _ = problem()

    class Untouchable:
        """stands in for the configuration: any attribute access is a failure"""

        def __getattr__(self, name):
            raise AssertionError(f"the constructor touched the configuration ({name}) before refusing the keyword")

    with pytest.raises(ValueError, match="facet_dtype must be float32 or None"):
        DistributedForward(cfg, facet_cfgs, reals, facet_dtype=torch.complex64, rank_world=(0, 2))
    # ... and refuses first: before the configuration is looked at, before a SwiftlyForward is constructed
    built = []
    real_init = api.SwiftlyForward.__init__
    monkeypatch.setattr(api.SwiftlyForward, "__init__", lambda self, *a, **k: (built.append(1), real_init(self, *a, **k))[1])
    for kw in (dict(facet_dtype=torch.complex64), dict(half_length_k1=True)):
        with pytest.raises(ValueError, match="float32"):
            DistributedForward(Untouchable(), facet_cfgs, reals, rank_world=(0, 2), **kw)
    for kw in (dict(half_length_finish=True), dict(facet_dtype=torch.float64), dict(facet_dtype=torch.float16)):
        with pytest.raises(ValueError, match="facet_dtype"):
            DistributedBackward(Untouchable(), facet_cfgs, rank_world=(0, 2), **kw)
    assert not built
    # float32 asked for complex facets: nothing to keep real, the object runs what it runs without the keyword
    fwd = DistributedForward(cfg, facet_cfgs, promoted, subgrid_configs=sg_cfgs, wave_axis=1, dtype=torch.complex64,
                             rank_world=(0, 2), facet_dtype=torch.float32, half_length_k1=True)
    assert fwd.facet_dtype == torch.complex64 and fwd.half_length_k1 is False
    assert type(fwd.local).__name__ == "_PromotingForward"


# ------------------------------------------------------------------------------------------------------ round trip
def test_round_trip_from_sources_without_a_complex_facet():
    """``DeviceSources.facet(float32)`` -> ``DistributedForward(facet_dtype=float32)`` -> ``check_subgrids`` ->
    ``DistributedBackward(facet_dtype=float32, wave_axis=1)`` -> ``check_facets``, world 2.

    tests/test_hip_sources_gpu.py has complex128 bounds only for its round trip, so the yardstick is the complex64 pass
    without the keywords on the same inputs, measured here: forward ``torch.equal``, backward equal to its real parts --
    and therefore the same figures from the device checks, which are printed.  (The 12 subgrids are not a cover: the
    finished facets are what those subgrids carry of the image, so the facet figures measure the plan, not the kernels.)"""
    import ska_sdp_exec_swiftly_amd as sw

    torch, _, cfg, facet_cfgs, _, _, _, sg_cfgs, _ = problem()
    rng = numpy.random.default_rng(12)
    sources = []
    for fc in facet_cfgs:  # 12 sources inside every facet
        for _ in range(12):
            p0, p1 = (int(v) for v in rng.integers(-fc.size // 2 + 8, fc.size // 2 - 8, size=2))
            sources.append((float(rng.uniform(0.5, 2.0)), fc.off0 + p0, fc.off1 + p1))
    dsrc = sw.DeviceSources(sources, cfg.image_size)
    reals = [dsrc.facet(fc, dtype=torch.float32) for fc in facet_cfgs]
    assert all(r.dtype == torch.float32 and int((r != 0).sum()) >= 12 for r in reals)
    fwds, _, out = forward_pass(2, reals, facet_dtype=torch.float32)
    _, _, out0 = forward_pass(2, [r.to(torch.complex64) for r in reals])
    assert all(f.facet_dtype == torch.float32 for f in fwds)
    assert same(out, out0)
    errs = dsrc.check_subgrids(sg_cfgs, torch.stack([out[(c.off0, c.off1)] for c in sg_cfgs]))
    assert tuple(errs.shape) == (len(sg_cfgs), 2) and bool(torch.isfinite(errs).all()) and bool((errs[:, 1] > 0).all())
    print(f"round trip: worst subgrid RMSE / truth RMS {float((errs[:, 0] / errs[:, 1]).max()):.3e}")
    bwds, done, _ = backward_pass(2, out, 1, facet_dtype=torch.float32)
    _, done0, _ = backward_pass(2, out0, 1)
    assert all(b.facet_dtype == torch.float32 and b.real_finish_native for b in bwds)
    facets = [done[j] for j in range(len(facet_cfgs))]
    assert all(f.dtype == torch.float32 and torch.equal(f, done0[j].real) for j, f in enumerate(facets))
    got = dsrc.check_facets(facet_cfgs, facets)
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(facet_cfgs), 2) and got.device == facets[0].device
    assert bool(torch.isfinite(got).all()) and bool((got[:, 1] > 0).all())
    assert torch.equal(got, dsrc.check_facets(facet_cfgs, [done0[j].real.contiguous() for j in range(len(facet_cfgs))]))
    print(f"round trip: facet RMSE / truth RMS {(got[:, 0] / got[:, 1]).cpu().numpy()}")
