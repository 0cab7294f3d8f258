"""
Forward K2 on column slabs of the padded facet axis (ska_sdp_exec_swiftly_amd/slabs.py): the slab
path of SwiftlyForward gives the bits of the per-wave path while it transforms fewer columns, agrees with the separable
oracle, and its two native forms -- K2 on a column range, K3 from two pieces -- equal the whole-window forms bit for bit.

The small problem of test_hip_band_pipeline_gpu.py (yN = 32768, m = 512, three facets of 352 rows) with a plan of eight
subgrid columns i1:  0 and 32 (p = 0: one slab, one piece of zero width);  3, 4, 5 (neighbours that share columns; p =
368, 320, 272 -- 368 and 272 put a 32-column tile of K3 across the piece boundary);  9 (the slabs between 5 and 9 are
never computed);  70, 0, 1 (the wrap of the cyclic axis: 70 overlaps 0 by 224 columns).  The i0 sets differ, so the slab
row maps are real unions.
"""
import numpy
import pytest

import bench
from oracle import separable as sep
from oracle import swiftly_oracle as orc

pytestmark = pytest.mark.gpu

W64, N64, xM64, yN64, yB, xA, M = 10.875, 65536, 1024, 32768, 352, 928, 512
SEED = 141
PLAN = {0: (0, 2), 1: (0, 2), 3: (0, 2, 69), 4: (0, 2), 5: (0,), 9: (0, 2, 69), 32: (0, 2), 70: (0, 2, 69)}  # i1: i0s

_cache = {}


def relrms(a, b):
    return float(numpy.sqrt(numpy.mean(numpy.abs(a - b) ** 2) / numpy.mean(numpy.abs(b) ** 2)))


def problem():
    """(torch, sw, cfg, facet_cfgs, facets, plan in ascending wave order, {off1: subgrids}) -- built once"""
    if "p" not in _cache:
        import torch

        import ska_sdp_exec_swiftly_amd as sw

        P = dict(W=W64, fov=1.0, N=N64, yB_size=yB, yN_size=yN64, xA_size=xA, xM_size=xM64)
        cfg = sw.SwiftlyConfig(backend="hip", **P)
        if not cfg.core.supports_band_pipeline(torch.complex64):
            pytest.skip("band pipeline not available")
        fstep = cfg.facet_off_step
        facet_cfgs = [sw.FacetConfig(o0, o1, yB) for o0, o1 in ((0, 0), (0, 50 * fstep), (-70 * fstep, 0))]
        vectors = [sep.facet_vectors(SEED + j, yB, rank=2) for j in range(len(facet_cfgs))]
        facets = [bench.separable_facet(torch, vectors[j], c) for j, c in enumerate(facet_cfgs)]
        plan = [sw.SubgridConfig(i0 * xA, i1 * xA, xA) for i1 in sorted(PLAN) for i0 in PLAN[i1]]
        waves = {}
        for c in plan:
            waves.setdefault(c.off1, []).append(c)
        _cache["p"] = (torch, sw, cfg, facet_cfgs, facets, plan, waves)
    return _cache["p"]


def run_waves(keys, slabs_on, prefetch, **kwargs):
    """``({off1: finished subgrids of the wave}, K2 columns per facet issued, forward object)`` for ``get_wave`` over
    ``keys``"""
    torch, sw, cfg, facet_cfgs, facets, plan, waves = problem()
    old = sw.api._K2_SLABS, sw.api._PREFETCH
    sw.api._K2_SLABS, sw.api._PREFETCH = slabs_on, prefetch
    try:
        fwd = sw.SwiftlyForward(cfg, list(zip(facet_cfgs, facets)), subgrid_configs=plan, wave_axis=1, **kwargs)
        before = cfg.core.k2_columns_issued
        out = {k: fwd.get_wave(waves[k]).cpu().numpy() for k in keys}
        columns = cfg.core.k2_columns_issued - before
    finally:
        sw.api._K2_SLABS, sw.api._PREFETCH = old
    torch.cuda.synchronize()
    return out, columns, fwd


def per_wave_reference(prefetch):
    """the per-wave path's subgrids of every planned wave and its K2 columns (once per prefetch setting)"""
    key = ("ref", prefetch)
    if key not in _cache:
        waves = problem()[6]
        out, columns, fwd = run_waves(sorted(waves), False, prefetch)
        assert columns >= len(waves) * M and not fwd._slab_lru._items and not fwd._slab_kept
        _cache[key] = (out, columns)
    return _cache[key]


def ordered(order):
    keys = sorted(problem()[6])  # i1 = 0, 1, 3, 4, 5, 9, 32, 70
    if order == "descending":
        return keys[::-1]
    if order == "shuffled":
        return [keys[i] for i in (5, 3, 2, 7, 0, 6, 4, 1)]  # 9, 4, 3, 70, 0, 32, 5, 1
    return keys


@pytest.mark.parametrize("prefetch", [False, True])
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_slab_path_is_bit_identical_to_the_per_wave_path(order, prefetch):
    """get_wave with api._K2_SLABS on gives the bits of the per-wave path in any wave order, with and without the
    prefetch, and hands fewer columns to K2 than the per-wave path asked for in the same order (a wrong prediction of the
    prefetch wastes a K2 in either path)."""
    keys = ordered(order)
    want, wave_columns, _ = run_waves(keys, False, prefetch)
    for k in keys:  # (and the per-wave path itself does not depend on the order)
        assert numpy.array_equal(want[k], per_wave_reference(prefetch)[0][k]), (order, prefetch, k)
    got, columns, fwd = run_waves(keys, True, prefetch)
    print(f"K2 columns per facet: per wave {wave_columns}, slabs {columns} ({order}, prefetch {prefetch}, "
          f"{fwd.prefetch_issued} prefetched K2 calls)")
    for k in keys:
        assert numpy.array_equal(got[k], want[k]), (order, prefetch, k)
    assert (fwd.prefetch_issued > 0) == prefetch
    assert not fwd.lru._items  # no per-wave Q: the slab path really ran
    assert columns < wave_columns, (columns, wave_columns)
    if not prefetch:  # without wasted predictions every planned column is computed exactly once in these orders
        assert wave_columns == len(keys) * M and columns == fwd._slab_plan.columns() == 3728


def test_slab_path_serves_the_reference_access_pattern():
    """the off0-major, one-subgrid-at-a-time loop over the plan: one launch sequence per off1 wave, the same bits"""
    torch, sw, cfg, facet_cfgs, facets, plan, waves = problem()
    want, _ = per_wave_reference(True)
    assert sw.api._K2_SLABS
    fwd = sw.SwiftlyForward(cfg, list(zip(facet_cfgs, facets)), subgrid_configs=plan)
    assert fwd.wave_axis == 1
    calls = []
    inner = fwd.get_wave
    fwd.get_wave = lambda sgs, timer=None: (calls.append(sgs[0].off1), inner(sgs, timer))[1]
    loop = sorted(plan, key=lambda c: (c.off0 % N64, c.off1))
    got = [fwd.get_subgrid_task(c).cpu().numpy() for c in loop]
    assert sorted(calls) == sorted(waves)  # every wave once
    assert not fwd._results and fwd._result_bytes == 0 and not fwd.lru._items and fwd._slab_lru._items
    for g, c in zip(got, loop):
        assert numpy.array_equal(g, want[c.off1][waves[c.off1].index(c)]), (c.off0, c.off1)


def test_slab_path_matches_the_separable_oracle():
    torch, sw, cfg, facet_cfgs, facets, plan, waves = problem()
    got, _, _ = run_waves([70 * xA, 4 * xA], True, True)
    so = sep.SeparableOracle(orc.OracleCore(W64, N64, xM64, yN64), [orc.CoverItem(c.off0, c.off1, c.size) for c in facet_cfgs],
                             [sep.facet_vectors(SEED + j, yB, rank=2) for j in range(3)])
    for off1, k in ((70 * xA, 2), (4 * xA, 1)):  # subgrids (69, 70) and (2, 4)
        c = waves[off1][k]
        rel = relrms(got[off1][k], so.subgrid(orc.CoverItem(c.off0, c.off1, c.size)))
        print(f"subgrid ({c.off0 // xA}, {c.off1 // xA}): relative RMSE vs oracle {rel:.3e}")
        assert rel < 2e-5, (c.off0, c.off1, rel)


def test_lru_forward_1_serves_the_whole_plan():
    """the slab cache holds the two slabs of a wave whatever the user's LRU size is"""
    want, _ = per_wave_reference(True)
    keys = ordered("ascending")
    got, columns, fwd = run_waves(keys, True, True, lru_forward=1)
    assert fwd._slab_lru.cache_size == 2
    for k in keys:
        assert numpy.array_equal(got[k], want[k]), k


# -- the native forms on their own ------------------------------------------------------------------------------------
def bands_of_plan():
    """(core, band buffers [F, yB, band columns], band, facet off0s) of the problem's facets for the plan's band"""
    if "bands" not in _cache:
        torch, sw, cfg, facet_cfgs, facets, plan, waves = problem()
        core = cfg.core
        band = core.band_for_offsets(sorted(waves))
        bands = torch.empty((len(facets), yB, core.band_columns(band)), dtype=torch.complex64, device=core.device)
        for j, c in enumerate(facet_cfgs):
            core.prepare_facet_band(facets[j], c.off1, band, out=bands[j])
        _cache["bands"] = (core, bands, band, [c.off0 for c in facet_cfgs])
    return _cache["bands"]


@pytest.mark.parametrize("off1,first,count", [(5 * xA, 272, 240), (5 * xA, 0, 448), (4 * 1024, 272, 240), (3 * 1024, 0, 512),
                                              (70 * xA, 208, 64)])
def test_k2_on_a_column_range_equals_the_columns_of_the_whole_window(off1, first, count):
    """(wave 5: a rotated window, un-chunked and chunked widths; slabs 4 and 3: the pseudo-waves; wave 70: across the
    wrap of the window's rotation)"""
    torch = problem()[0]
    core, bands, band, off0s = bands_of_plan()
    rowmap, n_rows = core.subgrid_column_rows([0, 2 * xA])
    full = core.prepare_facet_columns(bands, off0s, band, off1, rowmap, n_rows)
    fill = complex(7.0, -3.0)
    out = torch.full((len(off0s), n_rows, M), fill, dtype=torch.complex64, device=core.device)
    before = core.k2_columns_issued
    core.prepare_facet_columns_range(bands, off0s, band, off1, first, count, out, rowmap)
    assert core.k2_columns_issued - before == count
    out, full = out.cpu().numpy(), full.cpu().numpy()
    assert numpy.array_equal(out[:, :, first:first + count], full[:, :, first:first + count])
    rest = numpy.delete(out, numpy.s_[first:first + count], axis=2)
    assert rest.size == out.size - out.shape[0] * out.shape[1] * count and numpy.all(rest == numpy.complex64(fill))


def test_k2_column_range_outside_the_band_is_refused():
    torch = problem()[0]
    core, bands, band, off0s = bands_of_plan()
    rowmap, n_rows = core.subgrid_column_rows([0])
    out = torch.zeros((len(off0s), n_rows, M), dtype=torch.complex64, device=core.device)
    # slab 63 holds the first 288 columns of wave 70 at positions [224, 512); positions below 192 lie in front of the band
    core.prepare_facet_columns_range(bands, off0s, band, 63 * 1024, 224, 288, out, rowmap)
    torch.cuda.synchronize()
    kept = out.clone()
    for first, count in ((0, 512), (176, 336), (0, 16)):
        with pytest.raises(ValueError):
            core.prepare_facet_columns_range(bands, off0s, band, 63 * 1024, first, count, out, rowmap)
    with pytest.raises(ValueError):  # slab 40 lies in the gap of the band
        core.prepare_facet_columns_range(bands, off0s, band, 40 * 1024, 0, 512, out, rowmap)
    for first, count in ((8, 16), (0, 24), (496, 32), (0, 0)):  # not multiples of 16 / past the window / empty
        with pytest.raises(ValueError):
            core.prepare_facet_columns_range(bands, off0s, band, 4 * xA, first, count, out, rowmap)
    torch.cuda.synchronize()
    assert torch.equal(out, kept)  # nothing was computed


@pytest.mark.parametrize("i1", [3, 5, 70, 32])
def test_k3_from_two_pieces_equals_k3_on_the_assembled_window(i1):
    """the pieces live in slabs with row maps of their own (supersets of the wave's rows, different from each other)"""
    from ska_sdp_exec_swiftly_amd import slabs

    torch = problem()[0]
    core, bands, band, off0s = bands_of_plan()
    off1, sub_off0s = i1 * xA, [0, 2 * xA]
    wave_map, wave_rows = core.subgrid_column_rows(sub_off0s)
    slab_rows = [core.subgrid_column_rows([0, 2 * xA, 69 * xA]), core.subgrid_column_rows([0, 2 * xA, 5 * xA])]
    pieces = []
    rows = torch.nonzero(wave_map >= 0).flatten()
    assembled = torch.zeros((len(off0s), wave_rows, M), dtype=torch.complex64, device=core.device)
    for (j, first, count), (rowmap, n_rows) in zip(slabs.wave_pieces(N64, yN64, M, off1), slab_rows):
        Q = torch.full((len(off0s), n_rows, M), float("nan"), dtype=torch.complex64, device=core.device)
        core.prepare_facet_columns_range(bands, off0s, band, slabs.slab_off1(N64, yN64, M, j), first, count, Q, rowmap)
        pieces.append((Q, rowmap, n_rows, first, count))
        assembled[:, wave_map[rows].long(), first:first + count] = Q[:, rowmap[rows].long(), first:first + count]
    assert len(pieces) == (1 if i1 == 32 else 2)
    want = core.transform_contributions(assembled, 1, off0s, sub_off0s, rowmap=wave_map)
    got = torch.full_like(want, float("nan"))
    core.transform_contributions_pieces(pieces, off0s, sub_off0s, got)
    assert not torch.isnan(torch.view_as_real(got)).any()
    assert numpy.array_equal(got.cpu().numpy(), want.cpu().numpy())
    # and the assembled window is the wave's own Q
    Qw = core.prepare_facet_columns(bands, off0s, band, off1, wave_map, wave_rows)
    assert torch.equal(Qw, assembled)
    # the placed output form of wave_facet_side (a flat send buffer) takes the same pieces
    F, S = len(off0s), len(sub_off0s)
    flat = torch.zeros(F * S * M * M + 64, dtype=torch.complex64, device=core.device)
    layout = ([64 + b * F * M * M for b in range(S)], [M * M] * S)  # subgrid-major: block (f, b) at 64 + (b*F + f) * m*m
    core.transform_contributions_pieces(pieces, off0s, sub_off0s, flat, g_layout=layout)
    assert torch.equal(flat[64:].view(S, F, M, M).transpose(0, 1), want) and not flat[:64].any()
    # pieces that do not make up the window are refused
    with pytest.raises(ValueError):
        core.transform_contributions_pieces(pieces[:1] if len(pieces) == 2 else [(*pieces[0][:3], 0, 256)], off0s, sub_off0s, got)
