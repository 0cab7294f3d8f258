"""
K2 of the axis-1-first order with the contiguous-axis finish inside the first pass of its four-step
(``swiftly_hip_prepare_facet_columns_axis1``, csrc/swiftly_colaxis1.h; ``SwiftlyConfig(axis1_first="k2")``) on the GPU.

The primitive, at both sizes with an instance, against
  (i)  the two calls it replaces on the same band buffers: ``finish_axis1_rows`` + ``prepare_facet_columns``;
  (ii) the complex128 oracle composition of tests/test_hip_band_pipeline_gpu.py: the ``Z`` rows of
       test_finish_axis1_rows_matches_oracle, then ``prepare_facet(., off0, axis=0)`` without its window as in
       test_prepare_facet_columns.
Both forms are float32 roundings of (ii); the new one may not be worse than the two calls by more than the margin
test_window_rows_store_of_the_whole_row_k1_matches_the_row_pass_per_wave gives two float32 roundings of one value
(``err_new <= 1.25 * err_parent + 1e-8``), nor than ``ABS_CAP`` = 1.5 x the largest ``err_parent`` of this file.

Then the refusals, the whole pass through ``SwiftlyForward`` against the separable oracle and against ``"rows"``, and two
in-process virtual ranks of the multi-GPU class.
"""
import pickle

import numpy
import pytest

import bench
from oracle import separable as sep
from oracle import swiftly_oracle as orc

pytestmark = pytest.mark.gpu

W64, N64, xM64, yN64 = 10.875, 65536, 1024, 32768   # core64() of tests/test_hip_band_pipeline_gpu.py: m = 512, n1 = 32
W32, N32, xM32, yN32 = 11.0, 32768, 512, 16384      # 32k[1]-n16k-512: m = 256, n1 = 64
#: 1.5 x the largest err_parent (finish_axis1_rows + prepare_facet_columns against the oracle) the cases below measure on an
#: MI355X: measured 2.038e-7 (the wrapping band and the full-size facets; the docstring of each case has its own figures).
#: err_new measured 2.13e-7 at most
ABS_CAP = 1.5 * 2.038e-7

_cores = {}


def cores(W, N, xM, yN):
    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    key = (W, N, xM, yN)
    if key not in _cores:
        _cores[key] = (SwiftlyCoreHip(W, N, xM, yN), orc.OracleCore(W, N, xM, yN))
    return _cores[key]


def relrms(a, b):
    return float(numpy.sqrt(numpy.mean(numpy.abs(a - b) ** 2) / numpy.mean(numpy.abs(b) ** 2)))


def window_of(core, off1):
    """(s, logical padded-facet column of every contribution element j) of wave ``off1`` (extract_from_facet, core.py:243-253)"""
    yN, m = core.yN_size, core.xM_yN_size
    s = off1 * yN // core.N
    j = numpy.arange(m)
    return s, (yN // 2 - m // 2 + s + ((j - s) % m)) % yN


def pack_band(core, data, band):
    """logical band elements ``data[F, rows, band_len]`` (element d = column band_start + d) as parity-split band buffers"""
    F, rows, length = data.shape
    half = core.band_columns(band) // 2
    d = numpy.arange(length)
    phys = numpy.zeros((F, rows, 2 * half), dtype=numpy.complex64)
    phys[:, :, (d & 1) * half + (d >> 1)] = data
    return phys


def oracle_columns(ref, contrib, off0, off1f):
    """(ii) for one facet: ``contrib[rows, m]`` = extract_from_facet(axis 1) of its band rows, in complex128"""
    m, xM = ref.xM_yN_size, ref.xM_size
    rows = contrib.shape[0]
    placed = ref.add_to_subgrid(contrib, off1f, 1)                       # [rows, xM]
    sp = off1f * xM // ref.N
    Z = placed[:, (numpy.arange(m) + xM // 2 - m // 2 + sp) % xM]        # Z[k], core.py:274-285
    return ref.prepare_facet(Z / ref.facet_window(rows)[:, None], off0, axis=0)   # [yN, m], window NOT applied


def run_case(sizes, rows, off0s, off1s, band, off1, sub_off0s, seed, check_gather=False):
    """both forms and the oracle for one call; returns [(err_new, err_parent)] per facet after the relative asserts"""
    import torch

    core, ref = cores(*sizes)
    yN, m = core.yN_size, core.xM_yN_size
    F = len(off0s)
    rng = numpy.random.default_rng(seed)
    data = (rng.standard_normal((F, rows, band[1])) + 1j * rng.standard_normal((F, rows, band[1]))).astype(numpy.complex64)
    bands = torch.from_numpy(pack_band(core, data, band)).cuda()
    s, cols = window_of(core, off1)
    d = (cols - band[0]) % yN
    assert (d < band[1]).all()
    if check_gather:  # the gather above is the oracle's extract_from_facet
        full = numpy.zeros((rows, yN), dtype=complex)
        full[:, (band[0] + numpy.arange(band[1])) % yN] = data[0]
        assert numpy.array_equal(ref.extract_from_facet(full, off1, 1), data[0][:, d].astype(complex))
    rowmap, n_rows = core.subgrid_column_rows(sub_off0s) if sub_off0s is not None else (None, yN)
    rm = rowmap.cpu().numpy() if rowmap is not None else numpy.arange(yN)
    keep = rm >= 0
    spare = 3  # rows of `out` no map entry points to: never written
    out = torch.full((F, n_rows + spare, m), float("nan"), dtype=torch.complex64, device="cuda")
    before = core.axis1_columns_issued
    res = core.prepare_facet_columns_axis1(bands, off0s, off1s, band, off1, rowmap, n_rows, out=out)
    assert res is out and core.axis1_columns_issued == before + 1
    got = out.cpu().numpy()
    rows_done, wband = core.finish_axis1_rows(bands, off1s, band, off1)
    parent = core.prepare_facet_columns(rows_done, off0s, wband, off1, rowmap, n_rows).cpu().numpy()
    written = numpy.zeros(n_rows + spare, dtype=bool)
    written[rm[keep]] = True
    errs = []
    for f in range(F):
        assert numpy.isfinite(got[f][written]).all()
        assert (~written).sum() >= spare and numpy.isnan(got[f][~written]).all()   # rows no kept row maps to are not written
        want = oracle_columns(ref, data[f][:, d].astype(complex), off0s[f], off1s[f])[keep]
        err_new, err_parent = relrms(got[f][rm[keep]], want), relrms(parent[f][rm[keep]], want)
        print(f"axis1 columns yN {yN} rows {rows} band {band} off1 {off1} facet {f} (off0 {off0s[f]}, off1 {off1s[f]}): "
              f"err_new {err_new:.3e} err_parent {err_parent:.3e} new-vs-parent {relrms(got[f][rm[keep]], parent[f][rm[keep]]):.3e}")
        errs.append((err_new, err_parent))
    for err_new, err_parent in errs:
        assert err_new <= 1.25 * err_parent + 1e-8, errs
        assert err_new <= ABS_CAP, (errs, ABS_CAP)
    return errs


S64 = (W64, N64, xM64, yN64)
FACETS64 = ([0, 22528, -64 * 352], [0, 64 * 352, -32 * 352])   # (off0s, off1s) of the three facets of one call
SUBS = [0, 3 * 928, -5 * 928]                                   # off0 of the subgrids whose rows a row map keeps


@pytest.mark.parametrize("off1,use_rowmap", [(0, False), (3 * 928, True), (-5 * 928, True), (3 * 928 + 2, True)])
def test_small_facets_partial_band(off1, use_rowmap):
    """rows 352: at most one row of a tile of n1 = 32 rows, n2 = 1024 apart, is present.  Band (10736, 11472); the last
    wave's window starts at an odd distance from the band start (the parity runs swap).  Measured on MI355X,
    err_new / err_parent at worst over the facets: 2.05e-7 / 1.98e-7, 2.06e-7 / 1.97e-7, 2.05e-7 / 1.96e-7, 2.05e-7 / 1.97e-7"""
    run_case(S64, 352, *FACETS64, (10736, 11472), off1, SUBS if use_rowmap else None, seed=100 + off1 % 97,
             check_gather=(off1 == 0))


def test_small_facets_wrapping_band():
    """the band (32001, 2049) wraps around the padded axis and so does the window of off1 = 33000 (s = 16500: columns
    32628 .. 32767, 0 .. 371), at an odd distance (627) from the band start.  Measured on MI355X: err_new 2.13e-7,
    err_parent 2.04e-7 at worst"""
    run_case(S64, 352, *FACETS64, (32001, 2049), 33000, SUBS, seed=7)


def test_rows_not_a_multiple_of_the_tile_and_a_band_that_is_the_window():
    """355 rows (no multiple of n1 = 32; odd), the band exactly the window of the wave.  Measured on MI355X: err_new 2.08e-7,
    err_parent 2.00e-7 at worst"""
    core, _ = cores(*S64)
    off1 = -5 * 928
    s, _ = window_of(core, off1)
    band = ((yN64 // 2 - 256 + s) % yN64, 512)
    run_case(S64, 355, *FACETS64, band, off1, SUBS, seed=8)


def test_full_size_facets_at_offsets_off_the_tile_grid():
    """rows 22528 (22 of the 32 rows of a tile present) at facet offsets that are no multiples of n2 = 1024, so that the
    present rows start inside a tile; a short band around the window at an odd distance.  Measured on MI355X: err_new
    2.13e-7, err_parent 2.04e-7 on all three facets"""
    core, _ = cores(*S64)
    off1 = 3 * 928
    s, _ = window_of(core, off1)
    band = ((yN64 // 2 - 256 + s - 37) % yN64, 600)
    run_case(S64, 22528, [1056, 22528 + 352, -22528 - 704], FACETS64[1], band, off1, SUBS, seed=9)


@pytest.mark.parametrize("off1", [0, -7 * 448 + 2])
def test_yN_16384_m_256(off1):
    """the second instance: n1 = 64 rows of 256 columns, pass B of 256 points; a facet pair, two waves, rows 700 (no multiple
    of 64) and a row map.  Measured on MI355X: err_new 1.84e-7, err_parent 1.82e-7 at worst"""
    core, _ = cores(W32, N32, xM32, yN32)
    assert core.supports_axis1_columns() and core.xM_yN_size == 256
    band = core.band_for_offsets([0, -7 * 448 + 2, 5 * 448])
    run_case((W32, N32, xM32, yN32), 700, [0, -11264 + 64 * 3], [64 * 5, -64 * 40], band, off1, [0, 448 * 3, -448 * 9], seed=11)


def test_refusals_write_nothing():
    import torch

    core, _ = cores(*S64)
    assert core.supports_axis1_columns(torch.complex64) and not core.supports_axis1_columns(torch.complex128)
    band = (10736, 11472)
    bands = torch.zeros((1, 64, core.band_columns(band)), dtype=torch.complex64, device="cuda")

    def untouched(out):
        return bool(torch.isnan(out).all())

    # a complex128 tensor
    out = torch.full((1, yN64, 512), float("nan"), dtype=torch.complex128, device="cuda")
    with pytest.raises(Exception, match="complex64"):
        core.prepare_facet_columns_axis1(bands.to(torch.complex128), [0], [0], band, 0, out=out)
    assert untouched(out)
    # a window outside the band
    out = torch.full((1, yN64, 512), float("nan"), dtype=torch.complex64, device="cuda")
    with pytest.raises(Exception, match="not inside the band"):
        core.prepare_facet_columns_axis1(bands, [0], [0], band, 30 * 928, out=out)
    assert untouched(out)
    del out
    # a core of yN 65536 / m 512: pass B would be 2048 points
    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    big = SwiftlyCoreHip(W64, 131072, 1024, 65536)
    assert big.xM_yN_size == 512 and not big.supports_axis1_columns()
    b2 = torch.zeros((1, 64, big.band_columns(band)), dtype=torch.complex64, device="cuda")
    out = torch.full((1, 65536, 512), float("nan"), dtype=torch.complex64, device="cuda")
    with pytest.raises(Exception, match="yN 65536"):
        big.prepare_facet_columns_axis1(b2, [0], [0], band, 0, out=out)
    assert untouched(out)


# ------------------------------------------------------------------------------------------------ whole pass
def _small_rows_problem(seed):
    """_small_rows_problem of tests/test_hip_band_pipeline_gpu.py, restated: three facets of 352 x 352 of the 64k
    configuration, a 3 x 4 block of subgrids"""
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    yB, xA = 352, 928
    P = dict(W=W64, fov=1.0, N=N64, yB_size=yB, yN_size=yN64, xA_size=xA, xM_size=xM64)
    fstep = N64 // xM64
    facet_cfgs = [sw.FacetConfig(o0, o1, yB) for o0, o1 in ((0, 0), (0, 50 * fstep), (-70 * fstep, 0))]
    vectors = [sep.facet_vectors(seed + j, yB, rank=2) for j in range(len(facet_cfgs))]
    facets = [bench.separable_facet(torch, vectors[j], c) for j, c in enumerate(facet_cfgs)]
    sg_cfgs = [sw.SubgridConfig(i0 * xA, i1 * xA, xA) for i0 in (0, 2, 69) for i1 in (0, 3, 4, 70)]
    so = sep.SeparableOracle(cores(*S64)[1], [orc.CoverItem(c.off0, c.off1, c.size) for c in facet_cfgs], vectors)
    waves = {}
    for c in sg_cfgs:
        waves.setdefault(c.off1, []).append(c)
    return torch, sw, P, facet_cfgs, facets, sg_cfgs, so, waves


def _counting(core):
    """``core.finish_axis1_rows`` replaced by a counting wrapper; returns the list the calls are appended to"""
    calls, inner = [], core.finish_axis1_rows
    core.finish_axis1_rows = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    return calls


def test_whole_pass_matches_the_oracle_and_the_row_pass_form():
    torch, sw, P, facet_cfgs, facets, sg_cfgs, so, waves = _small_rows_problem(seed=191)
    cfg_rows = sw.SwiftlyConfig(backend="hip", axis1_first="rows", **P)
    cfg = sw.SwiftlyConfig(backend="hip", axis1_first="k2", **P)
    assert cfg.core.axis1_first == "k2" and cfg.core.supports_axis1_columns(torch.complex64)
    assert pickle.loads(pickle.dumps(cfg.core)).axis1_first == "k2"
    pairs = list(zip(facet_cfgs, facets))
    ref = sw.SwiftlyForward(cfg_rows, pairs, subgrid_configs=sg_cfgs, wave_axis=1)
    want, err_rows = {}, {}
    for key, wave in waves.items():
        base = ref.get_wave(wave).cpu().numpy()
        for k, c in enumerate(wave):
            want[key, k] = so.subgrid(orc.CoverItem(c.off0, c.off1, c.size))
            err_rows[key, k] = relrms(base[k], want[key, k])
    for prefetch, planned in ((True, True), (False, True), (False, False)):
        old = sw.api._PREFETCH
        sw.api._PREFETCH = prefetch
        calls = None
        try:
            calls, before = _counting(cfg.core), cfg.core.axis1_columns_issued
            fwd = sw.SwiftlyForward(cfg, pairs, subgrid_configs=sg_cfgs if planned else None, wave_axis=1)
            order = sorted(waves) if prefetch else sorted(waves)[::-1]
            for key in (order if planned else order[:2]):
                got = fwd.get_wave(waves[key]).cpu().numpy()
                for k in range(len(waves[key])):
                    err = relrms(got[k], want[key, k])
                    print(f"whole pass prefetch {prefetch} planned {planned} wave {key} subgrid {k}: k2 {err:.3e} rows {err_rows[key, k]:.3e}")
                    assert err < 4e-6, (prefetch, planned, key, k, err)
                    assert err <= 1.25 * err_rows[key, k] + 1e-8, (prefetch, planned, key, k, err, err_rows[key, k])
            torch.cuda.synchronize()
            assert fwd._axis1() == 1 and fwd._placed()  # pylint: disable=protected-access
            assert not calls and cfg.core.axis1_columns_issued >= before + (len(waves) if planned else 2)
            assert (fwd.prefetch_issued > 0) == prefetch
        finally:
            sw.api._PREFETCH = old
            if calls is not None:
                del cfg.core.finish_axis1_rows


def _both_forms(P, facet_cfgs, facets, sg_cfgs, wave_axis):
    """the planned subgrids with axis1_first = "rows" and "k2" on a core without an instance of the new entry"""
    import ska_sdp_exec_swiftly_amd as sw

    res = {}
    for form in ("rows", "k2"):
        cfg = sw.SwiftlyConfig(backend="hip", axis1_first=form, **P)
        assert cfg.core.axis1_first == form and not cfg.core.supports_axis1_columns()
        fwd = sw.SwiftlyForward(cfg, list(zip(facet_cfgs, facets)), subgrid_configs=sg_cfgs, wave_axis=wave_axis)
        order = sorted(sg_cfgs, key=(lambda c: (c.off1, c.off0)) if wave_axis == 1 else (lambda c: (c.off0, c.off1)))
        try:
            res[form] = [t.cpu().numpy() for t in fwd.get_subgrid_tasks(order)]
        except NotImplementedError as exc:
            res[form] = str(exc)
        assert cfg.core.axis1_columns_issued == 0
    return res


def _random_facets(sw, torch, yB, offs, seed):
    rng = numpy.random.default_rng(seed)
    facet_cfgs = [sw.FacetConfig(o0, o1, yB) for o0, o1 in offs]
    facets = [torch.from_numpy((rng.standard_normal((yB, yB)) + 1j * rng.standard_normal((yB, yB))).astype(numpy.complex64)).cuda()
              for _ in facet_cfgs]
    return facet_cfgs, facets


def test_a_core_without_the_instance_runs_the_row_pass_form():
    """"k2" on a core without the instance does what "rows" does there.  yN 512 (the P11 sizes of
    tests/test_hip_band_pipeline_gpu.py) keeps the plain band layout, for which finish_axis1_rows does not exist either: in
    the reference schedule (wave_axis = 0) both values give the same bits, in the band pipeline both meet the refusal of
    finish_axis1_rows.  yN 16384 with m = 128 has the row pass and no instance of the new entry: the same bits."""
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    P = dict(W=11.0, fov=1.0, N=1024, yB_size=352, yN_size=512, xA_size=192, xM_size=256)
    facet_cfgs, facets = _random_facets(sw, torch, 352, [(0, 0), (352, -352)], seed=5)
    sg_cfgs = [sw.SubgridConfig(i0 * 192, i1 * 192, 192) for i0 in (0, 2) for i1 in (0, 1, 4)]
    res = _both_forms(P, facet_cfgs, facets, sg_cfgs, wave_axis=0)
    assert all(numpy.array_equal(a, b) for a, b in zip(res["rows"], res["k2"])) and len(res["k2"]) == len(sg_cfgs)
    res = _both_forms(P, facet_cfgs, facets, sg_cfgs, wave_axis=1)
    assert isinstance(res["rows"], str) and "finish_axis1_rows" in res["rows"] and res["k2"] == res["rows"]
    # (N, yN, xM) = (32768, 16384, 256): m = 128
    P = dict(W=11.0, fov=1.0, N=32768, yB_size=256, yN_size=16384, xA_size=192, xM_size=256)
    facet_cfgs, facets = _random_facets(sw, torch, 256, [(0, 0), (128 * 3, -128 * 40)], seed=6)
    sg_cfgs = [sw.SubgridConfig(i0 * 192, i1 * 192, 192) for i0 in (0, 2) for i1 in (0, 1, 100)]
    res = _both_forms(P, facet_cfgs, facets, sg_cfgs, wave_axis=1)
    assert len(res["k2"]) == len(sg_cfgs) and all(numpy.array_equal(a, b) for a, b in zip(res["rows"], res["k2"]))


def test_two_virtual_ranks_of_the_multi_gpu_class():
    """as test_axis1_first_through_the_multi_gpu_classes: two in-process ranks with whole facets and "k2" give the subgrids
    of the single-process "rows" object within that test's bound"""
    torch, sw, P, facet_cfgs, facets, sg_cfgs, _, waves = _small_rows_problem(seed=193)
    from ska_sdp_exec_swiftly_amd.distributed import DistributedForward

    cfg_rows = sw.SwiftlyConfig(backend="hip", axis1_first="rows", **P)
    cfg = sw.SwiftlyConfig(backend="hip", axis1_first="k2", **P)
    world = 2
    ref = sw.SwiftlyForward(cfg_rows, list(zip(facet_cfgs, facets)), subgrid_configs=sg_cfgs, wave_axis=1)
    fwds = [DistributedForward(cfg, facet_cfgs, facets, dtype=torch.complex64, wave_axis=1, subgrid_configs=sg_cfgs,
                               rank_world=(r, world), cooperative=False) for r in range(world)]
    for wave in waves.values():
        want = ref.get_wave(wave)
        packed = [f.pack_wave(wave) for f in fwds]
        recvs = []  # in-process all-to-all: rank r receives chunk r of every sender, in sender order
        for r in range(world):
            parts = []
            for send, in_counts, _ in packed:
                pos = sum(in_counts[:r])
                parts.append(send[pos : pos + in_counts[r]])
            recvs.append(torch.cat(parts))
        got = {}
        for r, f in enumerate(fwds):
            mine, res = f.unpack_wave(wave, recvs[r])
            for k, i in enumerate(mine):
                got[i] = res[k]
        assert sorted(got) == list(range(len(wave)))
        scale = float(want.abs().max())
        for i in range(len(wave)):
            assert float((got[i] - want[i]).abs().max()) <= 5e-6 * scale
