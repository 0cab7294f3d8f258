"""
The backward band schedule (``SwiftlyBackward(..., wave_axis=1, dtype=torch.complex128)``) on
complex128 subgrids.

Every expected value is a composition of the 1-D oracle primitives (oracle/swiftly_oracle.py) in complex128, or comes from
oracle/separable.py; none comes from another HIP path.

(a) ``accumulate_facet_columns`` + ``band_zero_untouched`` at every length class, ``yN = 2^L``, L = 6 .. 15, on the cases of
    the complex64 facet sweep (tests/test_hip_facet_sweep_gpu.py: ``acc_problem``) with parts drawn in double and double masks
(b) ``finish_facet_band`` at L = 9, 13, 14, 15; refusals at L = 16 and ``yN = 3 * 2^10``
(c) ``split_prepare_facets`` and ``wave_split_subgrids`` for every pair of ``SPLIT_PAIRS_C128``
(d) whole passes against ``SeparableBackwardOracle``
(e) defaults and refusals

Single entry points: ``max|err| <= 5e-12 * max|want|`` (``C128_TOL``).  Whole passes, with ``e(x)`` the relative RMSE against
the separable oracle: ``e(band) <= 1e-10`` and ``e(band) <= 3 * e(wave_axis=0 complex128) + 1e-15``.

Every case prints its figure (``C128BWD ...`` lines, ``pytest -s``).  Measured on an MI355X, worst ``max|err| / max|want|``
per length (bound 5e-12):

   L   accumulate  finish_band
   6    2.8e-16        -
   7    2.5e-16        -
   8    3.0e-16        -       (33 facets 3.4e-16, one-facet workspace 2.2e-16, two chunks 3.0e-16)
   9    3.3e-16     3.5e-16
  10    2.9e-16        -
  11    3.8e-16        -
  12    4.0e-16        -
  13    4.9e-16     4.6e-16
  14    4.2e-16     4.1e-16
  15    5.6e-16     4.2e-16

split_prepare_facets / wave_split_subgrids: (7, 8) 4.6e-16 / 4.8e-16, (7, 10) 4.8e-16 / 5.3e-16, (8, 9) 5.3e-16 / 6.0e-16,
(8, 10) 5.4e-16 / 5.3e-16, (9, 10) 5.6e-16 / 5.8e-16; xA = xM 4.6e-16 / 5.6e-16; 64 facets x 65 subgrids 3.7e-16 / 3.7e-16.

Whole passes, relative RMSE against the separable oracle, band schedule / complex128 wave_axis=0: SMALL off1-major waves
1.57e-14 / 1.56e-14, single adds (lru_backward 1 and 4) 1.48e-14 (1.5e-14 from the whole-wave run), no plan, delayed and
two chunks 1.57e-14, sparse plan with duplicates 1.51e-14 / 1.52e-14, (64, 256) without a split instance 1.71e-14 /
1.70e-14, 64k[1]-n16k-1k 3.06e-11 / 3.04e-11 on 64 rows per facet, 3.8e-11 between the two schedules on whole facets.

Module wall time: 17 s for the 30 cases (pytest's own figure); the slowest case takes 2.2 s.
"""
import gc

import numpy
import pytest

import test_hip_c128_band_pipeline_gpu as fwd128
import test_hip_facet_sweep_gpu as fs
import test_hip_instance_sweep_gpu as sweep
from oracle import separable as sep
from oracle import swiftly_oracle as orc

pytestmark = pytest.mark.gpu

C128_TOL = 5e-12  # max|err| / max|expected|, single entry points
PASS_TOL = 1e-10  # relative RMSE against the separable oracle
SMALL = dict(W=11.0, fov=1.0, N=1024, yB_size=352, yN_size=512, xA_size=192, xM_size=256)
ACC_LENGTHS = list(range(6, 16))
SPLIT_PAIRS_C128 = [(7, 8), (7, 10), (8, 9), (8, 10), (9, 10)]  # csrc/swiftly_caps.h
SENTINEL = fs.SENTINEL


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    import torch

    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def relrms(got, want):
    return float(numpy.sqrt(numpy.mean(numpy.abs(got - want) ** 2) / numpy.mean(numpy.abs(want) ** 2)))


def check128(what, got, want, note=""):
    """all elements of ``got`` against ``want``: ``max|err| <= C128_TOL * max|want|``; returns the figure"""
    got = numpy.asarray(got)
    assert got.shape == want.shape and got.dtype == numpy.complex128, (what, got.shape, want.shape, got.dtype)
    assert numpy.isfinite(got).all(), what
    err = float(numpy.max(numpy.abs(got - want)) / numpy.max(numpy.abs(want)))
    print(f"C128BWD {what:<28s} {err:.3e} (bound {C128_TOL:.1e}) {note}")
    assert err <= C128_TOL, (what, note, err)
    return err


# ------------------------------------------------------------------------------------ (a) accumulate_facet_columns
_ACC128 = {}


def acc_problem128(L, F=2, n_waves=2, seed=0):
    """the case of ``acc_problem`` of the complex64 facet sweep (same cores, offsets, waves, band and masks) with parts drawn
    in DOUBLE -- values that float32 cannot hold, so a load that dropped low mantissa bits of the 16-byte points would
    show -- and ``want`` composed from those values by the oracle; cached per case"""
    key = (L, F, n_waves, seed)
    if key in _ACC128:
        return _ACC128[key]
    from ska_sdp_exec_swiftly_amd.core_hip import band_range

    core, ref = fs.cores(fs.params(L))
    N, yN, m = core.N, core.yN_size, core.xM_yN_size
    fstep, sstep = core.facet_off_step, core.subgrid_off_step
    yB = fs.facet_size(L, odd=(L == 9))
    rng = numpy.random.default_rng(5200 + 16 * L + seed)
    facet_off0s = [5 * fstep, -24 * fstep] if F == 2 else [((7 * f) % 61 - 30) * fstep for f in range(F)]
    assert len(set(facet_off0s)) == F
    masks = (rng.random((F, yB)) > 0.1).astype(numpy.float64)
    # adjacent windows share m / 4 band columns; a third offset widens the band so that untouched columns exist
    s1 = [yN // 8, yN // 8 + m - m // 4][:n_waves]
    s0 = [[-m, -(m // 4), m // 2], [m // 8, m // 8 + m // 2]][:n_waves]
    waves = [(a * sstep, [b * sstep for b in bs]) for a, bs in zip(s1, s0)]
    band = band_range(N, yN, m, [w[0] for w in waves] + [(s1[-1] + m + m // 2) * sstep]) if L >= 10 else (0, yN)
    cols = sorted({int(c) for a in s1 for c in (yN // 2 - m // 2 + numpy.arange(m) + a) % yN})
    pos = numpy.full(yN, -1)
    pos[cols] = numpy.arange(len(cols))
    want = numpy.zeros((F, yB, len(cols)), dtype=complex)
    parts = []
    i = numpy.arange(m)
    for (_off1, off0s), a in zip(waves, s1):
        shape = (F, len(off0s), m, m)
        pw = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
        assert (pw.real.astype(numpy.float32) != pw.real).any()
        parts.append(pw)
        big = (yN // 2 - m // 2 + i + a) % yN  # add_to_facet along axis 1: window index i holds contribution column (i + s1) mod m
        for f in range(F):
            acc = numpy.zeros((yN, m), dtype=complex)
            for b, o0 in enumerate(off0s):
                acc = ref.add_to_facet(pw[f, b], o0, axis=0, out=acc)
            fin = ref.finish_facet(acc, facet_off0s[f], yB, axis=0) * masks[f][:, None]
            want[f][:, pos[big]] += fin[:, (i + a) % m]
    prob = dict(yB=yB, facet_off0s=facet_off0s, masks=masks, waves=waves, band=band, cols=numpy.array(cols), want=want,
                parts=parts)
    _ACC128[key] = prob
    return prob


def acc_run128(L, prob, workspace_facets=None, two_chunks=False):
    """the waves of ``prob`` through accumulate_facet_columns + band_zero_untouched in complex128, from NaN-filled
    accumulators"""
    import torch

    core, _ = fs.cores(fs.params(L))
    yN, m = core.yN_size, core.xM_yN_size
    yB, band, cols = prob["yB"], prob["band"], prob["cols"]
    F = len(prob["facet_off0s"])
    start, length = band
    bands = torch.full((F, yB, length), float("nan"), dtype=torch.complex128, device="cuda")  # uninitialised on purpose
    touched = torch.zeros((length,), dtype=torch.uint8, device="cuda")
    work = torch.empty((F if workspace_facets is None else workspace_facets, yN, m), dtype=torch.complex128, device="cuda")
    masks = prob["masks"]
    mask_t = torch.from_numpy(masks).cuda()
    assert mask_t.dtype == torch.float64
    two_sources = False
    for (off1, off0s), pw in zip(prob["waves"], prob["parts"]):
        S = len(off0s)
        assert pw.dtype == numpy.complex128
        if two_chunks:
            # the last subgrid in a chunk of its own that lies BELOW the first chunk in memory: offsets are relative to
            # the lowest address, a negative one would read as "no source row"
            buf = torch.empty((F * S * m * m + 64,), dtype=torch.complex128, device="cuda")
            low = buf[: F * m * m].view(F, 1, m, m)
            high = buf[F * m * m + 64:].view(F, S - 1, m, m)
            high.copy_(torch.from_numpy(pw[:, : S - 1]).cuda())
            low.copy_(torch.from_numpy(pw[:, S - 1:]).cuda())
            assert high.data_ptr() > low.data_ptr()
            base, offs, fstr = buf, [F * m * m + 64, 0], [(S - 1) * m * m, m * m]
            locs = [(0, b) for b in range(S - 1)] + [(1, 0)]
        else:
            base = torch.from_numpy(pw).cuda()
            offs, fstr, locs = [0], [base.stride(0)], None
        groups = core.column_row_sources(off0s, locs)
        assert len(groups) == 1 or yN < 4 * m  # (short rings: three windows overlap in some rows, two tables)
        for _, table in groups:
            two_sources |= bool((table[1] >= 0).any())
            core.accumulate_facet_columns(base, m, offs, fstr, table, prob["facet_off0s"], yB, mask_t, off1, bands, band,
                                          workspace=work, touched=touched)
    core.band_zero_untouched(bands, touched)
    assert two_sources  # a row with two sources occurs
    tch = touched.cpu().numpy()
    d = (cols - start) % yN
    assert (d < length).all() and (tch[d] == 1).all() and int(tch.sum()) == len(cols)
    if m < yN:  # (m = yN at L = 6, 7: every column is in every window)
        assert (tch == 0).any()
    assert not bool((bands[:, :, torch.from_numpy(tch == 0).cuda()] != 0).any()), "an untouched band column is not zero"
    got = bands[:, :, torch.from_numpy(d).cuda()].cpu().numpy()
    assert (masks == 0).any()
    for f in range(F):
        assert not got[f][masks[f] == 0].any(), "a masked row is not exactly zero"
    return check128("accumulate_facet_columns", got, prob["want"], note=f"L {L} F {F}")


@pytest.mark.parametrize("L", ACC_LENGTHS)
def test_accumulate_facet_columns_c128_lengths(L):
    """the gather-sum column pass with 16-byte points at every length class: single passes of 64 and 128 points, of 256 and
    512 points on 32-column tiles (source rows per half-wave), the four-steps 5+5 .. 7+8; two waves whose band columns
    overlap (first-write flags + read-modify-write), three / two subgrids per wave with overlapping row windows, two facets
    with double masks and distinct offsets, an odd facet size at L = 9, a pruned band from L = 10 on"""
    prob = acc_problem128(L)
    assert (prob["yB"] % 2 == 1) == (L == 9)
    assert (prob["band"][1] < (1 << L)) == (L >= 10)
    assert len(set(prob["facet_off0s"])) == 2
    acc_run128(L, prob)


def test_accumulate_facet_columns_c128_launch_groups():
    """L = 8: 33 facets (second launch group: chunk offsets, masks and bands from facet 32 on), a workspace sized for one
    facet (one launch per facet), and the contributions in two chunks allocated in descending address order"""
    acc_run128(8, acc_problem128(8, F=33, n_waves=1, seed=33))
    acc_run128(8, acc_problem128(8, F=3, n_waves=2, seed=3), workspace_facets=1)
    acc_run128(8, acc_problem128(8), two_chunks=True)


# ------------------------------------------------------------------------------------ (b) finish_facet_band
def finish_band_run128(core, ref, rng, band, off, yB, mask, rows=24, note=""):
    import torch

    yN = core.yN_size
    start, length = band
    data = rng.standard_normal((rows, length)) + 1j * rng.standard_normal((rows, length))
    full = numpy.zeros((rows, yN), dtype=complex)
    full[:, (start + numpy.arange(length)) % yN] = data
    want = ref.finish_facet(full, off, yB, axis=1) * mask[None, :]
    obuf = torch.full((rows + 1, yB + 5), SENTINEL, dtype=torch.complex128, device="cuda")
    out = obuf[:rows, :yB]
    res = core.finish_facet_band(torch.from_numpy(data).cuda(), band, off, yB, mask=mask, out=out)
    assert res is out and res.dtype == torch.complex128
    assert bool((obuf[rows] == SENTINEL).all()) and bool((obuf[:, yB:] == SENTINEL).all()), "finish_facet_band wrote outside its rows"
    got = out.cpu().numpy()
    assert not got[:, mask == 0].any()  # masked pixels are exactly zero
    return check128("finish_facet_band", got, want, note=note)


@pytest.mark.parametrize("L", [9, 13, 14, 15])
def test_finish_facet_band_c128_lengths(L):
    """finish_facet along the contiguous axis of a complex128 band accumulator: one workgroup per row up to 8192 points, the
    two-kernel long rows at 16384 and 32768 with the band load map; interior, wrapping and full bands, a partial mask"""
    core, ref = fs.cores(fs.params(L))
    yN = core.yN_size
    yB = fs.facet_size(L)
    rng = numpy.random.default_rng(4100 + L)
    mask = (rng.random(yB) > 0.15).astype(float)
    assert 0 < mask.sum() < yB
    cases = [((yN // 2 - 5 * yN // 32, 11 * yN // 32 + 8), 0), ((yN - 3 * yN // 32, 7 * yN // 32 + 1), yB), ((0, yN), -yB)]
    if L == 15:
        cases.append(((yN // 4 + 1, 15000), 3 * 352))
    assert cases[1][0][0] + cases[1][0][1] > yN
    for k, (band, off) in enumerate(cases):
        finish_band_run128(core, ref, rng, band, off, yB, mask, note=f"L {L} band {k}")


def _accumulate_dummy(core, dtype):
    """a well-formed one-facet accumulate_facet_columns call on zeros (for the refusals: the gate comes first)"""
    import torch

    yN, m = core.yN_size, core.xM_yN_size
    parts = torch.zeros((1, 1, m, m), dtype=dtype, device="cuda")
    table = torch.full((2, yN), -1, dtype=torch.int32, device="cuda")
    bands = torch.full((1, 8, yN), SENTINEL, dtype=dtype, device="cuda")
    core.accumulate_facet_columns(parts, m, [0], [0], table, [0], 8, None, 0, bands, (0, yN))
    return bands


def test_backward_band_c128_entry_points_refuse_other_lengths():
    import torch

    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip, _lib

    core, _ = fs.cores(fs.params(16))
    yN = core.yN_size
    assert not core.supports_backward_band(torch.complex128, explicit=True) and core.supports_backward_band(torch.complex64)
    out = torch.full((4, 1024), SENTINEL, dtype=torch.complex128, device="cuda")
    with pytest.raises(NotImplementedError, match="complex128"):
        core.finish_facet_band(torch.zeros((4, yN), dtype=torch.complex128, device="cuda"), (0, yN), 0, 1024, out=out)
    assert bool((out == SENTINEL).all())
    with pytest.raises(NotImplementedError, match="complex128"):
        _accumulate_dummy(core, torch.complex128)
    core3 = SwiftlyCoreHip(fs.W, 6144, 256, 3 << 10)  # yN = 3 * 2^10, m = 128
    assert core3.supports_backward_band(torch.complex64) and not core3.supports_backward_band(torch.complex128, explicit=True)
    assert "Q * 2^k" in _lib.last_error()
    with pytest.raises(NotImplementedError, match="complex128"):
        _accumulate_dummy(core3, torch.complex128)
    bands = _accumulate_dummy(core3, torch.complex64)  # (complex64 runs there: the radix-3 pass)
    assert bool(torch.isfinite(bands.abs()).all())


# --------------------------------------------------------------- (c) split_prepare_facets + wave_split_subgrids
def split_case(pair, f_offs, s_offs, xA, seed):
    """complex128 subgrids ``[S, xA, xA]`` and the oracle's ``want[S, F, m, m]`` (prepare_and_split_subgrid) and
    ``tmp_want[S, xM, xA]`` (prepare_subgrid along axis 0 only)"""
    _, ref = sweep.cores(pair)
    xM = ref.xM_size
    rng = numpy.random.default_rng(seed)
    S = len(s_offs)
    sub = rng.standard_normal((S, xA, xA)) + 1j * rng.standard_normal((S, xA, xA))
    items = [orc.CoverItem(o0, o1, 0) for o0, o1 in f_offs]
    want = numpy.array([orc.prepare_and_split_subgrid(ref, sub[b], s_offs[b], items) for b in range(S)])
    tmp_want = numpy.empty((S, xM, xA), dtype=complex)
    for b, (s0, _s1) in enumerate(s_offs):
        tmp_want[b] = numpy.array([ref.prepare_subgrid(sub[b][:, c], s0) for c in range(xA)]).T
    return sub, want, tmp_want


def split_run(pair, f_offs, s_offs, xA, seed, note):
    import torch

    core, ref = sweep.cores(pair)
    m, xM = ref.xM_yN_size, ref.xM_size
    F, S = len(f_offs), len(s_offs)
    sub, want, tmp_want = split_case(pair, f_offs, s_offs, xA, seed)
    f0, f1 = [o[0] for o in f_offs], [o[1] for o in f_offs]
    assert core.supports_split_prepare(torch.complex128, F)
    # split_prepare_facets alone, from the oracle's axis-0 prepared subgrids (padded input strides)
    tbuf = torch.full((S, xM + 1, xA + 3), SENTINEL, dtype=torch.complex128, device="cuda")
    tview = tbuf[:, :xM, :xA]
    tview.copy_(torch.from_numpy(tmp_want).cuda())
    out, obuf = sweep.padded_blocks(F, S, m, torch.complex128)
    res = core.split_prepare_facets(tview, [s[1] for s in s_offs], f0, f1, out)
    assert res is out and res.dtype == torch.complex128 and tuple(res.shape) == (F, S, m, m)
    assert sweep.blocks_padding_intact(obuf, S, m * m)
    check128("split_prepare_facets", out.cpu().numpy().transpose(1, 0, 2, 3), want, note=note)
    # the whole wave natively
    work = torch.empty(2 * S * xM * xA, dtype=torch.complex128, device="cuda")
    out2, obuf2 = sweep.padded_blocks(F, S, m, torch.complex128)
    res = core.wave_split_subgrids(torch.from_numpy(sub).cuda(), [s[0] for s in s_offs], [s[1] for s in s_offs], f0, f1, work,
                                   out2)
    assert res is out2 and res.dtype == torch.complex128
    assert sweep.blocks_padding_intact(obuf2, S, m * m)
    check128("wave_split_subgrids", out2.cpu().numpy().transpose(1, 0, 2, 3), want, note=note)


@pytest.mark.parametrize("pair", SPLIT_PAIRS_C128, ids=[f"m{1 << a}-xM{1 << b}" for a, b in SPLIT_PAIRS_C128])
def test_split_prepare_facets_and_wave_split_subgrids_c128(pair):
    """every complex128 instance on the offsets of the instance sweep: five facets (two share off1, negative off0 / off1,
    placement windows and row bands that wrap), three subgrids with wrapping offsets, an odd subgrid size below xM"""
    f_offs, s_offs = sweep.offsets(pair)
    assert len(f_offs) == 5 and len(s_offs) == 3
    assert min(o[0] for o in f_offs) < 0 and min(o[1] for o in f_offs) < 0 and len({o[1] for o in f_offs}) < 5
    xM = 1 << pair[1]
    split_run(pair, f_offs, s_offs, xM - 2 * (xM // 8) - 1, 77 + 100 * pair[0] + pair[1], f"m {1 << pair[0]} xM {xM}")


def test_split_prepare_c128_limits_at_128_256():
    """(7, 8): an uncropped subgrid (xA = xM); 64 facets as an 8 x 8 grid of offsets with 65 subgrids (second launch from
    subgrid 64 on); 65 facets and a pair outside the table raise"""
    import torch

    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    pair = (7, 8)
    core, _ = sweep.cores(pair)
    fstep, sstep, xM, m, yN = core.facet_off_step, core.subgrid_off_step, core.xM_size, core.xM_yN_size, core.yN_size
    f_offs, s_offs = sweep.offsets(pair)
    split_run(pair, f_offs, s_offs, xM, 78, "xA = xM")
    grid = [-(xM // 5), -(xM // 11), 0, xM // 9, xM // 4 + 1, xM // 2 - 2, 5 * (xM // 8), xM - 3]
    f64 = [(a * fstep, b * fstep) for a in grid for b in grid]
    s65 = [(((7 * b) % yN - yN // 2) * sstep, ((11 * b + 3) % yN - yN // 3) * sstep) for b in range(65)]
    split_run(pair, f64, s65, 33, 79, "64 facets, 65 subgrids")
    G = torch.zeros((65, 1, m, m), dtype=torch.complex128, device="cuda")
    tmp = torch.zeros((1, xM, 33), dtype=torch.complex128, device="cuda")
    with pytest.raises(NotImplementedError):
        core.split_prepare_facets(tmp, [0], [0] * 65, [0] * 65, G)
    # (512, 2048): a complex64 instance without a complex128 one
    other = SwiftlyCoreHip(fs.W, 8192, 2048, 2048)
    assert other.xM_yN_size == 512 and other.supports_split_prepare(torch.complex64)
    assert not other.supports_split_prepare(torch.complex128)
    sub = torch.zeros((1, 33, 33), dtype=torch.complex128, device="cuda")
    out = torch.full((1, 1, 512, 512), SENTINEL, dtype=torch.complex128, device="cuda")
    work = torch.empty(2 * 2048 * 33, dtype=torch.complex128, device="cuda")
    with pytest.raises(NotImplementedError, match="complex128"):
        other.wave_split_subgrids(sub, [0], [0], [0], [0], work, out)
    with pytest.raises(NotImplementedError, match="complex128"):
        other.split_prepare_facets(torch.zeros((1, 2048, 33), dtype=torch.complex128, device="cuda"), [0], [0], [0], out)
    assert bool((out == SENTINEL).all())


# ----------------------------------------------------------------------------------------------------- (d) whole passes
def subgrid128(vec, cfg):
    """complex128 device subgrid ``sum_r u_r (x) v_r`` times the cover masks"""
    return fwd128._facet128(vec, cfg)


_SMALL = {}


def small_problem():
    """full facet and subgrid covers (masks on both sides) of SMALL, separable rank-2 subgrids, the oracle's facets and
    the complex128 reference schedule's error; computed once"""
    if _SMALL:
        return _SMALL
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    p = SMALL
    cfg = sw.SwiftlyConfig(backend="hip", **p)
    facet_cfgs = sw.api.make_full_cover_config(p["N"], p["yB_size"], sw.FacetConfig)
    sg_cfgs = sw.api.make_full_cover_config(p["N"], p["xA_size"], sw.SubgridConfig)
    assert any(c.mask0 is not None for c in facet_cfgs) and any(c.mask1 is not None for c in sg_cfgs)
    vectors = [sep.subgrid_vectors(1100 + i, p["xA_size"], rank=2) for i in range(len(sg_cfgs))]
    data = [subgrid128(v, c) for v, c in zip(vectors, sg_cfgs)]
    ref = orc.OracleCore(p["W"], p["N"], p["xM_size"], p["yN_size"])
    oracle = sep.SeparableBackwardOracle(ref, facet_cfgs, sg_cfgs, vectors)
    want = numpy.array([oracle.facet(j) for j in range(len(facet_cfgs))])
    assert cfg.core.supports_backward_band(torch.complex128, explicit=True)
    b0 = sw.SwiftlyBackward(cfg, facet_cfgs, wave_axis=0)
    b0.add_new_subgrid_tasks(sg_cfgs, data)
    got0 = numpy.array([t.cpu().numpy() for t in b0.finish()])
    assert got0.dtype == numpy.complex128
    _SMALL.update(sw=sw, cfg=cfg, facet_cfgs=facet_cfgs, sg_cfgs=sg_cfgs, vectors=vectors, data=data, ref=ref, want=want,
                  e_ref=relrms(got0, want), by1=sorted(range(len(sg_cfgs)), key=lambda i: (sg_cfgs[i].off1, sg_cfgs[i].off0)))
    return _SMALL


def pass_rule(what, got, want, e_ref):
    """``e(band) <= 1e-10`` and ``e(band) <= 3 e(wave_axis=0 complex128) + 1e-15``"""
    got = numpy.asarray(got)
    assert got.dtype == numpy.complex128 and got.shape == want.shape, (what, got.dtype, got.shape)
    e = relrms(got, want)
    print(f"C128BWD pass {what:<34s} band {e:.3e}  wave_axis=0 {e_ref:.3e}")
    assert e <= PASS_TOL and e <= 3 * e_ref + 1e-15, (what, e, e_ref)
    return e


def band_backward(P, **kw):
    import torch

    bwd = P["sw"].SwiftlyBackward(P["cfg"], P["facet_cfgs"], wave_axis=1, dtype=torch.complex128, **kw)
    assert bwd.wave_axis == 1
    return bwd


def finished(bwd):
    return numpy.array([t.cpu().numpy() for t in bwd.finish()])


def whole_waves_result(P):
    """the planned pass in off1-major whole waves (computed once: the staged runs are compared with it)"""
    import torch

    if "got_plan" in P:
        return P["got_plan"]
    sg, data, by1 = P["sg_cfgs"], P["data"], P["by1"]
    bwd = band_backward(P, subgrid_configs=sg)
    folds = []
    inner = bwd._add_wave
    bwd._add_wave = lambda sgs, subs: (folds.append(len(sgs)), inner(sgs, subs))[1]
    bwd.add_new_subgrid_tasks([sg[i] for i in by1], [data[i] for i in by1])
    assert bwd.bands.bands.dtype == torch.complex128 and bwd.bands.work.dtype == torch.complex128
    assert bwd.bands.masks0 is not None and bwd.bands.masks0.dtype == torch.float64
    n1 = len({c.off1 for c in sg})
    assert folds == [len(sg) // n1] * n1  # whole waves: no staging copy
    P["got_plan"] = finished(bwd)
    return P["got_plan"]


def test_backward_small_whole_waves_with_a_plan():
    P = small_problem()
    pass_rule("off1-major waves, plan", whole_waves_result(P), P["want"], P["e_ref"])


@pytest.mark.parametrize("lru_backward", [1, 4])
def test_backward_small_single_adds_are_staged(lru_backward):
    """the same subgrids one by one in off0-major order: complex128 staging buffers per off1, eviction from
    LRUCache(lru_backward) or completion of the planned wave folds them in"""
    import torch

    P = small_problem()
    sg, data = P["sg_cfgs"], P["data"]
    bwd = band_backward(P, subgrid_configs=sg, lru_backward=lru_backward)
    for i in range(len(sg)):
        bwd.add_new_subgrid_task(sg[i], data[i])
        for _key, staged in bwd.lru._items.items():  # pylint: disable=protected-access
            assert staged["buf"].dtype == torch.complex128
    got = finished(bwd)
    pass_rule(f"single adds, lru_backward={lru_backward}", got, P["want"], P["e_ref"])
    # the same kernels on the same waves; only the order of the subgrids inside a wave (row tables) may differ
    d = relrms(got, whole_waves_result(P))
    print(f"C128BWD single adds lru_backward={lru_backward} vs whole waves: {d:.3e}")
    assert d <= 1e-13


def test_backward_small_without_a_plan_delayed_and_in_chunks():
    P = small_problem()
    sg, data, by1 = P["sg_cfgs"], P["data"], P["by1"]
    yN = P["cfg"].core.yN_size
    # no plan: the band is the whole padded axis
    bwd = band_backward(P)
    bwd.add_new_subgrid_tasks([sg[i] for i in by1], [data[i] for i in by1])
    assert bwd.bands.band == (0, yN)
    pass_rule("no plan (whole-axis band)", finished(bwd), P["want"], P["e_ref"])
    # delayed=True: DeviceTask handles
    bwd = band_backward(P, subgrid_configs=sg, delayed=True)
    bwd.add_new_subgrid_tasks([sg[i] for i in by1], [data[i] for i in by1])
    tasks = bwd.finish()
    assert all(hasattr(t, "compute") for t in tasks)
    pass_rule("delayed=True", numpy.array([numpy.asarray(t.compute()) for t in tasks]), P["want"], P["e_ref"])
    # accumulate_chunks: every wave's contributions in two chunks
    bwd = band_backward(P, subgrid_configs=sg)
    for off1 in sorted({c.off1 for c in sg}):
        wave = [i for i in by1 if sg[i].off1 == off1]
        halves = [wave[: len(wave) // 2], wave[len(wave) // 2:]]
        chunks = []
        for half in halves:
            parts = bwd.wave_contributions([sg[i] for i in half], [data[i] for i in half])
            chunks.append(([sg[i] for i in half], parts))
        assert chunks[0][1].data_ptr() != chunks[1][1].data_ptr()
        bwd.accumulate_chunks(off1, chunks)
    pass_rule("accumulate_chunks, two chunks", finished(bwd), P["want"], P["e_ref"])


def test_backward_small_sparse_plan_with_duplicates():
    """a sparse subgrid set (band shorter than the padded axis, wrapped offsets) with duplicates (up to three sources per
    padded row: the row tables split into groups), as test_backward_band_sparse_plan_and_overlaps builds it"""
    P = small_problem()
    sw, cfg, facet_cfgs, sg = P["sw"], P["cfg"], P["facet_cfgs"], P["sg_cfgs"]
    keep = [c for c in sg if c.off1 in (0, 192, 960)][:14]
    keep = keep + keep[:3] + keep[:2]
    assert len({c.off1 for c in keep}) < len({c.off1 for c in sg})
    vectors = [sep.subgrid_vectors(1300 + i, c.size, rank=2) for i, c in enumerate(keep)]
    data = [subgrid128(v, c) for v, c in zip(vectors, keep)]
    oracle = sep.SeparableBackwardOracle(P["ref"], facet_cfgs, keep, vectors)
    want = numpy.array([oracle.facet(j) for j in range(len(facet_cfgs))])
    b0 = sw.SwiftlyBackward(cfg, facet_cfgs, wave_axis=0)
    b0.add_new_subgrid_tasks(keep, data)
    e_ref = relrms(numpy.array([t.cpu().numpy() for t in b0.finish()]), want)
    b1 = band_backward(P, subgrid_configs=keep)
    by1 = sorted(range(len(keep)), key=lambda i: keep[i].off1)
    b1.add_new_subgrid_tasks([keep[i] for i in by1], [data[i] for i in by1])
    assert b1.bands.band[1] < cfg.core.yN_size
    pass_rule("sparse plan with duplicates", finished(b1), want, e_ref)


def test_backward_band_without_a_split_instance():
    """(m, xM) = (64, 256) has no complex128 split_prepare_facets instance: the contributions come from the general launch
    sequence and the band schedule runs all the same; 2 facets, 4 subgrids in 2 waves, whole facets against the oracle"""
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    p = dict(W=11.0, fov=1.0, N=2048, yB_size=352, yN_size=512, xA_size=192, xM_size=256)
    cfg = sw.SwiftlyConfig(backend="hip", **p)
    core = cfg.core
    xA, yB = p["xA_size"], p["yB_size"]
    assert core.xM_yN_size == 64 and not core.supports_split_prepare(torch.complex128, 2)
    assert core.supports_backward_band(torch.complex128, explicit=True)
    facet_cfgs = [sw.FacetConfig(0, 0, yB), sw.FacetConfig(yB, -yB, yB)]
    sg_cfgs = [sw.SubgridConfig(o0, o1, xA) for o0, o1 in ((0, 0), (3 * xA, 0), (5 * xA, xA), (-2 * xA, xA))]
    vectors = [sep.subgrid_vectors(1700 + i, xA, rank=2) for i in range(len(sg_cfgs))]
    data = [subgrid128(v, c) for v, c in zip(vectors, sg_cfgs)]
    oracle = sep.SeparableBackwardOracle(orc.OracleCore(p["W"], p["N"], p["xM_size"], p["yN_size"]), facet_cfgs, sg_cfgs, vectors)
    want = numpy.array([oracle.facet(j) for j in range(2)])
    b0 = sw.SwiftlyBackward(cfg, facet_cfgs, wave_axis=0)
    b0.add_new_subgrid_tasks(sg_cfgs, data)
    e_ref = relrms(finished(b0), want)
    b1 = sw.SwiftlyBackward(cfg, facet_cfgs, wave_axis=1, subgrid_configs=sg_cfgs, dtype=torch.complex128)
    b1.add_new_subgrid_tasks(sg_cfgs, data)
    assert "work" not in b1.splitter._wsbuf  # the general launch sequence, not wave_split_subgrids
    pass_rule("(64, 256): no split instance", finished(b1), want, e_ref)


def test_backward_64k_n16k_1k():
    """64k[1]-n16k-1k (W = 13.5625): 2 facets of 13312^2, 4 planned subgrids in 2 waves with neighbouring off1 -- the
    (256, 1024) split instance, the 7+7 gather-sum four-step and the long-row finish; 64 seeded rows per facet against the
    separable oracle, and the whole facets against the complex128 reference schedule"""
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    p, facet_cfgs, _, _ = fwd128._large_problem("64k[1]-n16k-1k", 2)
    xA, yB = p["xA_size"], p["yB_size"]
    sg_cfgs = [sw.SubgridConfig(o0, o1, xA) for o0, o1 in ((0, 0), (3 * xA, 0), (10 * xA, xA), (-7 * xA, xA))]
    vectors = [sep.subgrid_vectors(1500 + i, xA, rank=2) for i in range(len(sg_cfgs))]
    data = [subgrid128(v, c) for v, c in zip(vectors, sg_cfgs)]
    cfg = sw.SwiftlyConfig(backend="hip", **p)
    core = cfg.core
    assert core.supports_backward_band(torch.complex128, explicit=True) and core.supports_split_prepare(torch.complex128, 2)
    assert (core.xM_yN_size, core.xM_size, core.yN_size) == (256, 1024, 16384)
    oracle = sep.SeparableBackwardOracle(orc.OracleCore(p["W"], p["N"], p["xM_size"], p["yN_size"]), facet_cfgs, sg_cfgs, vectors)
    rows = [numpy.sort(numpy.random.default_rng(1600 + j).choice(yB, 64, replace=False)) for j in range(2)]
    want = numpy.array([oracle.facet_rows(j, rows[j]) for j in range(2)])
    b1 = sw.SwiftlyBackward(cfg, facet_cfgs, wave_axis=1, subgrid_configs=sg_cfgs, dtype=torch.complex128)
    b1.add_new_subgrid_tasks(sg_cfgs, data)
    assert b1.bands.band[1] < core.yN_size and b1.bands.bands.dtype == torch.complex128
    out1 = b1.finish()
    del b1
    b0 = sw.SwiftlyBackward(cfg, facet_cfgs, wave_axis=0)
    b0.add_new_subgrid_tasks(sg_cfgs, data)
    out0 = b0.finish()
    del b0
    assert all(t.dtype == torch.complex128 and tuple(t.shape) == (yB, yB) for t in out1 + out0)
    pick = lambda outs: numpy.array([outs[j][torch.from_numpy(rows[j]).cuda()].cpu().numpy() for j in range(2)])
    e_ref = relrms(pick(out0), want)
    pass_rule("64k[1]-n16k-1k, 64 rows per facet", pick(out1), want, e_ref)
    num = sum(float((a - b).abs().pow(2).sum()) for a, b in zip(out1, out0))
    den = sum(float(b.abs().pow(2).sum()) for b in out0)
    sched = (num / den) ** 0.5
    print(f"C128BWD pass 64k[1]-n16k-1k wave_axis=1 vs 0, whole facets: {sched:.3e}")
    # two results that each lie within PASS_TOL of the exact one
    assert sched <= 2 * PASS_TOL


# -------------------------------------------------------------------------------------------- (e) defaults and refusals
def test_defaults_and_refusals():
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    p = SMALL
    cfg = sw.SwiftlyConfig(backend="hip", **p)
    xA, yB = p["xA_size"], p["yB_size"]
    facet_cfgs = [sw.FacetConfig(0, 0, yB), sw.FacetConfig(yB, 0, yB)]
    sg = sw.SubgridConfig(0, 0, xA)
    d128 = torch.zeros((xA, xA), dtype=torch.complex128, device="cuda")
    d64 = d128.to(torch.complex64)
    # wave_axis=1 alone is no request for complex128
    with pytest.raises(ValueError):
        sw.SwiftlyBackward(cfg, facet_cfgs, wave_axis=1).add_new_subgrid_task(sg, d128)
    # nothing picks the band schedule by itself in complex128
    for dt in (torch.complex128, numpy.complex128):
        bwd = sw.SwiftlyBackward(cfg, facet_cfgs, subgrid_configs=[sg], dtype=dt)
        bwd.add_new_subgrid_task(sg, d128)
        assert bwd.wave_axis == 0 and bwd.finish()[0].dtype == torch.complex128
    # dtype=None keeps the automatic choice for complex64 data, and an explicit complex64 is the same request
    for kw in ({}, dict(dtype=torch.complex64)):
        bwd = sw.SwiftlyBackward(cfg, facet_cfgs, subgrid_configs=[sg], **kw)
        bwd.add_new_subgrid_task(sg, d64)
        assert bwd.wave_axis == 1 and bwd.finish()[0].dtype == torch.complex64
    # no silent conversion on the explicit band schedule: single adds (staged), whole waves and contributions
    with pytest.raises(ValueError, match="complex64"):
        sw.SwiftlyBackward(cfg, facet_cfgs, wave_axis=1, dtype=torch.complex128).add_new_subgrid_task(sg, d64)
    with pytest.raises(ValueError, match="complex64"):
        sw.SwiftlyBackward(cfg, facet_cfgs, wave_axis=1, dtype=torch.complex128).add_new_subgrid_tasks([sg, sg], [d64, d64])
    with pytest.raises(ValueError, match="complex64"):
        m = cfg.core.xM_yN_size
        parts = torch.zeros((2, 1, m, m), dtype=torch.complex64, device="cuda")
        sw.SwiftlyBackward(cfg, facet_cfgs, wave_axis=1, dtype=torch.complex128).accumulate_wave([sg], parts)
    # ... and not only at the first data: complex64 contributions after a complex128 wave has created the accumulators
    bwd = sw.SwiftlyBackward(cfg, facet_cfgs, wave_axis=1, dtype=torch.complex128)
    p128 = bwd.wave_contributions([sg], [d128])
    assert p128.dtype == torch.complex128 and "work" in bwd.splitter._wsbuf  # (the split kernel, on the explicit schedule only)
    bwd.accumulate_wave([sg], p128)
    assert bwd.bands.bands is not None
    for call in (lambda: bwd.accumulate_wave([sg], p128.to(torch.complex64)),
                 lambda: bwd.accumulate_chunks(sg.off1, [([sg], p128), ([sg], p128.to(torch.complex64))]),
                 lambda: bwd.add_new_subgrid_tasks([sg, sg], [d64, d64]),
                 lambda: bwd.add_new_subgrid_task(sg, d64)):
        with pytest.raises(ValueError, match="complex64"):
            call()
    core = cfg.core
    with pytest.raises(ValueError, match="complex64"):
        core.accumulate_facet_columns(p128.to(torch.complex64), core.xM_yN_size, [0], [0], core.column_row_sources([0])[0][1],
                                      [0, 0], yB, None, 0, bwd.bands.bands, bwd.bands.band)
    assert all(t.dtype == torch.complex128 for t in bwd.finish())
    # every complex128 path that existed before keeps the general launch sequence for its contributions
    for kw in (dict(wave_axis=0), dict(subgrid_configs=[sg]), dict(wave_axis=0, dtype=torch.complex128)):
        old = sw.SwiftlyBackward(cfg, facet_cfgs, **kw)
        assert old.wave_contributions([sg], [d128]).dtype == torch.complex128 and "work" not in old.splitter._wsbuf, kw
    with pytest.raises(ValueError):
        sw.SwiftlyBackward(cfg, facet_cfgs, wave_axis=1, dtype=torch.float64)
    # facets of two sizes
    with pytest.raises(ValueError, match="one size"):
        two = [sw.FacetConfig(0, 0, yB), sw.FacetConfig(yB, 0, yB - 32)]
        sw.SwiftlyBackward(cfg, two, wave_axis=1, dtype=torch.complex128).add_new_subgrid_tasks([sg, sg], [d128, d128])
    # yN = 65536 and yN = 3 * 2^10: the reason comes from the capability table
    for q in (dict(W=10.875, fov=1.0, N=131072, yB_size=1024, yN_size=65536, xA_size=928, xM_size=1024),
              dict(W=11.0, fov=1.0, N=6144, yB_size=2112, yN_size=3072, xA_size=1792, xM_size=2048)):
        cq = sw.SwiftlyConfig(backend="hip", **q)
        assert cq.core.supports_backward_band(torch.complex64) and not cq.core.supports_backward_band(torch.complex128, explicit=True)
        with pytest.raises(ValueError, match="complex128 backward band"):
            bwd = sw.SwiftlyBackward(cq, [sw.FacetConfig(0, 0, q["yB_size"])], wave_axis=1, dtype=torch.complex128)
            bwd.add_new_subgrid_task(sw.SubgridConfig(0, 0, q["xA_size"]),
                                     torch.zeros((q["xA_size"],) * 2, dtype=torch.complex128, device="cuda"))
