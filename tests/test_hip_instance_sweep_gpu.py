"""
Every compiled instance of the fused subgrid-side kernels against the 1-D oracle.

The fused pipelines pick their kernels from compile-time tables: ``SF_PAIRS`` / ``SF_PAIRS_C128`` in csrc/swiftly_caps.h
((log2 m, log2 xM) pairs of sum_finish_rows, sum_finish_facets and split_prepare_facets) and the column-pass dispatcher
of csrc/col_pass.hip.  Each pair has its own threads per row, rows per workgroup, LDS layout and (from xM = 4096) the
wave-parallel form with rounds of disjoint placement windows.  This module runs one small synthetic core per pair (table
``PAIRS``; W = 11, ``m = xM * yN / N``) through the C ABI entry points one by one and compares every result with a
composition of the complex128 primitives of oracle/swiftly_oracle.py -- composed as test_sum_finish_facets
(test_hip_band_pipeline_gpu.py) and test_sum_finish_facets_and_subgrid_side_c128 (test_hip_c128_band_pipeline_gpu.py) do.
No expected value comes from another HIP path; the only exception is the bit-identity of the chunked four-step.

Inputs are chosen to hit the host-side arithmetic next to the kernels: odd subgrid size, partial masks, two facets that
share ``off1`` (summed before the m-point transform), negative ``off0`` / ``off1`` on both sides, an ``off1`` close to
``N``, a placement window and a first row (``base0``) that wrap the ring, padded strides with sentinels, the 64-facet and
64-subgrid limits, and for (10, 12) placement windows that need three rounds.

Bounds
* complex128: ``max|err| / max|want| <= 5e-12`` (``C128_TOL`` of the complex128 module; measured ~5e-16).
* complex64 against the complex128 oracle, relative RMSE over the whole output: at (7, 8) 2e-6 for one transform
  (transform_contributions, add_to_subgrid_from_columns, the split kernels) and 3e-6 for sum_finish (rows / facets), as in
  the existing tests; for larger pairs times ``sqrt((log2 m + log2 xM) / 15)`` -- transform rounding grows with the square
  root of the stage count -- which gives 3.6e-6 at (10, 12).  In addition ``max|err| <= 2e-5 * max|want|`` per subgrid.
* whole subgrid side in complex64 (wave_subgrid_side): the 3e-6 of sum_finish_facets covers the stages of K3, the
  m-point and the xM-point transform of the kernel (2 log2 m + log2 xM = 22 at (7, 8)); the axis-0 finish adds another
  log2 xM (30 at (7, 8)).  By the same square-root rule: ``3e-6 * sqrt(30 / 22) = 3.5e-6`` at (7, 8), then the pair scale.
None of the bounds was tuned against the kernels.

Measured on an MI355X (complex64: relative RMSE, complex128: max|err| / max|want|; "K3" = transform_contributions,
"facets" = sum_finish_facets, "side" = wave_subgrid_side, "placed" =
its placed mode, "rows" = sum_finish_rows with 8 groups, "cols" = add_to_subgrid_from_columns with 8 groups, "split" =
split_prepare_facets, "wsplit" = wave_split_subgrids):

    m    xM  dtype       K3   facets     side   placed     cols     rows    split   wsplit
  128   256  c64    1.0e-07  1.9e-07  2.3e-07  1.5e-07  1.0e-07  1.9e-07  1.9e-07  2.3e-07
  128  1024  c64    9.9e-08  2.0e-07  2.6e-07  1.9e-07  1.0e-07  2.0e-07  2.0e-07  2.6e-07
  256   512  c64    1.1e-07  2.0e-07  2.5e-07  1.7e-07  1.1e-07  2.1e-07  2.1e-07  2.5e-07
  256  1024  c64    1.1e-07  2.1e-07  2.7e-07  1.9e-07  1.1e-07  2.2e-07  2.1e-07  2.7e-07
  512  1024  c64    1.2e-07  2.3e-07  2.9e-07  1.9e-07  1.2e-07  2.3e-07  2.3e-07  2.9e-07
  512  2048  c64    1.2e-07  2.4e-07  2.9e-07  1.9e-07  1.2e-07  2.4e-07  2.4e-07  3.0e-07
 1024  2048  c64    1.3e-07  2.6e-07  3.2e-07  2.0e-07  1.3e-07  2.6e-07  2.6e-07  3.2e-07
 1024  4096  c64    1.3e-07  2.7e-07  3.3e-07        -  1.3e-07  2.6e-07  2.7e-07  3.3e-07
  128   256  c128   3.3e-16  4.7e-16  5.3e-16        -        -        -        -        -
  128  1024  c128   3.1e-16  5.4e-16  5.3e-16        -        -        -        -        -
  256   512  c128   3.6e-16  5.4e-16  5.9e-16        -        -        -        -        -
  256  1024  c128   3.9e-16  6.8e-16  6.2e-16        -        -        -        -        -
  512  1024  c128   3.4e-16  5.8e-16  6.1e-16        -        -        -        -        -

Limits at (7, 8), axis-1 workspace / whole side: 1 facet: complex64 1.9e-07 / 2.3e-07, complex128 4.4e-16 / 5.4e-16;
64 facets: complex64 1.9e-07 / 2.3e-07, complex128 5.6e-16 / 6.2e-16;
65 subgrids: complex64 1.8e-07 / 2.3e-07, complex128 5.3e-16 / 5.8e-16;
subgrid_size = xM: complex64 1.9e-07 / 2.3e-07, complex128 5.4e-16 / 5.2e-16.
With 1 group at (7, 8): cols 1.0e-07, rows 1.8e-07.

prepare_facet_columns in complex128 (case f), all rows / row map:
yN 128: 3.4e-16 / 3.4e-16, 256: 3.7e-16 / 3.9e-16, 512: 3.4e-16 / 3.5e-16, 1024: 3.5e-16 / 3.6e-16,
2048: 3.4e-16 / 3.8e-16, 4096: 4.0e-16 / 4.2e-16, 8192: 4.9e-16 / 4.1e-16, 32768: 5.2e-16 / 5.1e-16;
chunked four-step on / off at 8192 and 32768 points: bit-identical.

Module wall time on an MI355X: 50 s for the 87 cases (pytest's own figure; 52 s for the process).
"""
import os
import subprocess
import sys

import numpy
import pytest

from oracle import swiftly_oracle as orc

pytestmark = pytest.mark.gpu

W = 11.0
#: one synthetic core per (log2 m, log2 xM) pair of SF_PAIRS (csrc/swiftly_caps.h); all accepted by swiftly_hip_create
PAIRS = {
    (7, 8): dict(N=1024, yN=512, xM=256),
    (7, 10): dict(N=4096, yN=512, xM=1024),
    (8, 9): dict(N=2048, yN=1024, xM=512),
    (8, 10): dict(N=4096, yN=1024, xM=1024),
    (9, 10): dict(N=2048, yN=1024, xM=1024),
    (9, 11): dict(N=8192, yN=2048, xM=2048),
    (10, 11): dict(N=4096, yN=2048, xM=2048),
    (10, 12): dict(N=8192, yN=2048, xM=4096),
}
#: pairs with a complex128 sum_finish_facets instance (SF_PAIRS_C128)
PAIRS_C128 = [(7, 8), (7, 10), (8, 9), (8, 10), (9, 10)]
C128_TOL = 5e-12
SENTINEL = complex(7.5, -3.25)

CASES = [(p, "c64") for p in PAIRS] + [(p, "c128") for p in PAIRS_C128]
CASE_IDS = [f"m{1 << p[0]}-xM{1 << p[1]}-{d}" for p, d in CASES]
PAIR_IDS = [f"m{1 << p[0]}-xM{1 << p[1]}" for p in PAIRS]


def pair_scale(pair):
    """growth of the float32 transform rounding with the stage count, relative to (7, 8)"""
    return float(numpy.sqrt((pair[0] + pair[1]) / 15.0))


def relrms(got, want):
    return float(numpy.sqrt(numpy.mean(numpy.abs(got - want) ** 2) / numpy.mean(numpy.abs(want) ** 2)))


def maxrel(got, want):
    return float(numpy.max(numpy.abs(got - want)) / numpy.max(numpy.abs(want)))


def _record(what, pair, dtype, value, bound):
    print(f"SWEEP {what:<24s} m={1 << pair[0]:<5d} xM={1 << pair[1]:<5d} {dtype:<5s} {value:.3e} (bound {bound:.2e})")


def _check(what, pair, dtype, got, want, rms_bound):
    """``got`` / ``want``: numpy ``[S, ...]`` (first axis = subgrid).  complex128: max error; complex64: relative RMSE of
    the whole output and the per-subgrid max error."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if dtype == "c128":
        assert got.dtype == numpy.complex128
        err = maxrel(got, want)
        _record(what, pair, dtype, err, C128_TOL)
        assert err <= C128_TOL, (what, pair, err)
        return err
    assert got.dtype == numpy.complex64
    err = relrms(got, want)
    bound = rms_bound * pair_scale(pair)
    _record(what, pair, dtype, err, bound)
    peaks = [float(numpy.max(numpy.abs(got[b] - want[b])) / numpy.max(numpy.abs(want[b]))) for b in range(want.shape[0])]
    assert err < bound, (what, pair, err, bound)
    assert max(peaks) <= 2e-5, (what, pair, peaks)
    return err


_CORES = {}


def cores(pair):
    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    if pair not in _CORES:
        p = PAIRS[pair]
        core = SwiftlyCoreHip(W, p["N"], p["xM"], p["yN"])
        assert (core.xM_yN_size, core.xM_size) == (1 << pair[0], 1 << pair[1])
        _CORES[pair] = (core, orc.OracleCore(W, p["N"], p["xM"], p["yN"]))
    return _CORES[pair]


def _tdtype(dtype):
    import torch

    return torch.complex64 if dtype == "c64" else torch.complex128


def _ndtype(dtype):
    return numpy.complex64 if dtype == "c64" else numpy.complex128


def _crandn(rng, shape, dtype):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(_ndtype(dtype))


# ------------------------------------------------------------------------------------------------- the common problem
def offsets(pair):
    """facet offsets ``[(off0, off1)] * 5`` and subgrid offsets ``[(off0, off1)] * 3`` of the sweep for one core.

    In units of the offset steps (``s' = off * xM // N`` on the ring of xM, ``s = off * yN // N`` on the ring of yN):
    facets 0 and 1 share off1 (summed before the m-point transform); facet 2 has a negative off0 and an off1 whose
    placement window ``[xM/2 - m/2 + s', +m)`` wraps the ring; facet 3 has an off0 whose first row ``base0`` sits m/2 + 2
    below the end of the ring (its band wraps) and a negative off1; the off1 of facet 4 is three steps below N."""
    p = PAIRS[pair]
    N, xM, yN = p["N"], p["xM"], p["yN"]
    fstep, sstep = N // xM, N // yN
    f_sp = [(0, 0), (xM // 3, 0), (-(xM // 5), xM // 2 + 1), (xM // 2 - 2, -(xM // 6)), (xM // 7, xM - 3)]
    s_s = [(0, 0), (yN // 5, yN // 3), (-(yN // 7), -(yN // 9))]
    return [(a * fstep, b * fstep) for a, b in f_sp], [(a * sstep, b * sstep) for a, b in s_s]


def placement_rounds(off1s, N, xM, m):
    """the rounds of fill_group_rounds (csrc/swiftly_abi_internal.h) from the same arithmetic: groups = distinct off1 in
    ascending order, ``s' = off1 * xM // N``, windows of m on a ring of xM, greedy in group order"""
    sps = [o * xM // N for o in sorted(set(off1s))]

    def overlap(a, b):
        d = (b - a) % xM
        return d < m or xM - d < m

    rounds = []
    for sp in sps:
        for r in rounds:
            if not any(overlap(sp, o) for o in r):
                r.append(sp)
                break
        else:
            rounds.append([sp])
    return rounds, overlap


def G_want(ref, C, off0):
    """Fn * cfft_m(C, axis 0) rotated by the facet offset, without placement: rows of add_to_subgrid(axis 0)."""
    m, xM = ref.xM_yN_size, ref.xM_size
    placed = ref.add_to_subgrid(C, off0, axis=0)
    sp = off0 * xM // ref.N
    return placed[(numpy.arange(m) + xM // 2 - m // 2 + sp) % xM]


def finish_rows(ref, acc, off1, xA):
    """finish_subgrid along axis 1 of every row"""
    return numpy.array([ref.finish_subgrid(acc[r], off1, xA) for r in range(acc.shape[0])])


def finish_cols(ref, tmp, off0, xA):
    """finish_subgrid along axis 0 of every column"""
    return numpy.array([ref.finish_subgrid(tmp[:, c], off0, xA) for c in range(tmp.shape[1])]).T


_PROBLEMS = {}


def problem(pair, dtype, f_offs=None, s_offs=None, xA=None, seed=0):
    """inputs and oracle results of cases (a) and (b): contributions ``[F, S, m, m]`` -> ``G`` -> axis-1 finished rows
    ``[S, xM, xA]`` -> subgrids ``[S, xA, xA]``; cached for the default offsets (shared by the tests of one pair)"""
    key = (pair, dtype)
    default = f_offs is None and s_offs is None and xA is None
    if default and key in _PROBLEMS:
        return _PROBLEMS[key]
    _, ref = cores(pair)
    m, xM = ref.xM_yN_size, ref.xM_size
    d_f, d_s = offsets(pair)
    f_offs = d_f if f_offs is None else f_offs
    s_offs = d_s if s_offs is None else s_offs
    xA = xM - 2 * (xM // 8) - 1 if xA is None else xA
    F, S = len(f_offs), len(s_offs)
    rng = numpy.random.default_rng(1000 * pair[0] + 10 * pair[1] + seed)
    contrib = _crandn(rng, (F, S, m, m), dtype)
    mask1 = (rng.random((S, xA)) > 0.2).astype(float)
    mask0 = (rng.random((S, xA)) > 0.2).astype(float)
    G = numpy.empty((F, S, m, m), dtype=complex)
    want1 = numpy.empty((S, xM, xA), dtype=complex)
    want = numpy.empty((S, xA, xA), dtype=complex)
    k = numpy.arange(m)
    for b in range(S):
        acc = numpy.zeros((xM, xM), dtype=complex)
        for f, (o0, o1) in enumerate(f_offs):
            C = contrib[f, b].astype(complex)
            G[f, b] = G_want(ref, C, o0)
            # acc += add_to_subgrid(add_to_subgrid(C, o0, 0), o1, 1), the axis-1 step only on the m rows that the axis-0
            # step fills (G_want reads exactly those; every other row is zero and stays zero)
            acc[(k + xM // 2 - m // 2 + o0 * xM // ref.N) % xM] += ref.add_to_subgrid(G[f, b], o1, 1)
        want1[b] = finish_rows(ref, acc, s_offs[b][1], xA) * mask1[b][None, :]
        want[b] = finish_cols(ref, want1[b], s_offs[b][0], xA) * mask0[b][:, None]
    prob = dict(f_offs=f_offs, s_offs=s_offs, xA=xA, contrib=contrib, mask0=mask0, mask1=mask1, G=G, want1=want1, want=want)
    if default:
        _PROBLEMS[key] = prob
    return prob


def padded_blocks(F, S, m, tdtype, row_pad=0):
    """``[F, S, m, m]`` view with padded facet and subgrid strides (and a padded row stride when ``row_pad``) of a
    buffer filled with the sentinel; returns ``(view, buffer)``"""
    import torch

    buf = torch.full((F, S + 1, m * (m + row_pad) + 64), SENTINEL, dtype=tdtype, device="cuda")
    if row_pad:
        view = buf[:, :S, : m * (m + row_pad)].view(F, S, m, m + row_pad)[..., :m]
    else:
        view = buf[:, :S, : m * m].view(F, S, m, m)
    return view, buf


def blocks_padding_intact(buf, S, used):
    return bool((buf[:, S] == SENTINEL).all()) and bool((buf[:, :, used:] == SENTINEL).all())


def mask_tensor(mask, tdtype):
    import torch

    return torch.from_numpy(mask).to(device="cuda", dtype=torch.float32 if tdtype == torch.complex64 else torch.float64)


def run_transform(core, prob, dtype):
    """transform_contributions (layout 2) into a padded view; returns the device view"""
    import torch

    tdtype = _tdtype(dtype)
    F, S, m, _ = prob["contrib"].shape
    src, _ = padded_blocks(F, S, m, tdtype)
    src.copy_(torch.from_numpy(prob["contrib"]).cuda())
    G, gbuf = padded_blocks(F, S, m, tdtype)
    res = core.transform_contributions(src, 2, [o[0] for o in prob["f_offs"]], None, out=G, nsub=S)
    assert res is G and res.dtype == tdtype and tuple(res.shape) == (F, S, m, m)
    assert blocks_padding_intact(gbuf, S, m * m), "transform_contributions wrote outside its blocks"
    return G


# ------------------------------------------------------------------ (a) transform_contributions + sum_finish_facets
@pytest.mark.parametrize("pair,dtype", CASES, ids=CASE_IDS)
def test_transform_contributions_and_sum_finish_facets(pair, dtype):
    import torch

    core, ref = cores(pair)
    tdtype = _tdtype(dtype)
    m, xM, N = ref.xM_yN_size, ref.xM_size, ref.N
    prob = problem(pair, dtype)
    f_offs, s_offs, xA = prob["f_offs"], prob["s_offs"], prob["xA"]
    F, S = len(f_offs), len(s_offs)
    assert xA % 2 == 1 and F == 5 and S == 3 and f_offs[0][1] == f_offs[1][1]
    assert any(o[0] < 0 for o in f_offs) and any(o[1] < 0 for o in f_offs) and any(s[1] < 0 for s in s_offs)
    # a first row and a placement window that wrap the ring, an off1 close to N
    assert any((xM // 2 - m // 2 + o[0] * xM // N) % xM + m > xM for o in f_offs)
    assert any((xM // 2 - m // 2 + o[1] * xM // N) % xM + m > xM for o in f_offs)
    assert any(N - 4 * core.facet_off_step < o[1] < N for o in f_offs)
    if pair == (10, 12):
        # wave-parallel form: at least two rounds, one of them with two groups (two overlapping windows and one that is
        # disjoint from both)
        rounds, overlap = placement_rounds([o[1] for o in f_offs], N, xM, m)
        sps = sorted({o[1] * xM // N for o in f_offs})
        assert len(rounds) >= 2 and max(len(r) for r in rounds) >= 2, rounds
        assert any(overlap(a, b) and not overlap(a, c) and not overlap(b, c)
                   for a in sps for b in sps for c in sps if len({a, b, c}) == 3), sps

    G = run_transform(core, prob, dtype)
    _check("transform_contributions", pair, dtype, G.cpu().numpy().transpose(1, 0, 2, 3), prob["G"].transpose(1, 0, 2, 3),
           2e-6)

    # sum_finish_facets: input with a padded row stride too, output a view with padded row and subgrid strides
    Gp, _ = padded_blocks(F, S, m, tdtype, row_pad=8)
    Gp.copy_(G)
    assert Gp.stride(2) == m + 8
    obuf = torch.full((S, xM + 1, xA + 3), SENTINEL, dtype=tdtype, device="cuda")
    out = obuf[:, :xM, :xA]
    res = core.sum_finish_facets(Gp, [o[0] for o in f_offs], [o[1] for o in f_offs], out, [s[1] for s in s_offs], xA,
                                 mask=mask_tensor(prob["mask1"], tdtype))
    assert res is out and res.dtype == tdtype and tuple(res.shape) == (S, xM, xA)
    assert bool((obuf[:, xM] == SENTINEL).all()) and bool((obuf[:, :, xA:] == SENTINEL).all()), \
        "sum_finish_facets wrote outside its rows"
    _check("sum_finish_facets", pair, dtype, out.cpu().numpy(), prob["want1"], 3e-6)


# ------------------------------------------------------------------------------------------- (b) wave_subgrid_side
SIDE_TOL = 3e-6 * float(numpy.sqrt(30.0 / 22.0))  # see the module docstring


def _run_side(core, G, prob, dtype, placed=False):
    import torch

    tdtype = _tdtype(dtype)
    f_offs, s_offs, xA = prob["f_offs"], prob["s_offs"], prob["xA"]
    S, xM = len(s_offs), core.xM_size
    tmp = torch.empty((S, xM, xA), dtype=tdtype, device="cuda")
    res = torch.empty((S, xA, xA), dtype=tdtype, device="cuda")
    got = core.wave_subgrid_side(G, [o[0] for o in f_offs], [o[1] for o in f_offs], [s[0] for s in s_offs],
                                 [s[1] for s in s_offs], xA, mask_tensor(prob["mask0"], tdtype),
                                 mask_tensor(prob["mask1"], tdtype), tmp, res, placed=placed)
    assert got is res and got.dtype == tdtype and tuple(got.shape) == (S, xA, xA)
    return res, tmp


@pytest.mark.parametrize("pair,dtype", CASES, ids=CASE_IDS)
def test_wave_subgrid_side(pair, dtype):
    """both axes of the subgrid side (sum_finish_facets + the axis-0 finish) on the inputs of case (a)"""
    core, _ = cores(pair)
    prob = problem(pair, dtype)
    G = run_transform(core, prob, dtype)
    res, tmp = _run_side(core, G, prob, dtype)
    _check("side axis 1 (workspace)", pair, dtype, tmp.cpu().numpy(), prob["want1"], 3e-6)
    _check("wave_subgrid_side", pair, dtype, res.cpu().numpy(), prob["want"], SIDE_TOL)


def placed_blocks(ref, prob):
    """the blocks the axis-1-first pipeline hands to the subgrid side, from the oracle: along the contiguous axis the
    rows already are ``Z[k] = Fn[k] * cfft_m(x)[(k + s'1) mod m]`` -- add_to_subgrid(axis 1) read back from its placement,
    as test_finish_axis1_rows_matches_oracle does -- and along axis 0 what transform_contributions gives"""
    m, xM = ref.xM_yN_size, ref.xM_size
    k = numpy.arange(m)
    F, S = prob["contrib"].shape[:2]
    out = numpy.empty((F, S, m, m), dtype=complex)
    for f, (o0, o1) in enumerate(prob["f_offs"]):
        sp = o1 * xM // ref.N
        for b in range(S):
            placed = ref.add_to_subgrid(prob["contrib"][f, b].astype(complex), o1, 1)  # [m, xM]
            Z = placed[:, (k + xM // 2 - m // 2 + sp) % xM]
            out[f, b] = G_want(ref, Z, o0)
    return out


@pytest.mark.parametrize("pair", [p for p in PAIRS if p[1] <= 11], ids=[i for p, i in zip(PAIRS, PAIR_IDS) if p[1] <= 11])
def test_wave_subgrid_side_placed(pair):
    """placed mode (axis-1-first pipeline) of the register-form instances: the same subgrids as the unplaced call"""
    import torch

    core, ref = cores(pair)
    prob = problem(pair, "c64")
    F, S, m, _ = prob["contrib"].shape
    G, gbuf = padded_blocks(F, S, m, torch.complex64)
    G.copy_(torch.from_numpy(placed_blocks(ref, prob).astype(numpy.complex64)).cuda())
    res, tmp = _run_side(core, G, prob, "c64", placed=True)
    assert blocks_padding_intact(gbuf, S, m * m)
    _check("placed axis 1 (workspace)", pair, "c64", tmp.cpu().numpy(), prob["want1"], 3e-6)
    _check("wave_subgrid_side placed", pair, "c64", res.cpu().numpy(), prob["want"], SIDE_TOL)


@pytest.mark.parametrize("pair,dtype", [((7, 8), "c128"), ((9, 10), "c128"), ((10, 12), "c64")],
                         ids=["m128-xM256-c128", "m512-xM1024-c128", "m1024-xM4096-c64"])
def test_wave_subgrid_side_placed_refusals(pair, dtype):
    """complex128 and the wave-parallel form (xM = 4096) have no placed mode"""
    import torch

    core, _ = cores(pair)
    m, xM, xA = core.xM_yN_size, core.xM_size, 33
    G = torch.zeros((1, 1, m, m), dtype=_tdtype(dtype), device="cuda")
    tmp = torch.empty((1, xM, xA), dtype=G.dtype, device="cuda")
    res = torch.empty((1, xA, xA), dtype=G.dtype, device="cuda")
    with pytest.raises(NotImplementedError):
        core.wave_subgrid_side(G, [0], [0], [0], [0], xA, None, None, tmp, res, placed=True)
    core.wave_subgrid_side(G, [0], [0], [0], [0], xA, None, None, tmp, res)  # (the unplaced call runs)
    assert float(res.abs().max()) == 0.0


# -------------------------------------------------------- (c) add_to_subgrid_from_columns + sum_finish_rows
@pytest.mark.parametrize("ngroups", [1, 8])
@pytest.mark.parametrize("pair", list(PAIRS), ids=PAIR_IDS)
def test_columns_and_sum_finish_rows(pair, ngroups):
    """the grouped subgrid side of the reference schedule: per-off1-group axis-0 sums ``colacc[G, S, xM, m]`` straight
    from column buffers, then the sum over groups + axis-1 finish; 1 group and kSumFinishMaxGroups = 8 groups"""
    import torch

    core, ref = cores(pair)
    m, xM, yN, N = ref.xM_yN_size, ref.xM_size, ref.yN_size, ref.N
    fstep, sstep = core.facet_off_step, core.subgrid_off_step
    xA = xM - 2 * (xM // 8) - 1
    rng = numpy.random.default_rng(77 + 100 * pair[0] + pair[1] + ngroups)
    off0 = -(xM // 5) * fstep
    # group offsets spread over the ring (negative ones, one three steps below N); subgrid offsets with a negative one
    g_sp = [-(xM // 6), 0, xM // 9, xM // 4 + 1, xM // 2 + 1, 5 * (xM // 8), 7 * (xM // 8), xM - 3][:ngroups]
    g_offs = [sp * fstep for sp in g_sp]
    s_off1 = [-(yN // 9) * sstep, (yN // 3) * sstep] if ngroups == 1 else [-(yN // 9) * sstep]
    S = len(s_off1)
    cols = _crandn(rng, (ngroups, m, yN), "c64")
    colacc = torch.zeros((ngroups, S, xM, m), dtype=torch.complex64, device="cuda")
    res = core.add_to_subgrid_from_columns(torch.from_numpy(cols).cuda(), off0, colacc, s_off1)
    assert res is colacc and res.dtype == torch.complex64 and tuple(res.shape) == (ngroups, S, xM, m)
    want_acc = numpy.empty((S, ngroups, xM, m), dtype=complex)
    for g in range(ngroups):
        for b in range(S):
            want_acc[b, g] = ref.add_to_subgrid(ref.extract_from_facet(cols[g].astype(complex), s_off1[b], axis=1), off0, 0)
    _check(f"columns {ngroups} group(s)", pair, "c64", colacc.cpu().numpy().transpose(1, 0, 2, 3), want_acc, 2e-6)

    # sum_finish_rows on a view with padded group, subgrid and row strides
    cbuf = torch.full((ngroups, S + 1, xM + 1, m + 8), SENTINEL, dtype=torch.complex64, device="cuda")
    cview = cbuf[:, :S, :xM, :m]
    cview.copy_(colacc)
    mask = (rng.random((S, xA)) > 0.2).astype(float)
    obuf = torch.full((S, xM + 1, xA + 3), SENTINEL, dtype=torch.complex64, device="cuda")
    out = obuf[:, :xM, :xA]
    res = core.sum_finish_rows(cview, g_offs, out, s_off1, xA, mask=mask_tensor(mask, torch.complex64))
    assert res is out and res.dtype == torch.complex64 and tuple(res.shape) == (S, xM, xA)
    assert bool((obuf[:, xM] == SENTINEL).all()) and bool((obuf[:, :, xA:] == SENTINEL).all())
    want = numpy.empty((S, xM, xA), dtype=complex)
    for b in range(S):
        acc = numpy.zeros((xM, xM), dtype=complex)
        for g in range(ngroups):
            acc += ref.add_to_subgrid(want_acc[b, g], g_offs[g], 1)
        want[b] = finish_rows(ref, acc, s_off1[b], xA) * mask[b][None, :]
    _check(f"rows {ngroups} group(s)", pair, "c64", out.cpu().numpy(), want, 3e-6)


def test_sum_finish_rows_refuses_nine_groups():
    import torch

    core, _ = cores((7, 8))
    m, xM, xA = core.xM_yN_size, core.xM_size, 191
    colacc = torch.zeros((9, 1, xM, m), dtype=torch.complex64, device="cuda")
    out = torch.empty((1, xM, xA), dtype=torch.complex64, device="cuda")
    with pytest.raises(NotImplementedError):
        core.sum_finish_rows(colacc, [g * core.facet_off_step for g in range(9)], out, [0], xA)
    core.sum_finish_rows(colacc[:8], [g * core.facet_off_step for g in range(8)], out, [0], xA)


# --------------------------------------------------------------- (d) split_prepare_facets + wave_split_subgrids
@pytest.mark.parametrize("pair", list(PAIRS), ids=PAIR_IDS)
def test_split_prepare_facets_and_wave_split_subgrids(pair):
    """the subgrid side of the backward pass against the oracle's prepare_subgrid and extract_from_subgrid on both axes
    (reference api_helper.py:115-139), with the wrapping offsets of case (a) and an odd subgrid size"""
    import torch

    core, ref = cores(pair)
    m, xM = ref.xM_yN_size, ref.xM_size
    f_offs, s_offs = offsets(pair)
    xA = xM - 2 * (xM // 8) - 1
    F, S = len(f_offs), len(s_offs)
    rng = numpy.random.default_rng(55 + 100 * pair[0] + pair[1])
    sub = _crandn(rng, (S, xA, xA), "c64")
    want = numpy.empty((S, F, m, m), dtype=complex)
    tmp_want = numpy.empty((S, xM, xA), dtype=complex)
    for b, (s0, s1) in enumerate(s_offs):
        x = sub[b].astype(complex)
        tmp_want[b] = numpy.array([ref.prepare_subgrid(x[:, c], s0) for c in range(xA)]).T  # axis 0 only
        P = ref.prepare_subgrid(x, [s0, s1])
        for f, (o0, o1) in enumerate(f_offs):
            want[b, f] = ref.extract_from_subgrid(ref.extract_from_subgrid(P, o0, 0), o1, 1)
    f0, f1 = [o[0] for o in f_offs], [o[1] for o in f_offs]
    # split_prepare_facets alone, from the oracle's axis-0 prepared subgrids (padded input strides)
    tbuf = torch.full((S, xM + 1, xA + 3), SENTINEL, dtype=torch.complex64, device="cuda")
    tview = tbuf[:, :xM, :xA]
    tview.copy_(torch.from_numpy(tmp_want.astype(numpy.complex64)).cuda())
    out, obuf = padded_blocks(F, S, m, torch.complex64)
    res = core.split_prepare_facets(tview, [s[1] for s in s_offs], f0, f1, out)
    assert res is out and res.dtype == torch.complex64 and tuple(res.shape) == (F, S, m, m)
    assert blocks_padding_intact(obuf, S, m * m)
    _check("split_prepare_facets", pair, "c64", out.cpu().numpy().transpose(1, 0, 2, 3), want, 2e-6)
    # the whole wave natively
    work = torch.empty(2 * S * xM * xA, dtype=torch.complex64, device="cuda")
    out2, obuf2 = padded_blocks(F, S, m, torch.complex64)
    res = core.wave_split_subgrids(torch.from_numpy(sub).cuda(), [s[0] for s in s_offs], [s[1] for s in s_offs], f0, f1,
                                   work, out2)
    assert res is out2 and res.dtype == torch.complex64 and tuple(res.shape) == (F, S, m, m)
    assert blocks_padding_intact(obuf2, S, m * m)
    _check("wave_split_subgrids", pair, "c64", out2.cpu().numpy().transpose(1, 0, 2, 3), want, 2e-6)


# ------------------------------------------------------------------------------------------- (e) limits at (7, 8)
def _side_case(pair, dtype, f_offs, s_offs, xA, seed):
    core, _ = cores(pair)
    prob = problem(pair, dtype, f_offs=f_offs, s_offs=s_offs, xA=xA, seed=seed)
    G = run_transform(core, prob, dtype)
    res, tmp = _run_side(core, G, prob, dtype)
    return prob, tmp.cpu().numpy(), res.cpu().numpy()


@pytest.mark.parametrize("dtype", ["c64", "c128"])
@pytest.mark.parametrize("nfacets", [1, 64])
def test_facet_count_limits(nfacets, dtype):
    """1 facet, and kSumFinishMaxFacets = 64 facets as an 8 x 8 grid of offsets (8 groups of 8); 65 facets raise"""
    import torch

    pair = (7, 8)
    core, _ = cores(pair)
    fstep, xM, m = core.facet_off_step, core.xM_size, core.xM_yN_size
    grid = [-(xM // 5), -(xM // 11), 0, xM // 9, xM // 4 + 1, xM // 2 - 2, 5 * (xM // 8), xM - 3]
    f_offs = [(a * fstep, b * fstep) for a in grid for b in grid]
    if nfacets == 1:
        f_offs = [(-(xM // 5) * fstep, (xM // 2 + 1) * fstep)]
    _, s_offs = offsets(pair)
    prob, tmp, res = _side_case(pair, dtype, f_offs, s_offs[1:], 191, seed=nfacets)
    # (the sum of 64 blocks: eight times the magnitude of one, the relative bounds stay as they are)
    _check(f"{nfacets} facet(s) axis 1", pair, dtype, tmp, prob["want1"], 3e-6)
    _check(f"{nfacets} facet(s) side", pair, dtype, res, prob["want"], SIDE_TOL)
    if nfacets == 64:
        tdtype = _tdtype(dtype)
        G = torch.zeros((65, 1, m, m), dtype=tdtype, device="cuda")
        out = torch.empty((1, xM, 191), dtype=tdtype, device="cuda")
        with pytest.raises(NotImplementedError):
            core.sum_finish_facets(G, [0] * 65, [0] * 65, out, [0], 191)
        if dtype == "c64":
            with pytest.raises(NotImplementedError):
                core.split_prepare_facets(out, [0], [0] * 65, [0] * 65, G)


@pytest.mark.parametrize("dtype", ["c64", "c128"])
def test_sixty_five_subgrids_in_one_call(dtype):
    """65 subgrids cross kSumFinishMaxBatch = 64: the second launch starts at subgrid 64 of the blocks, the output and the
    masks.  Every subgrid has its own offsets, mask and data (subgrids 63, 64 and 65 -- the last of the first launch, the
    only one of the second -- among them), so a wrong batch offset shows."""
    pair = (7, 8)
    core, _ = cores(pair)
    sstep, yN = core.subgrid_off_step, core.yN_size
    s_offs = [(((7 * b) % yN - yN // 2) * sstep, ((11 * b + 3) % yN - yN // 3) * sstep) for b in range(65)]
    assert len(set(s_offs[62:])) == 3 and len({s[1] for s in s_offs}) == 65
    f_offs, _ = offsets(pair)
    prob, tmp, res = _side_case(pair, dtype, f_offs[1:4], s_offs, 191, seed=65)
    assert len({prob["mask1"][b].tobytes() for b in (62, 63, 64)}) == 3
    _check("65 subgrids axis 1", pair, dtype, tmp, prob["want1"], 3e-6)
    _check("65 subgrids side", pair, dtype, res, prob["want"], SIDE_TOL)


@pytest.mark.parametrize("dtype", ["c64", "c128"])
def test_uncropped_subgrid(dtype):
    """``subgrid_size = xM``: nothing is cropped"""
    pair = (7, 8)
    core, _ = cores(pair)
    f_offs, s_offs = offsets(pair)
    prob, tmp, res = _side_case(pair, dtype, f_offs, s_offs, core.xM_size, seed=3)
    _check("xA = xM axis 1", pair, dtype, tmp, prob["want1"], 3e-6)
    _check("xA = xM side", pair, dtype, res, prob["want"], SIDE_TOL)


# ------------------------------------------------------------------------------- (f) complex128 column passes (K2)
K2_LENGTHS = [128, 256, 512, 1024, 2048, 4096, 8192, 32768]  # (16384: test_prepare_facet_columns_c128)


def k2_problem(yN):
    """``(core parameters, band rows [F, yB0, yN], facet off0s, subgrid off1)`` of the column-pass sweep: pair (7, 8)
    with ``N = 2 yN``; 2 facets, one negative off0, 96 band rows"""
    N, xM = 2 * yN, 256
    rng = numpy.random.default_rng(600 + yN)
    fstep = N // xM
    # (facet offsets are multiples of N / xM; in units of the padded axis they move the rows by off0 * yN / N)
    return dict(N=N, xM=xM, yN=yN), _crandn(rng, (2, 96, yN), "c128"), [0, -24 * fstep], -5 * (N // yN) * max(1, yN // 37)


def k2_run(yN, use_rowmap):
    import torch

    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    p, logical, off0s, off1 = k2_problem(yN)
    core = SwiftlyCoreHip(W, p["N"], p["xM"], p["yN"])
    sstep = core.subgrid_off_step
    rowmap, n_rows = core.subgrid_column_rows([0, (yN // 3) * sstep]) if use_rowmap else (None, yN)
    got = core.prepare_facet_columns(torch.from_numpy(logical).cuda(), off0s, (0, yN), off1, rowmap, n_rows)
    assert got.dtype == torch.complex128 and tuple(got.shape) == (2, n_rows, core.xM_yN_size)
    rm = rowmap.cpu().numpy() if rowmap is not None else numpy.arange(yN)
    return got.cpu().numpy(), rm


@pytest.mark.parametrize("use_rowmap", [False, True], ids=["all-rows", "rowmap"])
@pytest.mark.parametrize("yN", K2_LENGTHS)
def test_prepare_facet_columns_c128_lengths(yN, use_rowmap):
    """K2 in complex128 at every length class: one column pass (128, 256, 512 points) and the four-step splits
    5+5, 5+6, 6+6, 6+7 and 7+8 (1024 .. 8192 and 32768 points; 16384 = 7+7 is covered next to the pipeline tests)"""
    p, logical, off0s, off1 = k2_problem(yN)
    ref = orc.OracleCore(W, p["N"], p["xM"], p["yN"])
    m, yB0 = ref.xM_yN_size, logical.shape[1]
    assert m == 128
    got, rm = k2_run(yN, use_rowmap)
    keep = rm >= 0
    assert 0 < keep.sum() and (use_rowmap == bool(keep.sum() < yN) or yN == m)  # (m = yN: every row is read)
    worst = 0.0
    for f in range(2):
        win = ref.extract_from_facet(logical[f], off1, axis=1)  # [yB0, m]
        want = ref.prepare_facet(win / ref.facet_window(yB0)[:, None], off0s[f], axis=0)  # window NOT applied
        err = maxrel(got[f][rm[keep]], want[keep])
        worst = max(worst, err)
        assert err <= C128_TOL, (yN, use_rowmap, f, err)
    print(f"SWEEP K2 complex128 yN={yN:<6d} {'rowmap' if use_rowmap else 'all rows'}: {worst:.3e} (bound {C128_TOL:.2e})")


_K2_CHILD = r"""
import sys, numpy
sys.path[:0] = [sys.argv[2] + "/tests", sys.argv[2], sys.argv[3]]
import test_hip_instance_sweep_gpu as t
for yN in (8192, 32768):
    for use_rowmap in (False, True):
        got, _ = t.k2_run(yN, use_rowmap)
        numpy.save(f"{sys.argv[1]}_{yN}_{int(use_rowmap)}.npy", got)
"""


def test_prepare_facet_columns_c128_chunked_bit_identical(tmp_path):
    """the chunked two-stream four-step (SWIFTLY_K2_CHUNK, read once per process: one fresh child process per setting) gives
    the same bits as the plain one at 8192 and 32768 points"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "ska-sdp-distributed-fourier-transform_amd")
    stems = []
    for chunk in ("0", "64,1"):
        stem = str(tmp_path / f"chunk_{chunk.replace(',', '_')}")
        env = dict(os.environ, SWIFTLY_K2_CHUNK=chunk)
        res = subprocess.run([sys.executable, "-c", _K2_CHILD, stem, root, pkg], env=env, cwd=root, timeout=600,
                             capture_output=True, text=True, check=False)
        assert res.returncode == 0, (chunk, res.returncode, res.stderr[-3000:])
        stems.append(stem)
    for yN in (8192, 32768):
        for use_rowmap in (0, 1):
            a, b = (numpy.load(f"{stem}_{yN}_{use_rowmap}.npy") for stem in stems)
            assert a.dtype == numpy.complex128 and a.shape == b.shape and a.shape[0] == 2
            assert numpy.array_equal(a, b), (yN, use_rowmap)


K2_C64_CHUNK_LENGTHS = [11, 13]  # log2 yN: the four-step splits 5+6 and 6+7


def k2_c64_problem(L):
    """``(core, oracle core, band rows [2, 96, yN], facet off0s, subgrid off1, row map, rows kept)`` of the complex64 chunk
    test: the K2 case of the facet sweep at ``yN = 2^L`` (m = 128, 2 facets, its seed) with the negative ``off1``"""
    import test_hip_facet_sweep_gpu as fs

    core, ref = fs.cores(fs.params(L))
    logical = fs.crandn(numpy.random.default_rng(600 + L), (2, 96, core.yN_size))
    off0s, off1s, map_offs = fs.k2_offsets(core)
    rowmap, n_kept = core.subgrid_column_rows(map_offs)
    return core, ref, logical, off0s, off1s[1], rowmap, n_kept


_K2_C64_CHILD = r"""
import sys, numpy, torch
sys.path[:0] = [sys.argv[2] + "/tests", sys.argv[2], sys.argv[3]]
import test_hip_facet_sweep_gpu as fs
import test_hip_instance_sweep_gpu as t
for L in t.K2_C64_CHUNK_LENGTHS:
    core, _, logical, off0s, off1, rowmap, n_kept = t.k2_c64_problem(L)
    dev = torch.from_numpy(logical).cuda()
    for bits in (32, 64):
        with fs.precision(core, bits):
            for use_rowmap in (False, True):
                got = fs.k2_run(core, dev, off0s, (0, core.yN_size), off1, rowmap if use_rowmap else None,
                                n_kept if use_rowmap else core.yN_size)
                numpy.save(f"{sys.argv[1]}_{L}_{bits}_{int(use_rowmap)}.npy", got)
"""


def test_prepare_facet_columns_c64_chunked_bit_identical(tmp_path):
    """the chunked two-stream four-step of COMPLEX64 K2 (which otherwise runs at the benchmark's size only) gives the same
    bits as the plain one at 2048 (5+6) and 8192 (6+7) points, m = 128, 2 facets, with and without a row map, in float32
    and in float64 arithmetic: ``SWIFTLY_K2_CHUNK=64,1`` makes four chunks (2 items x 2 x 64 columns) that alternate between
    the two streams; one fresh child process per setting (the variable is read once per process).  The plain result also
    meets the facet sweep's bound for its length and arithmetic against the oracle: identical means identically right."""
    import test_hip_facet_sweep_gpu as fs

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "ska-sdp-distributed-fourier-transform_amd")
    stems = []
    for chunk in ("0", "64,1"):
        stem = str(tmp_path / f"chunk_{chunk.replace(',', '_')}")
        env = dict(os.environ, SWIFTLY_K2_CHUNK=chunk)
        res = subprocess.run([sys.executable, "-c", _K2_C64_CHILD, stem, root, pkg], env=env, cwd=root, timeout=600,
                             capture_output=True, text=True, check=False)
        assert res.returncode == 0, (chunk, res.returncode, res.stderr[-3000:])
        stems.append(stem)
    for L in K2_C64_CHUNK_LENGTHS:
        core, ref, logical, off0s, off1, rowmap, n_kept = k2_c64_problem(L)
        yN, rm = core.yN_size, rowmap.cpu().numpy()
        assert core.xM_yN_size == 128 and 0 < n_kept < yN
        want = [fs.k2_want(ref, logical[f], off0s[f], off1) for f in range(2)]
        for bits in (32, 64):
            for use_rowmap in (0, 1):
                plain, chunked = (numpy.load(f"{stem}_{L}_{bits}_{use_rowmap}.npy") for stem in stems)
                assert plain.dtype == numpy.complex64 and plain.shape == chunked.shape == (2, n_kept if use_rowmap else yN, 128)
                assert numpy.array_equal(plain, chunked), (L, bits, use_rowmap)
                keep = rm >= 0 if use_rowmap else numpy.ones(yN, dtype=bool)
                idx = rm[keep] if use_rowmap else numpy.arange(yN)
                fs.check("K2 complex64, chunks off", L, bits, plain[:, idx], numpy.stack([w[keep] for w in want]), 1,
                         fs.k2_has_f64(L), note=f"rowmap {use_rowmap}")


# ------------------------------------------------------------------------------------------- (g) tables stay in step
def _cell_params(logm, logx):
    """a valid parameter set with ``m = 2^logm`` and ``xM = 2^logx`` (``m < xM``: ``N = 2 xM``, ``yN = 2 m``), else None"""
    if logm >= logx:
        return None  # m = xM * yN / N with yN < N
    return dict(N=2 << logx, xM=1 << logx, yN=2 << logm)


def library_pairs(feature, dtype):
    """(log2 m, log2 xM) in 0..17 x 0..17 that the built library's capability table (``swiftly_hip_supports``) has
    ``feature`` for, without a GPU; the padded facet of ``2^max(10, log2 m)`` points is in range for every pipeline"""
    from ska_sdp_exec_swiftly_amd import _lib

    lib, found = _lib.load(), set()
    for logm in range(18):
        for logx in range(18):
            xM, yN = 1 << logx, 1 << max(10, logm)
            if lib.swiftly_hip_supports(feature, dtype, (xM * yN) >> logm, yN, xM, 0):
                found.add((logm, logx))
    return found


def test_python_and_native_tables_agree():
    """one core per cell of log2 m in 6..10 by log2 xM in 7..12: the Python-side gates, this module's tables and the
    entry point itself name the same instances"""
    import torch

    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip, _lib

    assert set(PAIRS_C128) == library_pairs(_lib.FEATURE_BAND_PIPELINE_EXPLICIT, _lib.C128)
    cells = 0
    for logm in range(6, 11):
        for logx in range(7, 13):
            p = _cell_params(logm, logx)
            if p is None:
                continue
            cells += 1
            core = SwiftlyCoreHip(W, p["N"], p["xM"], p["yN"])
            m, xM, xA = core.xM_yN_size, core.xM_size, 33
            assert (m, xM) == (1 << logm, 1 << logx)
            assert core.supports_fused_subgrid(torch.complex64) == ((logm, logx) in PAIRS), (logm, logx)
            assert core.supports_band_pipeline(torch.complex128, explicit=True) == ((logm, logx) in PAIRS_C128), (logm, logx)
            for tdtype, table in ((torch.complex64, PAIRS), (torch.complex128, PAIRS_C128)):
                G = torch.zeros((1, 1, m, m), dtype=tdtype, device="cuda")
                G[0, 0, 0, 0] = 1.0
                out = torch.zeros((1, xM, xA), dtype=tdtype, device="cuda")
                if (logm, logx) in table:
                    res = core.sum_finish_facets(G, [0], [0], out, [0], xA)
                    assert res.dtype == tdtype and tuple(res.shape) == (1, xM, xA)
                    assert float(out.abs().max()) > 0.0 and bool(torch.isfinite(out.abs()).all()), (logm, logx, tdtype)
                else:
                    with pytest.raises(NotImplementedError):
                        core.sum_finish_facets(G, [0], [0], out, [0], xA)
            del core
    assert cells == 20  # every cell with m < xM
