"""
Every length class of the facet-side kernels against the 1-D oracle.

The facet side picks its code at run time from the padded facet size ``yN = 2^L``, the contribution size ``m`` and the
column precision: the column passes (``col_transform``, csrc/swiftly_abi.hip) run one pass up to 1024 points (512 with the
gather-sum load of the backward pass) and a four-step ``l1 = L / 2``, ``l2 = L - l1`` above, every pass length with its own
tile geometry (``CGeoFor``, csrc/swiftly_colpass.h) in float32 and in float64 arithmetic; the contiguous-axis kernels have
the generic rows up to 8192 points, ``BandGeo16k``, the 32768-point pair kernels with their ``NSEG`` instances and the
65536-point kernel with ``NSEG = 44``; K2 and ``accumulate_facet_columns`` loop over launch groups of facets and waves.  This
module runs each of them through the C ABI entry points, one by one, at every ``L`` the capability table
(``swiftly_hip_supports``, csrc/swiftly_caps.h) accepts, and compares ALL output elements with a composition of the
complex128 primitives of oracle/swiftly_oracle.py -- composed as test_prepare_facet_columns, test_prepare_facet_band,
test_finish_axis1_rows_matches_oracle (test_hip_band_pipeline_gpu.py), test_accumulate_facet_columns_long_columns and
test_finish_facet_band_long_rows (test_hip_backward_parity_gpu.py) do.  No expected value comes from another HIP path.

Cores: ``k2_problem`` of the instance sweep extended to every length -- W = 11, ``yN = 2^L``, ``N = 2 yN``, ``xM = 256``,
so ``m = 128``, for L = 7 .. 16, and ``(N, xM, yN) = (128, 128, 64)`` with ``m = 64`` for L = 6.  At L = 6 and 7, ``m = yN``:
every band column lies in every window, so "an untouched band column exists" can be asked only from L = 8 on.  Inputs are
seeded complex Gaussian noise in complex64.

Bounds (none tuned against the kernels)
* float32 arithmetic: relative RMSE over the whole output below ``2e-6 * sqrt(min(L, 15) / 15)`` -- the project's 2e-6 for
  one long transform of 15 or more stages, scaled by the square-root-of-stages rule of the instance sweep -- and
  ``max|err| <= 2e-5 * max|want|`` for every transformed vector (every output row of K1 / finish_facet_band /
  finish_axis1_rows, every column of K2 / accumulate_facet_columns).  finish_axis1_rows is an m-point transform: its stage
  count is ``log2 m``.
* ``column_precision = 64``: the only float32 steps left are the complex64 stores, so the bound is ``3 * floor`` with
  ``floor = relrms(want.astype(complex64), want)`` from the oracle alone (a four-step rounds twice: ``sqrt(2) * floor``),
  and the float64 result must have a smaller error than the float32 result of the same case.  Lengths without float64
  instances keep the float32 bound: K2 at 1024 points (single pass; float64 passes end at 512) and the gather-sum load of
  accumulate_facet_columns at 512 points (single pass; float64 gather-sum passes end at 256).  L = 6 has float64 instances
  in both.
* padding and sentinel regions compare exactly equal; masked pixels and untouched band columns are exactly zero.

Measured on an MI355X: the worst relative RMSE over the cases of one length (every case prints a ``FACETSWEEP`` line with
its figure, bound and per-vector peak; "=" marks a length without float64 instances, where both precisions run float32).
K2 = prepare_facet_columns, acc = accumulate_facet_columns, K1 = prepare_facet_band, fin = finish_facet_band (L = 6: the
gate test); float32 bounds 1.3e-06 (L = 6) .. 2.0e-06 (L >= 15), float64 bound 7.5e-08 .. 7.7e-08 (3 * floor):

   L   K2 f32   K2 f64  acc f32  acc f64   K1 f32  fin f32
   6  8.3e-08  2.5e-08  1.2e-07  4.3e-08        -  8.9e-08
   7  9.3e-08  2.5e-08  1.1e-07  4.1e-08  1.4e-07  1.1e-07
   8  1.0e-07  2.5e-08  1.2e-07  3.6e-08  1.3e-07  1.2e-07
   9  1.1e-07  2.6e-08  1.3e-07        =  1.3e-07  1.2e-07
  10  1.2e-07        =  1.2e-07  4.4e-08  1.4e-07  1.3e-07
  11  1.1e-07  3.6e-08  1.2e-07  4.4e-08  1.4e-07  1.4e-07
  12  1.2e-07  3.6e-08  1.3e-07  4.6e-08  1.5e-07  1.5e-07
  13  1.2e-07  3.6e-08  1.3e-07  4.5e-08  1.5e-07  1.4e-07
  14  1.2e-07  3.6e-08  1.3e-07  4.5e-08  1.8e-07  1.6e-07
  15  1.3e-07  3.6e-08  1.4e-07  4.5e-08  2.0e-07  1.9e-07
  16  1.4e-07  3.6e-08  1.4e-07  4.5e-08  1.9e-07  1.8e-07

Worst per-vector peak (bound 2e-05): K2 1.1e-06 (L = 16, float32), acc 4.2e-07, K1 3.4e-07, fin 3.1e-07.  Launch groups
at L = 8, float32 / float64: K2 with 33 facets, 65 waves and the one-facet workspace 1.0e-07 / 2.5e-08 each (L = 11:
1.1e-07 / 3.6e-08); accumulate with 33 facets and the one-facet workspace within the L = 8 figures above.
finish_axis1_rows: 1.3e-07 at worst over m = 128 .. 1024 at 16384 points, 1.0e-07 at 65536 (bound 1.4e-06 .. 1.6e-06).

Module wall time on an MI355X: 19 s for the 56 cases (pytest's own figure); the slowest case, K2 at L = 16, takes 4.9 s.
"""
import numpy
import pytest

from oracle import swiftly_oracle as orc

pytestmark = pytest.mark.gpu

W = 11.0
#: log2 yN of the column-pass sweeps (K2, accumulate_facet_columns): what BACKWARD_BAND accepts (tests/test_instance_tables_cpu.py)
LENGTHS = list(range(6, 17))
#: log2 yN of the contiguous-axis sweeps (K1, finish_facet_band): what BAND_PIPELINE accepts with m = 128, xM = 256
K1_LENGTHS = list(range(7, 17))
#: log2 yN with the parity-split band layout (SPLIT_BAND)
SPLIT_LENGTHS = [14, 15, 16]
#: (log2 m, log2 xM, log2 yN) of the finish_axis1_rows sweep: one instance per m (csrc/sum_finish.hip, launch_axis1_rows)
AXIS1_CASES = [(7, 10, 14), (8, 10, 14), (9, 10, 14), (10, 11, 14), (7, 8, 16)]
SENTINEL = complex(7.5, -3.25)


def params(L):
    """the sweep's core for ``yN = 2^L``"""
    if L == 6:
        return dict(N=128, xM=128, yN=64)
    return dict(N=2 << L, xM=256, yN=1 << L)


def k2_has_f64(L):
    """float64 instances of the plain column transform (col_transform): single passes of 2^5 .. 2^9 points; four-steps whose
    two lengths lie in that range (2^11 = 5 + 6 .. 2^16 = 8 + 8); the 1024-point single pass has none"""
    return L != 10


def acc_has_f64(L):
    """... of the gather-sum transform: single pass up to 2^9 points with float64 up to 2^8; 2^10 = 5 + 5 is a four-step"""
    return L != 9


def f32_bound(stages):
    return 2e-6 * float(numpy.sqrt(min(stages, 15) / 15.0))


def relrms(got, want):
    return float(numpy.sqrt(numpy.mean(numpy.abs(got - want) ** 2) / numpy.mean(numpy.abs(want) ** 2)))


def vector_peak(got, want, axis):
    """largest ``max|err| / max|want|`` over the transformed vectors (``axis`` = the transform axis); a vector that must be
    zero must be exactly zero"""
    err = numpy.abs(got - want).max(axis=axis)
    ref = numpy.abs(want).max(axis=axis)
    assert not err[ref == 0].any(), "a vector that must be zero is not"
    return float((err[ref > 0] / ref[ref > 0]).max())


def _record(what, L, bits, value, bound, note="", label=None):
    print(f"{label or f'FACETSWEEP {what:<26s} L={L:<3d}'} f{bits:<3d} {value:.3e} (bound {bound:.2e}) {note}")


def check(what, L, bits, got, want, axis, f64=False, stages=None, note="", label=None):
    """all elements of ``got`` against ``want``; returns the relative RMSE.  ``label``: the head of the record line of
    another sweep (tests/test_hip_mixed_sweep_gpu.py), whose ``L`` is the stage count of its bound"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert got.dtype == numpy.complex64, (what, got.dtype)
    assert numpy.isfinite(got).all(), what  # (``got`` may be a gathered, non-contiguous selection)
    err = relrms(got, want)
    if bits == 64 and f64:
        bound = 3.0 * relrms(want.astype(numpy.complex64), want)
    else:
        bound = f32_bound(L if stages is None else stages)
    peak = vector_peak(got, want, axis)
    _record(what, L, bits, err, bound, f"peak {peak:.2e} {note}", label)
    assert err < bound, (what, L, bits, note, err, bound)
    assert peak <= 2e-5, (what, L, bits, note, peak)
    return err


def crandn(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(numpy.complex64)


def band_cols(yN, band):
    """physical column of every logical (centred) column, -1 outside the band (parity-split layout; band_cols of
    test_hip_band_pipeline_gpu.py)"""
    start, length = band
    half = ((length + 1) // 2 + 15) // 16 * 16  # swiftly_hip_band_columns(length) / 2
    d = (numpy.arange(yN) - start) % yN
    return numpy.where(d < length, (d & 1) * half + (d >> 1), -1)


_CORES = {}


def cores(p):
    """``(SwiftlyCoreHip, OracleCore)``, built once per parameter set (the window function costs 0.5 s at 16384 points
    and 2.2 s at 65536, twice)"""
    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    key = (p["N"], p["xM"], p["yN"])
    if key not in _CORES:
        _CORES[key] = (SwiftlyCoreHip(W, p["N"], p["xM"], p["yN"]), orc.OracleCore(W, p["N"], p["xM"], p["yN"]))
    return _CORES[key]


class precision:
    """``with precision(core, bits):`` -- the column precision of a shared core, put back to 32 afterwards"""

    def __init__(self, core, bits):
        self.core, self.bits = core, bits

    def __enter__(self):
        self.core.column_precision = self.bits
        assert self.core.column_precision == self.bits

    def __exit__(self, *exc):
        self.core.column_precision = 32


def is_split(core):
    return core.band_columns((0, 2)) != 2  # (parity-split: two halves of a multiple of 16 columns)


def pack_bands(core, logical, band):
    """``logical[..., yN]`` in the band layout of the core: parity-split band buffers, or the whole axis in plain order"""
    yN = core.yN_size
    if not is_split(core):
        assert tuple(band) == (0, yN)
        return numpy.ascontiguousarray(logical)
    pc = band_cols(yN, band)
    packed = numpy.zeros(logical.shape[:-1] + (core.band_columns(band),), dtype=logical.dtype)
    packed[..., pc[pc >= 0]] = logical[..., pc >= 0]
    return packed


# ------------------------------------------------------------------------------------ (a) K2, prepare_facet_columns
def k2_want(ref, logical_f, off0, off1):
    """window gather + strided-axis prepare_facet WITHOUT its window (applied by K1), as test_prepare_facet_columns"""
    yB0 = logical_f.shape[0]
    win = ref.extract_from_facet(logical_f, off1, axis=1).astype(complex)  # [yB0, m]
    return ref.prepare_facet(win / ref.facet_window(yB0)[:, None], off0, axis=0)  # [yN, m]


def k2_run(core, bands, off0s, band, off1, rowmap, n_rows):
    """one K2 call into a sentinel-padded output; returns ``got[F, n_rows, m]``"""
    import torch

    F, m = bands.shape[0], core.xM_yN_size
    obuf = torch.full((F, n_rows + 1, m + 8), SENTINEL, dtype=torch.complex64, device="cuda")
    out = obuf[:, :n_rows, :m]
    res = core.prepare_facet_columns(bands, off0s, band, off1, rowmap, n_rows, out=out)
    assert res is out and res.dtype == torch.complex64
    assert bool((obuf[:, n_rows] == SENTINEL).all()) and bool((obuf[:, :, m:] == SENTINEL).all()), \
        "prepare_facet_columns wrote outside its rows"
    return out.cpu().numpy()


def k2_offsets(core):
    """two facet off0 (one negative), two subgrid off1 (one negative), the off0 of the row map"""
    yN = core.yN_size
    fstep, sstep = core.facet_off_step, core.subgrid_off_step
    return [3 * fstep, -24 * fstep], [3 * max(1, yN // 41) * sstep, -5 * max(1, yN // 37) * sstep], [0, (yN // 3) * sstep]


@pytest.mark.parametrize("L", LENGTHS)
def test_prepare_facet_columns_lengths(L):
    """K2 in complex64 at every length class, float32 and float64 arithmetic: single passes of 64 .. 1024 points and the
    four-steps 5+6, 6+6, 6+7, 7+7, 7+8 and 8+8; 2 facets (one negative off0), with and without the row map, two off1 (one
    negative); split sizes: the full band and a partial one.  No float64 instance at 1024 points (float32 bound there)."""
    import torch

    core, ref = cores(params(L))
    yN, m = core.yN_size, core.xM_yN_size
    rows = 40 if L == 6 else 96
    logical = crandn(numpy.random.default_rng(600 + L), (2, rows, yN))
    off0s, off1s, map_offs = k2_offsets(core)
    assert off0s[1] < 0 < off0s[0] and off1s[1] < 0 < off1s[0]
    rowmap, n_kept = core.subgrid_column_rows(map_offs)
    rm = rowmap.cpu().numpy()
    assert (n_kept < yN) == (m < yN)
    bands = [(0, yN)]
    if L in SPLIT_LENGTHS:
        bands.append(core.band_for_offsets(off1s))
        assert bands[1][1] < yN and is_split(core)
    else:
        assert not is_split(core) and core.band_for_offsets(off1s) == (0, yN)
    want = {(i, f): k2_want(ref, logical[f], off0s[f], off1s[i]) for i in range(2) for f in range(2)}
    # full band: both off1 with and without the row map; partial band: one of each
    runs = [(0, i, r) for i in range(2) for r in (False, True)] + ([(1, 0, True), (1, 1, False)] if len(bands) > 1 else [])
    errs = {}
    for bits in (32, 64):
        with precision(core, bits):
            for b, band in enumerate(bands):
                dev = torch.from_numpy(pack_bands(core, logical, band)).cuda()
                for bb, i, use_rowmap in runs:
                    if bb != b:
                        continue
                    got = k2_run(core, dev, off0s, band, off1s[i], rowmap if use_rowmap else None, n_kept if use_rowmap else yN)
                    keep = rm >= 0 if use_rowmap else numpy.ones(yN, dtype=bool)
                    idx = rm[keep] if use_rowmap else numpy.arange(yN)
                    w = numpy.stack([want[(i, f)][keep] for f in range(2)])
                    errs[(bits, b, i, use_rowmap)] = check("prepare_facet_columns", L, bits, got[:, idx], w, 1, k2_has_f64(L),
                                                           note=f"band {b} off1 {i} rowmap {int(use_rowmap)}")
    if k2_has_f64(L):
        for key, e32 in errs.items():
            if key[0] == 32:
                assert errs[(64,) + key[1:]] < e32, (L, key, errs[(64,) + key[1:]], e32)


def _k2_group_problem(F, n_waves, seed):
    """L = 8 (256 points, one pass): every facet and every wave with its own offset and data"""
    core, ref = cores(params(8))
    yN = core.yN_size
    fstep, sstep = core.facet_off_step, core.subgrid_off_step
    logical = crandn(numpy.random.default_rng(seed), (F, 96, yN))
    off0s = [((7 * f) % 61 - 30) * fstep for f in range(F)]
    off1s = [((5 * w + 3) % yN - yN // 2) * sstep for w in range(n_waves)]
    assert len(set(off0s)) == F and len(set(off1s)) == n_waves
    return core, ref, logical, off0s, off1s


def test_prepare_facet_columns_thirty_three_facets():
    """33 facets in one call cross kColZF = 32: the second launch group starts at facet 32 of the band buffers, the offsets
    and the output"""
    import torch

    core, ref, logical, off0s, off1s = _k2_group_problem(33, 1, 833)
    yN = core.yN_size
    dev = torch.from_numpy(logical).cuda()
    want = numpy.stack([k2_want(ref, logical[f], off0s[f], off1s[0]) for f in range(33)])
    for bits in (32, 64):
        with precision(core, bits):
            got = k2_run(core, dev, off0s, (0, yN), off1s[0], None, yN)
        check("K2 33 facets", 8, bits, got, want, 1, True)
        for f in (31, 32):  # the last facet of the first group, the only one of the second
            check(f"K2 33 facets, facet {f}", 8, bits, got[f], want[f], 0, True)


def _k2_waves(core, dev, off0s, off1s, workspace):
    import torch

    F, nw, yN, m = dev.shape[0], len(off1s), core.yN_size, core.xM_yN_size
    obuf = torch.full((F, nw + 1, yN, m), SENTINEL, dtype=torch.complex64, device="cuda")
    out = obuf[:, :nw]
    res = core.prepare_facet_columns_waves(dev, off0s, (0, yN), off1s, out, workspace=workspace)
    assert res is out
    assert bool((obuf[:, nw] == SENTINEL).all()), "prepare_facet_columns_waves wrote outside its waves"
    return out.cpu().numpy()


def test_prepare_facet_columns_sixty_five_waves():
    """65 waves through prepare_facet_columns_waves cross kColZB = 64: the second launch group starts at wave 64 of the
    offsets and the output"""
    import torch

    core, ref, logical, off0s, off1s = _k2_group_problem(2, 65, 865)
    dev = torch.from_numpy(logical).cuda()
    want = numpy.stack([numpy.stack([k2_want(ref, logical[f], off0s[f], o) for o in off1s]) for f in range(2)])
    for bits in (32, 64):
        with precision(core, bits):
            got = _k2_waves(core, dev, off0s, off1s, None)
        check("K2 65 waves", 8, bits, got, want, 2, True)
        for w in (63, 64):
            check(f"K2 65 waves, wave {w}", 8, bits, got[:, w], want[:, w], 1, True)


@pytest.mark.parametrize("L", [8, 11])
def test_prepare_facet_columns_workspace_of_one_facet(L):
    """a workspace that holds the four-step scratch of exactly ONE facet and wave (2 facets, 3 waves): every wave becomes a
    launch group of its own (w0 advances by one).  256 points (one pass) and 2048 points (a four-step, whose scratch of two
    facets no longer fits the workspace)."""
    import torch

    core, ref = cores(params(L))
    yN, m = core.yN_size, core.xM_yN_size
    fstep, sstep = core.facet_off_step, core.subgrid_off_step
    logical = crandn(numpy.random.default_rng(880 + L), (2, 96, yN))
    off0s = [5 * fstep, -17 * fstep]
    off1s = [(yN // 9) * sstep, -(yN // 5) * sstep, (yN // 2 + 3) * sstep]
    dev = torch.from_numpy(logical).cuda()
    work = torch.empty((yN * m * 8,), dtype=torch.uint8, device="cuda")
    want = numpy.stack([numpy.stack([k2_want(ref, logical[f], off0s[f], o) for o in off1s]) for f in range(2)])
    for bits in (32, 64):
        with precision(core, bits):
            got = _k2_waves(core, dev, off0s, off1s, work)
        check("K2 one-facet workspace", L, bits, got, want, 2, True)


# ------------------------------------------------------------------------------------ (b) accumulate_facet_columns
def facet_size(L, odd=False, yN=None):
    """a facet size near 0.69 yN (0.6875 yN: even, and a whole number of load segments of the long-row kernels);
    ``yN`` = ``2^L`` unless given"""
    yB = 11 * ((1 << L) if yN is None else yN) // 16
    return yB + 1 if odd else yB


_ACC = {}


def acc_problem(L, F=2, n_waves=2, seed=0):
    """inputs and oracle result of the gather-sum sweep, cached per case: ``n_waves`` waves whose band columns overlap,
    three / two subgrids per wave with overlapping row windows, ``F`` facets with float masks, every facet its own offset.

    ``want[F, yB, columns]`` holds every touched band column (``cols``: their logical column numbers)."""
    key = (L, F, n_waves, seed)
    if key not in _ACC:
        _ACC[key] = acc_problem_at(params(L), facet_size(L, odd=(L == 9)), numpy.random.default_rng(3200 + 16 * L + seed),
                                   L >= 10, F, n_waves)
    return _ACC[key]


def acc_problem_at(p, yB, rng, pruned_band, F=2, n_waves=2):
    """:py:func:`acc_problem` for the parameter set ``p`` (N, xM, yN) and facet size ``yB`` (not cached); ``pruned_band``:
    the smallest band that holds the windows, else the whole axis"""
    from ska_sdp_exec_swiftly_amd.core_hip import band_range

    core, ref = cores(p)
    N, yN, m = core.N, core.yN_size, core.xM_yN_size
    fstep, sstep = core.facet_off_step, core.subgrid_off_step
    facet_off0s = [5 * fstep, -24 * fstep] if F == 2 else [((7 * f) % 61 - 30) * fstep for f in range(F)]
    assert len(set(facet_off0s)) == F
    masks = (rng.random((F, yB)) > 0.1).astype(numpy.float32)
    # adjacent windows share m / 4 band columns; a third offset widens the band so that untouched columns exist
    s1 = [yN // 8, yN // 8 + m - m // 4][:n_waves]
    s0 = [[-m, -(m // 4), m // 2], [m // 8, m // 8 + m // 2]][:n_waves]
    waves = [(a * sstep, [b * sstep for b in bs]) for a, bs in zip(s1, s0)]
    band = band_range(N, yN, m, [w[0] for w in waves] + [(s1[-1] + m + m // 2) * sstep]) if pruned_band else (0, yN)
    cols = sorted({int(c) for a in s1 for c in (yN // 2 - m // 2 + numpy.arange(m) + a) % yN})
    pos = numpy.full(yN, -1)
    pos[cols] = numpy.arange(len(cols))
    want = numpy.zeros((F, yB, len(cols)), dtype=complex)
    parts = []
    i = numpy.arange(m)
    for (off1, off0s), a in zip(waves, s1):
        pw = crandn(rng, (F, len(off0s), m, m))
        parts.append(pw)
        big = (yN // 2 - m // 2 + i + a) % yN  # add_to_facet along axis 1: window index i holds contribution column (i + s1) mod m
        for f in range(F):
            acc = numpy.zeros((yN, m), dtype=complex)
            for b, o0 in enumerate(off0s):
                acc = ref.add_to_facet(pw[f, b].astype(complex), o0, axis=0, out=acc)
            fin = ref.finish_facet(acc, facet_off0s[f], yB, axis=0) * masks[f][:, None]
            want[f][:, pos[big]] += fin[:, (i + a) % m]
    return dict(yB=yB, facet_off0s=facet_off0s, masks=masks, waves=waves, band=band, cols=numpy.array(cols), want=want,
                parts=parts)


def acc_run(L, bits, prob, workspace_facets=None):
    """the waves of ``prob`` through accumulate_facet_columns + band_zero_untouched from NaN-filled accumulators; checks
    the touched flags, the untouched columns and every touched column; returns the relative RMSE"""
    import torch

    core, _ = cores(params(L))
    F = len(prob["facet_off0s"])
    work = torch.empty((F if workspace_facets is None else workspace_facets, core.yN_size, core.xM_yN_size),
                       dtype=torch.complex64, device="cuda")
    got = acc_run_at(params(L), bits, prob, work)
    return check("accumulate_facet_columns", L, bits, got, prob["want"], 1, acc_has_f64(L), note=f"F {F}")


def acc_run_at(p, bits, prob, workspace, two_chunks=False):
    """:py:func:`acc_run` for the parameter set ``p`` up to the comparison of the touched columns: returns them,
    ``got[F, yB, columns]``.  ``workspace``: a device tensor, or None (the library allocates its own).  ``two_chunks``: the
    last subgrid of every wave in a source chunk of its own that lies BELOW the first chunk in memory (offsets are
    relative to the lowest address), both chunks inside one allocation, the row table naming both."""
    import torch

    core, _ = cores(p)
    yN, m = core.yN_size, core.xM_yN_size
    yB, band, cols = prob["yB"], prob["band"], prob["cols"]
    F = len(prob["facet_off0s"])
    start, length = band
    bands = torch.full((F, yB, length), float("nan"), dtype=torch.complex64, device="cuda")  # uninitialised on purpose
    touched = torch.zeros((length,), dtype=torch.uint8, device="cuda")
    mask_t = torch.from_numpy(prob["masks"]).cuda()
    two_sources = False
    with precision(core, bits):
        for (off1, off0s), pw in zip(prob["waves"], prob["parts"]):
            S = len(off0s)
            if two_chunks:
                pt = torch.empty((F * S * m * m + 64,), dtype=torch.complex64, device="cuda")
                low = pt[: F * m * m].view(F, 1, m, m)
                high = pt[F * m * m + 64:].view(F, S - 1, m, m)
                high.copy_(torch.from_numpy(pw[:, : S - 1]).cuda())
                low.copy_(torch.from_numpy(pw[:, S - 1:]).cuda())
                assert high.data_ptr() > low.data_ptr()
                offs, fstr = [F * m * m + 64, 0], [(S - 1) * m * m, m * m]
                locs = [(0, b) for b in range(S - 1)] + [(1, 0)]
            else:
                pt = torch.from_numpy(pw).cuda()
                offs, fstr, locs = [0], [pt.stride(0)], None
            groups = core.column_row_sources(off0s, locs)
            assert len(groups) == 1 or yN < 4 * m  # (short rings: three windows overlap in some rows, two tables)
            for _, table in groups:
                two_sources |= bool((table[1] >= 0).any())
                if two_chunks:
                    assert sorted(set((table[table >= 0] >> 20).cpu().tolist())) == [0, 1]
                core.accumulate_facet_columns(pt, m, offs, fstr, table, prob["facet_off0s"], yB, mask_t, off1, bands,
                                              band, workspace=workspace, touched=touched)
        core.band_zero_untouched(bands, touched)
    assert two_sources
    tch = touched.cpu().numpy()
    d = (cols - start) % yN
    assert (d < length).all() and (tch[d] == 1).all() and int(tch.sum()) == len(cols)
    if m < yN:  # (m = yN at L = 6, 7: every column is in every window)
        assert (tch == 0).any()
    assert not bool((bands[:, :, torch.from_numpy(tch == 0).cuda()] != 0).any()), "an untouched band column is not zero"
    return bands[:, :, torch.from_numpy(d).cuda()].cpu().numpy()


@pytest.mark.parametrize("L", LENGTHS)
def test_accumulate_facet_columns_lengths(L):
    """the gather-sum column pass at every length class in both precisions: single passes of 64 .. 512 points, the four-steps
    5+5 (1024 points: the gather-sum load has no single pass there) .. 8+8; two waves whose band columns overlap (first-write
    flags + read-modify-write), three subgrids per wave with overlapping row windows (two sources per row), two facets with
    float masks, an odd facet size at L = 9.  No float64 gather-sum instance at 512 points (float32 bound there)."""
    prob = acc_problem(L)
    assert (prob["yB"] % 2 == 1) == (L == 9)
    e32 = acc_run(L, 32, prob)
    e64 = acc_run(L, 64, prob)
    if acc_has_f64(L):
        assert e64 < e32, (L, e64, e32)


def test_accumulate_facet_columns_thirty_three_facets():
    """33 facets cross kColZF = 32: the second launch group starts at facet 32 of the chunk offsets, the masks and the bands"""
    prob = acc_problem(8, F=33, n_waves=1, seed=33)
    for bits in (32, 64):
        acc_run(8, bits, prob)


def test_accumulate_facet_columns_workspace_of_one_facet():
    """a workspace sized for one facet gives ``per_f = 1``: three launch groups for three facets"""
    prob = acc_problem(8, F=3, n_waves=2, seed=3)
    for bits in (32, 64):
        acc_run(8, bits, prob, workspace_facets=1)


# ------------------------------------------------------------------------------------ (c) K1, prepare_facet_band
def data_segments(yN, size, off, seglen):
    """the run of load segments that hold data (data_segment_run of csrc/row_pass.hip, same arithmetic)"""
    lo = yN // 2 - size // 2
    base = ((-(off + lo)) % yN + yN // 2) % yN
    valid = [(seglen * r + base) % yN < size or (seglen * r + base) % yN + seglen > yN for r in range(yN // seglen)]
    return sum(valid)


def k1_run(core, ref, L, x, xt, off, band, fold, rows_of=None, note="", label=None):
    import torch

    yN = core.yN_size
    rows = x.shape[0]
    ncols = core.band_columns(band)
    obuf = torch.full((rows + 1, ncols + 16), SENTINEL, dtype=torch.complex64, device="cuda")
    out = obuf[:rows, :ncols]
    res = core.prepare_facet_band(xt, off, band, out=out, fold_other_axis_window=fold, rows_of=rows_of)
    assert res is out
    assert bool((obuf[rows] == SENTINEL).all()) and bool((obuf[:, ncols:] == SENTINEL).all()), \
        "prepare_facet_band wrote right of band_columns(band)"
    want = ref.prepare_facet(x.astype(complex), off, 1)
    if fold:
        size, row0 = rows_of if rows_of is not None else (rows, 0)
        want = want * ref.facet_window(size)[row0 : row0 + rows, None]
    got = out.cpu().numpy()
    if is_split(core):
        pc = band_cols(yN, band)
        keep = pc >= 0
        got, want = got[:, pc[keep]], want[:, keep]
    return check("prepare_facet_band", L, 32, got, want, 1, note=note, label=label)


@pytest.mark.parametrize("L", K1_LENGTHS)
def test_prepare_facet_band_lengths(L):
    """K1 in complex64 on 7 rows (not a multiple of the 8 rows per workgroup pair): the generic rows with the plain band
    layout (L < 14), BandGeo16k, the 32768-point pair / odd-offset kernels and the 65536-point kernel with NSEG = 44 and,
    for more than 44 segments of data, its generic instance; facet offsets 0, negative, odd and >= N; the axis-0 window
    folded in and not; split sizes: full, interior and odd wrapping bands, and a block of rows of a taller facet."""
    import torch

    core, ref = cores(params(L))
    yN, N = core.yN_size, core.N
    split = L in SPLIT_LENGTHS
    assert split == is_split(core)
    rows = 7
    offs = [0, -(3 * yN // 16), (yN // 7) | 1, N + yN // 8]
    sizes = [facet_size(L)] + ([47000] if L == 16 else [])
    bands = [(0, yN)]
    if split:
        bands += [(yN // 3, yN // 3 + 16), ((yN - yN // 32) | 1, (yN // 16) | 1)]
        assert bands[2][0] % 2 == 1 and bands[2][1] % 2 == 1 and bands[2][0] + bands[2][1] > yN
    rng = numpy.random.default_rng(2100 + L)
    for size in sizes:
        assert size % 2 == 0 and size < yN
        if L == 16:  # both instances of the 65536-point band store
            segs = [data_segments(yN, size, off, 1024) for off in offs]
            assert (min(segs) <= 44 < max(segs)) if size == sizes[0] else min(segs) > 44, segs
        x = crandn(rng, (rows, size))
        xt = torch.from_numpy(x).cuda()
        for io, off in enumerate(offs):
            for ib, band in enumerate(bands):
                k1_run(core, ref, L, x, xt, off, band, fold=(io + ib) % 2 == 0, note=f"size {size} off {io} band {ib}")
    if split:
        k1_run(core, ref, L, x, xt, offs[1], bands[1], fold=True, rows_of=(20, 5), note="rows 5..12 of 20")
    elif L == 10:
        with pytest.raises(NotImplementedError):
            core.prepare_facet_band(xt, 0, (16, 512))


# ------------------------------------------------------------------------------------ (d) finish_facet_band
def finish_band_run(core, ref, L, rng, band, off, yB, mask, rows=24, note=""):
    import torch

    yN = core.yN_size
    start, length = band
    data = crandn(rng, (rows, length))
    full = numpy.zeros((rows, yN), dtype=complex)
    full[:, (start + numpy.arange(length)) % yN] = data
    want = ref.finish_facet(full, off, yB, axis=1) * mask[None, :]
    obuf = torch.full((rows + 1, yB + 5), SENTINEL, dtype=torch.complex64, device="cuda")
    out = obuf[:rows, :yB]
    res = core.finish_facet_band(torch.from_numpy(data).cuda(), band, off, yB, mask=mask, out=out)
    assert res is out
    assert bool((obuf[rows] == SENTINEL).all()) and bool((obuf[:, yB:] == SENTINEL).all()), "finish_facet_band wrote outside its rows"
    got = out.cpu().numpy()
    assert not got[:, mask == 0].any()  # masked pixels are exactly zero
    return check("finish_facet_band", L, 32, got, want, 1, note=note)


@pytest.mark.parametrize("L", K1_LENGTHS)
def test_finish_facet_band_lengths(L):
    """finish_facet along the contiguous axis of a band accumulator (plain column order, zero outside the band): the generic
    rows up to 8192 points, BandGeo16k, the NSEG = 13 / 16 instances at 32768 (a band of 15000 columns spans 15 or 16
    segments of 1024) and the 65536-point kernel; interior, wrapping and full bands, a partial mask"""
    core, ref = cores(params(L))
    yN = core.yN_size
    yB = facet_size(L)
    rng = numpy.random.default_rng(3100 + L)
    mask = (rng.random(yB) > 0.15).astype(float)
    assert 0 < mask.sum() < yB
    cases = [((yN // 2 - 5 * yN // 32, 11 * yN // 32 + 8), 0), ((yN - 3 * yN // 32, 7 * yN // 32 + 1), yB), ((0, yN), -yB)]
    if L == 15:
        cases.append(((yN // 4 + 1, 15000), 3 * 352))
    assert cases[1][0][0] + cases[1][0][1] > yN
    for k, (band, off) in enumerate(cases):
        finish_band_run(core, ref, L, rng, band, off, yB, mask, note=f"band {k}")


# ------------------------------------------------------------------------------------ (e) finish_axis1_rows
@pytest.mark.parametrize("logm,logx,L", AXIS1_CASES, ids=[f"m{1 << a}-xM{1 << b}-yN{1 << c}" for a, b, c in AXIS1_CASES])
def test_finish_axis1_rows_instances(logm, logx, L):
    """one instance per m in {128, 256, 512, 1024}: 6 rows, 2 facets with different off1 and data, three wave offsets (one
    negative), a partial band that contains the windows; composed as test_finish_axis1_rows_matches_oracle"""
    import torch

    m, xM, yN = 1 << logm, 1 << logx, 1 << L
    core, ref = cores(dict(N=xM * yN // m, xM=xM, yN=yN))
    N = core.N
    assert core.xM_yN_size == m
    fstep, sstep = core.facet_off_step, core.subgrid_off_step
    rows = 6
    full = crandn(numpy.random.default_rng(700 + 10 * logm + L), (2, rows, yN))
    facet_off1s = [3 * fstep, -(m // 3) * fstep]
    sub_off1s = [0, (yN // 20) * sstep, -(yN // 25) * sstep]
    band = core.band_for_offsets(sub_off1s)
    assert band[1] < yN
    bands = torch.from_numpy(pack_bands(core, full, band)).cuda()
    k = numpy.arange(m)
    for sub_off1 in sub_off1s:
        obuf = torch.full((2, rows + 1, m + 8), SENTINEL, dtype=torch.complex64, device="cuda")
        out = obuf[:, :rows, :m]
        res, wband = core.finish_axis1_rows(bands, facet_off1s, band, sub_off1, out=out)
        s = sub_off1 * yN // N
        assert res is out and wband == ((yN // 2 - m // 2 + s) % yN, m)
        assert bool((obuf[:, rows] == SENTINEL).all()) and bool((obuf[:, :, m:] == SENTINEL).all())
        got = out.cpu().numpy()
        wpc = band_cols(yN, wband)
        want = numpy.empty((2, rows, m), dtype=complex)
        for f, foff in enumerate(facet_off1s):
            contrib = ref.extract_from_facet(full[f].astype(complex), sub_off1, 1)  # [rows, m]
            placed = ref.add_to_subgrid(contrib, foff, 1)  # [rows, xM]
            Z = placed[:, (k + xM // 2 - m // 2 + foff * xM // N) % xM]
            want[f] = Z[:, (k + s) % m]  # logical window element i holds Z[(i + s) mod m]
        check("finish_axis1_rows", L, 32, got[:, :, wpc[(wband[0] + k) % yN]], want, 2, stages=logm, note=f"m {m} off1 {sub_off1}")
    with pytest.raises(ValueError):  # a window outside the band
        core.finish_axis1_rows(bands, facet_off1s, band, (yN // 2) * sstep)


# ------------------------------------------------------------------------------------ (f) gates and entry points agree
def _gate(feature, p):
    from ska_sdp_exec_swiftly_amd import _lib

    return bool(_lib.load().swiftly_hip_supports(getattr(_lib, "FEATURE_" + feature), _lib.C64, p["N"], p["yN"], p["xM"], 0))


def _stand_in_core(p, monkeypatch):
    """a core whose window function is a cheap stand-in: for sizes every entry point under test must refuse before it looks
    at any table (the real window costs seconds from 131072 points on)"""
    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip, core_hip

    def flat(_, yN):
        vals = numpy.cos(numpy.linspace(-1.2, 1.2, yN))
        vals[0] = 0.0
        return vals

    with monkeypatch.context() as patch:  # (undone at once: the cores built afterwards get the real window)
        patch.setattr(core_hip, "calculate_pswf", flat)
        return SwiftlyCoreHip(W, p["N"], p["xM"], p["yN"])


def backward_tiny(core, ref, L, seed):
    """accumulate_facet_columns (one facet, one wave, two overlapping subgrids) + finish_facet_band on tiny data"""
    import torch

    N, yN, m = core.N, core.yN_size, core.xM_yN_size
    sstep = core.subgrid_off_step
    yB = min(40, yN // 2)
    rng = numpy.random.default_rng(seed)
    s1, s0s = yN // 8, [0, m // 2]
    parts = crandn(rng, (1, 2, m, m))
    acc = numpy.zeros((yN, m), dtype=complex)
    for b, s0 in enumerate(s0s):
        acc = ref.add_to_facet(parts[0, b].astype(complex), s0 * sstep, axis=0, out=acc)
    off0 = 3 * core.facet_off_step
    fin = ref.finish_facet(acc, off0, yB, axis=0)  # [yB, m]
    i = numpy.arange(m)
    want = fin[:, (i + s1) % m]  # window index i
    bands = torch.full((1, yB, yN), float("nan"), dtype=torch.complex64, device="cuda")
    touched = torch.zeros((yN,), dtype=torch.uint8, device="cuda")
    pt = torch.from_numpy(parts).cuda()
    for _, table in core.column_row_sources([s * sstep for s in s0s]):
        core.accumulate_facet_columns(pt, m, [0], [pt.stride(0)], table, [off0], yB, None, s1 * sstep, bands, (0, yN),
                                      touched=touched)
    core.band_zero_untouched(bands, touched)
    got = bands.cpu().numpy()[0][:, (yN // 2 - m // 2 + i + s1) % yN]
    check("gate: accumulate", L, 32, got, want, 0, note=f"yN {yN}")
    finish_band_run(core, ref, L, rng, (yN // 4, yN // 2 + 1), off0, yB, numpy.ones(yB), rows=3, note=f"gate yN {yN}")


def forward_tiny(core, ref, L, seed):
    """K1 + K2 on tiny data (whole band)"""
    import torch

    yN = core.yN_size
    rng = numpy.random.default_rng(seed)
    x = crandn(rng, (3, min(40, yN // 2)))
    k1_run(core, ref, L, x, torch.from_numpy(x).cuda(), 5 * core.facet_off_step, (0, yN), fold=True, note=f"gate yN {yN}")
    logical = crandn(rng, (1, 24, yN))
    off0, off1 = -3 * core.facet_off_step, (yN // 9) * core.subgrid_off_step
    got = k2_run(core, torch.from_numpy(pack_bands(core, logical, (0, yN))).cuda(), [off0], (0, yN), off1, None, yN)
    check("gate: prepare_facet_columns", L, 32, got[0], k2_want(ref, logical[0], off0, off1), 0, note=f"yN {yN}")


def backward_refuses(core):
    """both entry points of the backward band raise NotImplementedError and leave their outputs alone"""
    import torch

    yN, m = core.yN_size, core.xM_yN_size
    bands = torch.full((1, 8, 16), SENTINEL, dtype=torch.complex64, device="cuda")
    parts = torch.zeros((1, 1, m, m), dtype=torch.complex64, device="cuda")
    table = torch.full((2, yN), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(NotImplementedError):
        core.accumulate_facet_columns(parts, m, [0], [parts.stride(0)], table, [0], 8, None, 0, bands, (0, 16))
    out = torch.full((2, 8), SENTINEL, dtype=torch.complex64, device="cuda")
    with pytest.raises(NotImplementedError):
        core.finish_facet_band(bands[0, :2], (0, 16), 0, 8, out=out)
    assert bool((bands == SENTINEL).all()) and bool((out == SENTINEL).all())


def forward_refuses(core, upper):
    """the band pipeline cannot run: above the range K1 and K2 refuse; below it (m = 64) the sum over facets has no instance --
    K1, K2 and K3 are shared with other paths (the L = 6 sweep core runs K2) and do run there"""
    import torch

    yN, m, xM = core.yN_size, core.xM_yN_size, core.xM_size
    if upper:
        x = torch.zeros((2, 8), dtype=torch.complex64, device="cuda")
        out = torch.full((2, core.band_columns((0, yN))), SENTINEL, dtype=torch.complex64, device="cuda")
        with pytest.raises(NotImplementedError):
            core.prepare_facet_band(x, 0, (0, yN), out=out)
        bands = torch.zeros((1, 8, out.shape[1]), dtype=torch.complex64, device="cuda")
        q = torch.full((1, 4, m), SENTINEL, dtype=torch.complex64, device="cuda")
        rowmap = torch.full((yN,), -1, dtype=torch.int32, device="cuda")
        with pytest.raises(NotImplementedError):
            core.prepare_facet_columns(bands, [0], (0, yN), 0, rowmap, 4, out=q)
        assert bool((out == SENTINEL).all()) and bool((q == SENTINEL).all())
    else:
        G = torch.zeros((1, 1, m, m), dtype=torch.complex64, device="cuda")
        out = torch.full((1, xM, 33), SENTINEL, dtype=torch.complex64, device="cuda")
        with pytest.raises(NotImplementedError):
            core.sum_finish_facets(G, [0], [0], out, [0], 33)
        assert bool((out == SENTINEL).all())


def _sizes(logm, logx, yN):
    xM = 1 << logx
    return dict(N=(xM * yN) >> logm, xM=xM, yN=yN)


#: feature -> (first refused below, first accepted, last accepted, first refused above) as log2 yN; settled from
#: csrc/swiftly_caps.h and the table builders of csrc/swiftly_abi.hip (make_twiddles: float tables for 2^3 .. 2^16)
GATE_EDGES = {"BACKWARD_BAND": (5, 6, 16, 17), "BAND_PIPELINE": (6, 7, 16, 17)}


def _edge_params(feature, L):
    if feature == "BACKWARD_BAND":
        return params(L) if L >= 6 else _sizes(L, L + 1, 1 << L)  # (L = 5: (N, xM, yN) = (64, 64, 32), m = 32)
    return params(L) if L >= 7 else _sizes(L, 8, 1 << L)  # (L = 6 with xM = 256: m = 64, no sum_finish pair)


@pytest.mark.parametrize("feature", list(GATE_EDGES))
def test_gate_and_entry_points_agree_power_of_two(feature, monkeypatch):
    """swiftly_hip_supports and the entry points answer alike at the first and last accepted yN = 2^L and at the first
    refused one on each side.  The refused cores get a stand-in window function (nothing is computed with it)."""
    lo_out, lo_in, hi_in, hi_out = GATE_EDGES[feature]
    assert (lo_in, hi_in) == ((LENGTHS if feature == "BACKWARD_BAND" else K1_LENGTHS)[0], LENGTHS[-1])
    for L in (lo_in, hi_in):
        p = _edge_params(feature, L)
        assert _gate(feature, p), (feature, L)
        core, ref = cores(p)
        (backward_tiny if feature == "BACKWARD_BAND" else forward_tiny)(core, ref, L, 4000 + L)
    for L in (lo_out, hi_out):
        p = _edge_params(feature, L)
        assert not _gate(feature, p), (feature, L)
        core = _stand_in_core(p, monkeypatch)
        if feature == "BACKWARD_BAND":
            backward_refuses(core)
        else:
            forward_refuses(core, upper=L == hi_out)


#: yN = 3 * 2^k: feature -> log2 of (m, xM) at (first refused below, first accepted, last accepted, first refused above)
MIXED_EDGES = {
    "BACKWARD_BAND": ((5, (5, 5)), (6, (6, 7)), (15, (7, 8)), (16, (7, 8))),
    "BAND_PIPELINE": ((6, (6, 8)), (7, (7, 8)), (15, (7, 8)), (16, (7, 8))),
}


def test_gate_and_entry_points_agree_three_times_power_of_two(monkeypatch):
    """the same for ``yN = 3 * 2^k`` (radix-3 pass in front of the power-of-two kernels): BACKWARD_BAND accepts k = 6 .. 15,
    BAND_PIPELINE (m >= 128) k = 7 .. 15.  The last accepted size, 98304 points, needs a real window function: 3 s of host
    time for the core and 3 s for the oracle -- the only such size in the module, one core for both features."""
    for feature, edges in MIXED_EDGES.items():
        for j, (k, (logm, logx)) in enumerate(edges):
            p = _sizes(logm, logx, 3 << k)
            assert _gate(feature, p) == (j in (1, 2)), (feature, k, p)
            if j in (1, 2):
                core, ref = cores(p)
                # (stage count of the bound: the radix-3 pass counts as two)
                (backward_tiny if feature == "BACKWARD_BAND" else forward_tiny)(core, ref, k + 2, 5000 + k)
            else:
                core = _stand_in_core(p, monkeypatch)
                if feature == "BACKWARD_BAND":
                    backward_refuses(core)
                else:
                    forward_refuses(core, upper=j == 3)
