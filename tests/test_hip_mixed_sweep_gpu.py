"""
Every radix-Q length class of the facet-side kernels against the 1-D oracle.

171 of the 244 catalogue entries have a padded facet size ``yN = Q * 2^k`` with Q in {3, 5, 7, 9}; with power-of-two ``xM``
and ``m >= 64`` they run the radix-Q forms by default (csrc/swiftly_mixed.h): ``mixed_radix_pass_kernel<Q>`` -- along the
contiguous axis in ``prepare_facet_band`` / ``finish_facet_band`` (``run_rows_mixed``, the one-launch "all j" form of the
sub-transforms), with lanes along the rows (``rowfast``), the modular row map and per-facet load offsets in K2
(``prepare_facet_columns_mixed``) -- and the gather-sum pass ``mixed_gs_pass_kernel<Q>`` of ``accumulate_facet_columns``, each
followed by Q power-of-two sub-transforms whose store side carries the output index ``Q * k2 + j``.  This module runs each
of them through the entry points at every ``(Q, k)`` class of the catalogue -- Q = 3: k = 7 .. 14, Q = 5, 7: k = 7 .. 13,
Q = 9: k = 12 -- as the power-of-two sweep (tests/test_hip_facet_sweep_gpu.py) does for ``yN = 2^L``, with its helpers, and
compares ALL output elements with a composition of the complex128 primitives of oracle/swiftly_oracle.py (numpy takes any
length).  No expected value comes from another HIP path or from Bluestein; SWIFTLY_NO_MIXED stays unset.

Cores: W = 11, ``yN = Q * 2^k``, ``N = 2 yN``; ``xM = 256`` (``m = 128``) for k >= 7 and ``xM = 128`` (``m = 64``) for k = 6.  Every
test asserts that the library sees the intended ``(Q, k)`` (``swiftly_hip_mixed_factor``) and that ``supports_backward_band``
accepts the core, and ``supports_band_pipeline`` for k >= 7 (at ``m = 64`` the forward pipeline has no sum over facets; K2
itself runs there, as at L = 6 of the power-of-two sweep).  These sizes keep the plain band layout (asserted).

Classes
* (a), (b): every Q at k = 6, 7, 9, 10, 11 -- sub-transforms in single passes of 64, 128 and 512 points, the 1024-point single
  pass without a float64 instance, the smallest four-step -- the catalogue's largest class per Q, (3, 14), (5, 13), (7, 13),
  (9, 12), and the upper edge of the capability table, (3, 15) (``kBandMixedMaxLog``).
* (c): every Q at k = 7 and 10, the four largest classes and (3, 15).
* (d): every Q at k = 8 and 9 through the generic primitives (``prepare_facet`` / ``finish_facet`` on host arrays), along axis 0
  with 70 columns (not a multiple of the 64 lanes; k = 9: the per-j four-step along a strided axis) and along axis 1 with 5
  rows, in complex64 and complex128.

Bounds (none tuned against the kernels)
* float32 arithmetic: relative RMSE over the whole output below ``2e-6 * sqrt(min(s, 15) / 15)`` with ``s = ceil(log2 yN)`` --
  the rule of the power-of-two sweep at the full length; the Q-term sum of the radix pass stands for its ``log2 Q`` stages --
  and ``max|err| <= 2e-5 * max|want|`` for every transformed vector.
* ``column_precision = 64``: the radix pass stays float32 (``MixedArgs<float>``), only the sub-transforms change, so both
  settings are held to the float32 bound and float64 is not required to beat float32; both figures are recorded.  The
  setting has to REACH the sub-transforms, though: in (a) and (b) the two settings must give different bits, and the same
  bits at k = 10, whose 1024-point single pass has no float64 instance (``assert_precision_honoured``).
* complex128 primitives of (d): relative RMSE below 1e-11 (the figure of tests/test_hip_nonpow2_gpu.py for them).
* padding, sentinels, untouched band columns and masked pixels compare exactly.

Every case prints ``MIXEDSWEEP <what> Q=.. k=.. f32|f64 <value> (bound ..) peak ..`` lines (``pytest -s``).

Measured on an MI355X: the worst relative RMSE over the cases of one class (float32 bounds 1.46e-06 at yN = 192 .. 2.0e-06
from yN = 16385 on).  K2 = prepare_facet_columns, acc = accumulate_facet_columns, K1 = prepare_facet_band, rows =
prepare_facet_band_rows, fin = finish_facet_band; at k = 10 both precisions run the float32 1024-point pass:

  Q   k   K2 f32   K2 f64  acc f32  acc f64   K1 f32 rows f32  fin f32
  3   6  9.8e-08  5.4e-08  1.1e-07  6.1e-08        -        -        -
  5   6  9.8e-08  5.6e-08  1.1e-07  6.1e-08        -        -        -
  7   6  1.0e-07  6.7e-08  1.1e-07  6.2e-08        -        -        -
  9   6  1.0e-07  5.6e-08  1.1e-07  6.4e-08        -        -        -
  3   7  1.0e-07  4.9e-08  1.1e-07  6.1e-08  1.3e-07  1.3e-07  1.3e-07
  5   7  1.0e-07  5.2e-08  1.1e-07  6.3e-08  1.2e-07  1.3e-07  1.2e-07
  7   7  1.0e-07  6.3e-08  1.1e-07  6.4e-08  1.2e-07  1.3e-07  1.3e-07
  9   7  1.1e-07  5.1e-08  1.2e-07  6.5e-08  1.3e-07  1.4e-07  1.4e-07
  3   9  1.1e-07  5.0e-08  1.3e-07  5.4e-08        -        -        -
  5   9  1.1e-07  5.1e-08  1.3e-07  5.8e-08        -        -        -
  7   9  1.1e-07  6.4e-08  1.3e-07  5.7e-08        -        -        -
  9   9  1.2e-07  5.0e-08  1.3e-07  5.9e-08        -        -        -
  3  10  1.2e-07  1.2e-07  1.4e-07  1.4e-07  1.5e-07  1.5e-07  1.5e-07
  5  10  1.2e-07  1.2e-07  1.4e-07  1.4e-07  1.4e-07  1.4e-07  1.5e-07
  7  10  1.2e-07  1.2e-07  1.4e-07  1.4e-07  1.5e-07  1.5e-07  1.5e-07
  9  10  1.3e-07  1.3e-07  1.4e-07  1.4e-07  1.5e-07  1.6e-07  1.5e-07
  3  11  1.1e-07  5.6e-08  1.3e-07  6.0e-08        -        -        -
  5  11  1.2e-07  5.7e-08  1.3e-07  6.2e-08        -        -        -
  7  11  1.2e-07  7.0e-08  1.3e-07  6.3e-08        -        -        -
  9  11  1.2e-07  5.6e-08  1.3e-07  6.3e-08        -        -        -
  9  12  1.3e-07  5.7e-08  1.3e-07  6.4e-08  1.7e-07  1.7e-07  1.7e-07
  5  13  1.3e-07  5.9e-08  1.3e-07  6.2e-08  1.6e-07  1.6e-07  1.6e-07
  7  13  1.2e-07  6.9e-08  1.3e-07  6.3e-08  1.6e-07  1.6e-07  1.7e-07
  3  14  1.2e-07  5.7e-08  1.4e-07  6.0e-08  1.7e-07  1.7e-07  1.7e-07
  3  15  1.2e-07  5.6e-08  1.5e-07  6.0e-08  1.7e-07  1.8e-07  1.9e-07

Worst per-vector peak (bound 2e-05): K2 1.1e-06, acc 4.6e-07, K1 2.7e-07, rows 2.9e-07, fin 3.0e-07.  Launch groups, float32 /
float64: K2 with 33 facets at (5, 7) 1.0e-07 / 5.1e-08 (facets 31 and 32 alone 1.0e-07 and 9.9e-08); accumulate with 33
facets at (7, 7) 1.2e-07 / 6.6e-08, with the exact caller's workspace at (5, 8) 1.2e-07 / 6.0e-08 and the same bits with
one byte less, in two source chunks at (9, 7) 1.2e-07 / 6.5e-08.  (d): complex64 1.2e-07 .. 1.5e-07 over Q, k = 8, 9 and the
four calls; complex128 3.0e-16 .. 3.8e-16 (bound 1e-11).

Found by this sweep: K2 ignored ``column_precision = 64`` at these sizes -- ``prepare_facet_columns_mixed`` never handed the
setting to its sub-transforms (``accumulate_facet_columns`` did) -- so ``test_prepare_facet_columns_classes`` failed
``assert_precision_honoured`` at every class but k = 10; e.g. K2 with 33 facets at (5, 7): float32 / float64 1.013e-07 /
1.013e-07 before, 1.013e-07 / 5.1e-08 with the setting passed on (csrc/swiftly_abi_pipeline.hip).  The whole-axis
accumulator at (3, 15) with 0.69 yN rows is refused by ``accumulate_facet_columns`` ("strides too large for 32-bit
offsets"; see ``acc_problem``): a limit of the entry point above the catalogue's sizes, left as it is.

Module wall time on an MI355X: 33 s for the 109 cases (pytest's own figure); the slowest case, K2 at (3, 15) with one facet,
takes 4.0 s, accumulate there 2.6 s with two facets: both keep their two off1 / two waves.  Much of the time is the host's: the
window function of the two cores of a class (4 s at 98304 points) and the oracle's complex128 transforms.
"""
import numpy
import pytest

import test_hip_facet_sweep_gpu as fs
from test_hip_facet_sweep_gpu import SENTINEL, check, crandn, k1_run, k2_offsets, k2_run, k2_want, precision, vector_peak

pytestmark = pytest.mark.gpu

QS = (3, 5, 7, 9)
#: the catalogue's largest class per Q, and the upper edge of the capability table (kBandMixedMaxLog, csrc/swiftly_caps.h)
LARGEST = [(3, 14), (5, 13), (7, 13), (9, 12)]
EDGE = (3, 15)
COLUMN_CLASSES = [(Q, k) for k in (6, 7, 9, 10, 11) for Q in QS] + LARGEST + [EDGE]
ROW_CLASSES = [(Q, k) for k in (7, 10) for Q in QS] + LARGEST + [EDGE]
PRIMITIVE_CLASSES = [(Q, k) for k in (8, 9) for Q in QS]
C128_TOL = 1e-11


def ids(classes):
    return [f"Q{Q}-k{k}" for Q, k in classes]


def params(Q, k):
    yN = Q << k
    return dict(N=2 * yN, xM=128 if k == 6 else 256, yN=yN)


def case(Q, k):
    """``(core, oracle core, stage count of the bound)`` of a class; the library must see ``(Q, k)`` and accept the core"""
    import torch

    from ska_sdp_exec_swiftly_amd.core_hip import mixed_factor

    p = params(Q, k)
    core, ref = fs.cores(p)
    yN = core.yN_size
    assert mixed_factor(yN) == (Q, k), (yN, mixed_factor(yN))
    assert core.xM_yN_size == p["xM"] // 2 == ref.xM_yN_size
    assert core.supports_backward_band(torch.complex64), (Q, k)
    assert core.supports_band_pipeline(torch.complex64) == (k >= 7), (Q, k)
    assert not fs.is_split(core)  # plain band layout
    return core, ref, (yN - 1).bit_length()


def assert_precision_honoured(k, got32, got64):
    """``column_precision = 64`` reaches the sub-transforms: float64 butterflies round differently, so the outputs of the
    two settings differ -- except at k = 10, whose 1024-point single pass has no float64 instance: the same kernel, the
    same bits"""
    assert bool((got32 != got64).any()) == (k != 10), ("column_precision = 64", k)


def label(what, Q, k):
    return f"MIXEDSWEEP {what:<30s} Q={Q} k={k:<2d}"


def rng_for(base, Q, k):
    return numpy.random.default_rng(base + 32 * Q + k)


# ------------------------------------------------------------------------------------ (a) K2, prepare_facet_columns
@pytest.mark.parametrize("Q,k", COLUMN_CLASSES, ids=ids(COLUMN_CLASSES))
def test_prepare_facet_columns_classes(Q, k):
    """K2 in complex64, float32 and float64 sub-transforms: ``mixed_radix_pass_kernel<Q>`` with lanes along the window columns,
    the modular row map of the window and per-facet load offsets, then Q sub-transforms storing rows ``Q * k2 + j``; 2 facets
    (one negative off0; one facet at (3, 15)), two off1 (one negative), with and without the row map of
    subgrid_column_rows; sentinel-padded output, all elements compared."""
    import torch

    core, ref, s = case(Q, k)
    yN = core.yN_size
    F = 1 if (Q, k) == EDGE else 2
    logical = crandn(rng_for(6000, Q, k), (F, 96, yN))
    off0s, off1s, map_offs = k2_offsets(core)
    off0s = off0s[:F]
    assert off1s[1] < 0 < off1s[0] and off0s[0] > 0 and (F == 1 or off0s[1] < 0)
    rowmap, n_kept = core.subgrid_column_rows(map_offs)
    rm = rowmap.cpu().numpy()
    assert n_kept < yN
    assert core.band_for_offsets(off1s) == (0, yN)
    want = {(i, f): k2_want(ref, logical[f], off0s[f], off1s[i]) for i in range(2) for f in range(F)}
    dev = torch.from_numpy(logical).cuda()
    got32 = {}
    for bits in (32, 64):
        with precision(core, bits):
            for i in range(2):
                for use_rowmap in (False, True):
                    got = k2_run(core, dev, off0s, (0, yN), off1s[i], rowmap if use_rowmap else None, n_kept if use_rowmap else yN)
                    keep = rm >= 0 if use_rowmap else numpy.ones(yN, dtype=bool)
                    idx = rm[keep] if use_rowmap else numpy.arange(yN)
                    w = numpy.stack([want[(i, f)][keep] for f in range(F)])
                    check("prepare_facet_columns", s, bits, got[:, idx], w, 1, note=f"off1 {i} rowmap {int(use_rowmap)}",
                          label=label("prepare_facet_columns", Q, k))
                    if bits == 32:
                        got32[(i, use_rowmap)] = got
                    else:
                        assert_precision_honoured(k, got32.pop((i, use_rowmap)), got)


def test_prepare_facet_columns_thirty_three_facets_radix5():
    """33 facets at (5, 7) cross ``per_f_cap`` = 32 of prepare_facet_columns_mixed: the second launch group starts at facet 32
    of the band buffers, the offsets and the output"""
    import torch

    Q, k = 5, 7
    core, ref, s = case(Q, k)
    yN = core.yN_size
    fstep, sstep = core.facet_off_step, core.subgrid_off_step
    logical = crandn(rng_for(6500, Q, k), (33, 96, yN))
    off0s = [((7 * f) % 61 - 30) * fstep for f in range(33)]
    off1 = (3 - yN // 2) * sstep
    assert len(set(off0s)) == 33
    dev = torch.from_numpy(logical).cuda()
    want = numpy.stack([k2_want(ref, logical[f], off0s[f], off1) for f in range(33)])
    for bits in (32, 64):
        with precision(core, bits):
            got = k2_run(core, dev, off0s, (0, yN), off1, None, yN)
        check("K2 33 facets", s, bits, got, want, 1, label=label("K2 33 facets", Q, k))
        for f in (31, 32):  # the last facet of the first group, the only one of the second
            check(f"K2 33 facets, facet {f}", s, bits, got[f], want[f], 0, label=label(f"K2 33 facets, facet {f}", Q, k))


# ------------------------------------------------------------------------------------ (b) accumulate_facet_columns
def acc_problem(Q, k, F=2, n_waves=2, seed=0):
    """``acc_problem`` of the power-of-two sweep on the core of the class: an odd facet size at k = 9 and, as there from 1024
    points on, a pruned band for k >= 10 (plain layout: band column d at physical column d).  The whole axis would do for
    the kernels, but not for the test: an accumulator of 0.69 yN rows of yN columns is 13 GB per facet at (3, 14) and 53 GB
    at (3, 15), where ``accumulate_facet_columns`` refuses it besides (rows * pitch must stay below 2^32 elements)."""
    core, _, _ = case(Q, k)
    yB = fs.facet_size(0, odd=(k == 9), yN=core.yN_size)
    return fs.acc_problem_at(params(Q, k), yB, rng_for(7000 + 1000 * seed, Q, k), k >= 10, F, n_waves)


def acc_run(Q, k, bits, prob, workspace=None, two_chunks=False, what="accumulate_facet_columns"):
    """``acc_run`` of the power-of-two sweep (touched flags, untouched columns exactly zero, every touched column checked,
    "two sources per row" did occur); returns the touched columns"""
    core, _, s = case(Q, k)
    got = fs.acc_run_at(params(Q, k), bits, prob, workspace, two_chunks)
    check(what, s, bits, got, prob["want"], 1, note=f"F {len(prob['facet_off0s'])}", label=label(what, Q, k))
    return got


@pytest.mark.parametrize("Q,k", COLUMN_CLASSES, ids=ids(COLUMN_CLASSES))
def test_accumulate_facet_columns_classes(Q, k):
    """``mixed_gs_pass_kernel<Q>`` (its own chunk decoding and row tables) + Q sub-transforms with column scatter, accumulate and
    first-write flags on the store side, float32 and float64 sub-transforms: two waves whose band columns overlap, three /
    two subgrids per wave with overlapping row windows, two facets with float masks, NaN-filled accumulators, an odd facet
    size at k = 9, a pruned band for k >= 10"""
    prob = acc_problem(Q, k)
    assert (prob["yB"] % 2 == 1) == (k == 9) and (prob["band"][1] < (Q << k)) == (k >= 10)
    assert_precision_honoured(k, acc_run(Q, k, 32, prob), acc_run(Q, k, 64, prob))


def test_accumulate_facet_columns_thirty_three_facets_radix7():
    """33 facets at (7, 7) cross ``per_f`` = 32: the second launch group starts at facet 32 of the chunk offsets, the masks and
    the bands"""
    prob = acc_problem(7, 7, F=33, n_waves=1, seed=33)
    for bits in (32, 64):
        acc_run(7, 7, bits, prob, what="accumulate 33 facets")


def test_accumulate_facet_columns_caller_workspace_radix5():
    """three facets at (5, 8) with a caller's workspace of exactly ``MixedWorkspace(1, yN, M, m).bytes()`` =
    ``yN m 8 + M m 8 + 4096`` bytes: ``per_f = 1``, three launch groups, the sub-transform scratch carved behind the radix-Q
    scratch (``MixedWorkspace::sub``).  One byte less: the library allocates its own -- the same bits."""
    import torch

    Q, k = 5, 8
    core, _, _ = case(Q, k)
    yN, m, M = core.yN_size, core.xM_yN_size, 1 << k
    nbytes = yN * m * 8 + M * m * 8 + 4096
    prob = acc_problem(Q, k, F=3, n_waves=2, seed=3)
    for bits in (32, 64):
        exact = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
        got = acc_run(Q, k, bits, prob, workspace=exact, what="accumulate exact workspace")
        short = torch.empty((nbytes - 1,), dtype=torch.uint8, device="cuda")
        assert short.numel() // nbytes == 0 and exact.numel() // nbytes == 1
        own = acc_run(Q, k, bits, prob, workspace=short, what="accumulate workspace - 1 byte")
        same = numpy.array_equal(got.view(numpy.uint64), own.view(numpy.uint64))
        print(f"{label('accumulate workspace runs', Q, k)} f{bits:<3d} bit-equal {same}")
        assert same, "the caller's workspace and the library's own give different bits"


def test_accumulate_facet_columns_two_chunks_radix9():
    """(9, 7) with the contributions of every wave in two source chunks inside one allocation (two entries in the offset and
    stride lists, the second chunk below the first in memory), the row table naming both (asserted in ``acc_run_at``)"""
    prob = acc_problem(9, 7)
    for bits in (32, 64):
        acc_run(9, 7, bits, prob, two_chunks=True, what="accumulate two chunks")


# ------------------------------------------------------------------------------------ (c) contiguous axis
def row_cases(core):
    """an even and an odd facet size near 0.69 yN, a positive (odd) and a negative facet offset"""
    yN = core.yN_size
    sizes = [fs.facet_size(0, yN=yN), fs.facet_size(0, odd=True, yN=yN)]
    offs = [(yN // 7) | 1, -(3 * yN // 16)]
    assert sizes[0] % 2 == 0 and sizes[1] % 2 == 1 and offs[1] < 0 < offs[0]
    return sizes, offs


def pitched(x, pad):
    """``x`` on the device as a view of a buffer whose pitch is ``x.shape[1] + pad``"""
    import torch

    buf = torch.full((x.shape[0], x.shape[1] + pad), SENTINEL, dtype=torch.complex64, device="cuda")
    view = buf[:, : x.shape[1]]
    view.copy_(torch.from_numpy(x).cuda())
    assert view.stride(0) != x.shape[1]
    return view


@pytest.mark.parametrize("rows_entry", [False, True], ids=["prepare_facet_band", "prepare_facet_band_rows"])
@pytest.mark.parametrize("Q,k", ROW_CLASSES, ids=ids(ROW_CLASSES))
def test_prepare_facet_band_classes(Q, k, rows_entry):
    """K1 through ``run_rows_mixed``: the radix-Q pass along the contiguous axis and the one-launch "all j" sub-transforms
    (``st_mul`` / ``st_add0`` / ``outer_group``); five rows in a buffer whose pitch is not the row length, sentinel padding
    behind every output row (``k1_run``).  ``prepare_facet_band_rows``: the whole facet as the row block (the plain layout has
    no row blocks), the other-axis window folded in."""
    core, ref, s = case(Q, k)
    assert k >= 7
    yN = core.yN_size
    sizes, offs = row_cases(core)
    rng = rng_for(8000 + 500 * rows_entry, Q, k)
    what = "prepare_facet_band_rows" if rows_entry else "prepare_facet_band"
    for size in sizes:
        x = crandn(rng, (5, size))
        xt = pitched(x, 3)
        for io, off in enumerate(offs):
            fold = rows_entry or io == 0
            k1_run(core, ref, s, x, xt, off, (0, yN), fold=fold, rows_of=(5, 0) if rows_entry else None,
                   note=f"size {size} off {io} fold {int(fold)}", label=label(what, Q, k))


@pytest.mark.parametrize("Q,k", ROW_CLASSES, ids=ids(ROW_CLASSES))
def test_finish_facet_band_classes(Q, k):
    """finish_facet along the contiguous axis of a band accumulator through ``run_rows_mixed``: five rows at a pitch that is
    not the band length, the whole axis and a wrapping band, an even and an odd facet size, a positive and a negative
    offset; crop, mask and Fb on every output pixel, masked pixels exactly zero, sentinel padding behind every row"""
    import torch

    core, ref, s = case(Q, k)
    yN = core.yN_size
    sizes, offs = row_cases(core)
    rng = rng_for(9000, Q, k)
    rows = 5
    bands = [(0, yN), (yN - 3 * yN // 32, 7 * yN // 32 + 1)]
    assert bands[1][0] + bands[1][1] > yN
    for yB in sizes:
        mask = (rng.random(yB) > 0.15).astype(float)
        assert 0 < mask.sum() < yB
        for io, off in enumerate(offs):
            start, length = bands[io]
            data = crandn(rng, (rows, length))
            full = numpy.zeros((rows, yN), dtype=complex)
            full[:, (start + numpy.arange(length)) % yN] = data
            want = ref.finish_facet(full, off, yB, axis=1) * mask[None, :]
            obuf = torch.full((rows + 1, yB + 5), SENTINEL, dtype=torch.complex64, device="cuda")
            out = obuf[:rows, :yB]
            res = core.finish_facet_band(pitched(data, 7), bands[io], off, yB, mask=mask, out=out)
            assert res is out
            assert bool((obuf[rows] == SENTINEL).all()) and bool((obuf[:, yB:] == SENTINEL).all()), \
                "finish_facet_band wrote outside its rows"
            got = out.cpu().numpy()
            assert not got[:, mask == 0].any()  # masked pixels are exactly zero
            check("finish_facet_band", s, 32, got, want, 1, note=f"size {yB} off {io} band {io}",
                  label=label("finish_facet_band", Q, k))


# ------------------------------------------------------------------------------------ (d) generic primitives
@pytest.mark.parametrize("dtype", [numpy.complex64, numpy.complex128], ids=["c64", "c128"])
@pytest.mark.parametrize("Q,k", PRIMITIVE_CLASSES, ids=ids(PRIMITIVE_CLASSES))
def test_facet_primitives_classes(Q, k, dtype):
    """prepare_facet / finish_facet on host arrays: along axis 0 with 70 columns (lanes along the rows; k = 9: one four-step
    pair per j, ``st_mul = Q n1``, ``st_addmul = Q``) and along axis 1 with 5 rows (the one-launch form)"""
    core, ref, s = case(Q, k)
    yN = core.yN_size
    assert core.supports_dtype(dtype)
    sizes, _ = row_cases(core)
    fstep = core.facet_off_step
    rng = rng_for(9500, Q, k)
    c128 = dtype == numpy.complex128

    def rnd(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)

    def compare(what, got, want, axis):
        assert got.dtype == dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
        if not c128:
            return check(what, s, 32, got, want, axis, label=label(what + " c64", Q, k))
        assert numpy.isfinite(got).all(), what
        err, peak = fs.relrms(got, want), vector_peak(got, want, axis)
        print(f"{label(what + ' c128', Q, k)} f64  {err:.3e} (bound {C128_TOL:.2e}) peak {peak:.2e}")
        assert err < C128_TOL, (what, Q, k, err)
        return err

    x0 = rnd(sizes[0], 70)
    compare("prepare_facet axis 0", core.prepare_facet(x0, 5 * fstep, 0), ref.prepare_facet(x0.astype(complex), 5 * fstep, 0), 0)
    x1 = rnd(5, sizes[1])
    compare("prepare_facet axis 1", core.prepare_facet(x1, -7 * fstep, 1), ref.prepare_facet(x1.astype(complex), -7 * fstep, 1), 1)
    a0 = rnd(yN, 70)
    compare("finish_facet axis 0", core.finish_facet(a0, -9 * fstep, sizes[1], 0),
            ref.finish_facet(a0.astype(complex), -9 * fstep, sizes[1], 0), 0)
    a1 = rnd(5, yN)
    compare("finish_facet axis 1", core.finish_facet(a1, 5 * fstep, sizes[0], 1),
            ref.finish_facet(a1.astype(complex), 5 * fstep, sizes[0], 1), 1)
