"""
K3 of a wave whose window lies in two ``Q`` buffers as ONE launch (swiftly_hip_transform_contributions_pieces with the
two-source load of csrc/swiftly_colpass.h, ColPassSrc2): the bits of ``transform_contributions`` (layout 1) on the
assembled window and of the per-piece launches (``swiftly_hip_k3_one_launch(0)``), and the 1-D oracle primitives.

K3 is linear in ``Q``, so the pieces hold random numbers; what a piece does not hold is NaN -- the columns of the other
piece and the physical rows no map entry points to -- so that a column read from the wrong piece, or a row read through
the wrong map or facet stride, cannot pass.  The two row maps keep different supersets of the wave's rows, piece A in
ascending order behind two unused rows, piece B in DESCENDING order (behind one unused row where needed): every shared row sits at different physical
positions, and the facet strides differ.

The small problem of test_hip_k2_slabs_gpu.py (yN = 32768, m = 512, three facets, xA = 928); split p = 16, 272, 496
(p = 16 mod 32: a 32-column tile across the split, at the first, a middle and the last tile), 224 (p = 0 mod 32: every
tile inside one piece), 0 (one piece).  The other instances at their own smallest sizes: float64 column arithmetic at
m = 512, float arithmetic at m = 128 and 256 (64-column tiles: the split inside a wave at p = 16, 48, 112 / 144, on a
tile boundary at p = 64 / 128); m = 64 has no two-source instance and takes the per-piece launches.
"""
import numpy
import pytest

from oracle import swiftly_oracle as orc

pytestmark = pytest.mark.gpu

W64, N64, xM64, yN64, xA, M = 10.875, 65536, 1024, 32768, 928, 512

_cache = {}


def relrms(a, b):
    return float(numpy.sqrt(numpy.mean(numpy.abs(a - b) ** 2) / numpy.mean(numpy.abs(b) ** 2)))


def core_of(W, N, xM, yN, precision=32):
    """one core per configuration for the module"""
    key = (W, N, xM, yN, precision)
    if key not in _cache:
        from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

        _cache[key] = SwiftlyCoreHip(W, N, xM, yN, column_precision=precision)
    return _cache[key]


def one_launch(core, on):
    """sets the library's switch, returns the previous value"""
    return core._lib.swiftly_hip_k3_one_launch(int(on))


def rows_kept(core, sub_off0s):
    return (core.subgrid_column_rows(sub_off0s)[0] >= 0).cpu().numpy()


def two_pieces(core, dtype, F, sub_off0s, extra_a, extra_b, p, seed):
    """``(pieces A and B of the window split at p, assembled Q, the wave's row map)``: piece A holds the positions [p, m),
    piece B [0, p); see the module's docstring for what else they hold"""
    import torch

    m, yN = core.xM_yN_size, core.yN_size
    wave_map, wave_rows = core.subgrid_column_rows(sub_off0s)
    rows = torch.nonzero(wave_map >= 0).flatten()
    keep_a, keep_b = rows_kept(core, list(sub_off0s) + extra_a), rows_kept(core, list(sub_off0s) + extra_b)
    shared = rows.cpu().numpy()
    n_a = int(keep_a.sum()) + 2
    map_a, map_b = numpy.full(yN, -1, dtype=numpy.int32), numpy.full(yN, -1, dtype=numpy.int32)
    map_a[keep_a] = 2 + numpy.arange(n_a - 2, dtype=numpy.int32)
    for lead in (0, 1):  # (an unused first row where the descending order would meet the ascending one on a shared row)
        n_b = int(keep_b.sum()) + lead
        map_b[keep_b] = n_b - 1 - numpy.arange(n_b - lead, dtype=numpy.int32)
        if (map_a[shared] != map_b[shared]).all():
            break
    assert n_a != n_b and (keep_a != keep_b).any() and (map_a[shared] != map_b[shared]).all()
    assert (map_a[shared] != wave_map.cpu().numpy()[shared]).all()
    gen = torch.Generator(device=core.device).manual_seed(seed)
    rdt = torch.float64 if dtype == torch.complex128 else torch.float32
    assembled = torch.zeros((F, wave_rows, m), dtype=dtype, device=core.device)
    pieces = []
    for rowmap, n_rows, pad, first, count in ((map_a, n_a, 11, p, m - p), (map_b, n_b, 5, 0, p)):
        rowmap = torch.from_numpy(rowmap).to(core.device)
        Q = torch.full((F, n_rows + pad, m), float("nan"), dtype=dtype, device=core.device)[:, :n_rows]  # (facet stride)
        used = rowmap[rowmap >= 0].long()
        fill = torch.randn((F, used.numel(), count, 2), generator=gen, dtype=rdt, device=core.device)
        Q[:, used, first:first + count] = torch.view_as_complex(fill)
        assembled[:, wave_map[rows].long(), first:first + count] = Q[:, rowmap[rows].long(), first:first + count]
        pieces.append((Q, rowmap, n_rows, first, count))
    assert pieces[0][0].stride(0) != pieces[1][0].stride(0)
    assert not torch.isnan(torch.view_as_real(assembled)).any()
    return pieces, assembled, wave_map


def check_bits(core, dtype, off0s, sub_off0s, extra_a, extra_b, p, seed=5, order=(0, 1)):
    """one launch == transform_contributions on the assembled window == one launch per piece; returns what they gave"""
    import torch

    pieces, assembled, wave_map = two_pieces(core, dtype, len(off0s), sub_off0s, extra_a, extra_b, p, seed)
    pieces = [pieces[i] for i in order]
    want = core.transform_contributions(assembled, 1, off0s, sub_off0s, rowmap=wave_map)
    assert not torch.isnan(torch.view_as_real(want)).any()
    assert one_launch(core, 1) == 1  # (the default; every test leaves it on)
    got = core.transform_contributions_pieces(pieces, off0s, sub_off0s, torch.full_like(want, float("nan")))
    assert torch.equal(got, want)
    try:
        one_launch(core, 0)
        per_piece = core.transform_contributions_pieces(pieces, off0s, sub_off0s, torch.full_like(want, float("nan")))
    finally:
        one_launch(core, 1)
    assert torch.equal(per_piece, want)
    return pieces, assembled, want


def small_problem():
    core = core_of(W64, N64, xM64, yN64)
    fstep = core.facet_off_step
    return core, [0, 0, -70 * fstep], [0, 2 * xA]  # (the facets' off0s of test_hip_k2_slabs_gpu.py)


@pytest.mark.parametrize("p,order", [(16, (0, 1)), (272, (0, 1)), (496, (0, 1)), (224, (0, 1)), (16, (1, 0)), (224, (1, 0))])
def test_one_launch_gives_the_bits_of_the_assembled_window(p, order):
    """(the pieces in either order of the call)"""
    import torch

    core, off0s, sub_off0s = small_problem()
    check_bits(core, torch.complex64, off0s, sub_off0s, [69 * xA], [5 * xA], p, order=order)


def test_an_empty_piece_is_the_plain_launch():
    """p = 0: the window lies in one slab -- one piece, or two of which one is empty"""
    import torch

    core, off0s, sub_off0s = small_problem()
    pieces, assembled, wave_map = two_pieces(core, torch.complex64, len(off0s), sub_off0s, [69 * xA], [5 * xA], 16, 9)
    Q, rowmap, n_rows = pieces[0][:3]
    used = rowmap[rowmap >= 0].long()
    Q[:, used, :16] = 1.5  # piece A now holds the whole window
    rows = torch.nonzero(wave_map >= 0).flatten()
    assembled[:, wave_map[rows].long()] = Q[:, rowmap[rows].long()]
    want = core.transform_contributions(assembled, 1, off0s, sub_off0s, rowmap=wave_map)
    for pcs in ([(Q, rowmap, n_rows, 0, M)], [(Q, rowmap, n_rows, 0, M), (*pieces[1][:3], 0, 0)],
                [(*pieces[1][:3], 496, 0), (Q, rowmap, n_rows, 0, M)]):
        got = core.transform_contributions_pieces(pcs, off0s, sub_off0s, torch.full_like(want, float("nan")))
        assert torch.equal(got, want)


def test_flat_send_buffer_layout():
    """the placed output form of wave_facet_side (g_layout) through the one launch"""
    import torch

    core, off0s, sub_off0s = small_problem()
    pieces, _, want = check_bits(core, torch.complex64, off0s, sub_off0s, [69 * xA], [5 * xA], 16, seed=6)
    F, S = len(off0s), len(sub_off0s)
    flat = torch.zeros(F * S * M * M + 64, dtype=torch.complex64, device=core.device)
    layout = ([64 + b * F * M * M for b in range(S)], [M * M] * S)  # subgrid-major: block (f, b) at 64 + (b*F + f) * m*m
    core.transform_contributions_pieces(pieces, off0s, sub_off0s, flat, g_layout=layout)
    assert torch.equal(flat[64:].view(S, F, M, M).transpose(0, 1), want) and not flat[:64].any()


def test_batch_loops_of_33_facets_and_65_subgrids():
    """more than kColZF = 32 facets and kColZB = 64 subgrids: four launches, each with the second source of ITS facets;
    the subgrids one offset step apart, so that they read 576 rows in all (blocks: 33 x 65 x 2 MiB)"""
    import torch

    core = core_of(W64, N64, xM64, yN64)
    fstep, sstep = core.facet_off_step, core.subgrid_off_step
    off0s = [(k - 16) * fstep for k in range(33)]
    sub_off0s = [k * sstep for k in range(65)]
    check_bits(core, torch.complex64, off0s, sub_off0s, [69 * xA], [5 * xA], 272, seed=7)


def test_one_launch_matches_the_oracle_primitives():
    """extract_from_facet(axis 0) and add_to_subgrid(axis 0) of the numpy reference on the assembled window, with the
    bound of test_hip_band_pipeline_gpu.py::test_transform_contributions_all_layouts (random data, float arithmetic)"""
    import torch

    core, off0s, sub_off0s = small_problem()
    ref = orc.OracleCore(W64, N64, xM64, yN64)
    _, assembled, got = check_bits(core, torch.complex64, off0s, sub_off0s, [69 * xA], [5 * xA], 272, seed=8)
    wave_map = core.subgrid_column_rows(sub_off0s)[0].cpu().numpy()
    got, assembled = got.cpu().numpy(), assembled.cpu().numpy()
    for f, off0 in enumerate(off0s):
        full = numpy.zeros((yN64, M), dtype=complex)
        full[wave_map >= 0] = assembled[f, wave_map[wave_map >= 0]]
        for b, sub_off0 in enumerate(sub_off0s):
            placed = ref.add_to_subgrid(ref.extract_from_facet(full, sub_off0, axis=0), off0, axis=0)
            want = placed[(numpy.arange(M) + xM64 // 2 - M // 2 + off0 * xM64 // N64) % xM64]
            rel = relrms(got[f, b], want)
            print(f"facet {f} subgrid {b}: relative RMSE vs oracle {rel:.3e}")
            assert rel < 2e-6, (f, b, rel)


@pytest.mark.parametrize("p", [16, 224])
def test_float64_column_arithmetic(p):
    """column_precision = 64 takes the slab path too: the 512-point float64 instance (32-column tiles, 16 points per lane)"""
    import torch

    core = core_of(W64, N64, xM64, yN64, precision=64)
    assert core.column_precision == 64
    fstep = core.facet_off_step
    check_bits(core, torch.complex64, [0, 0, -70 * fstep], [0, 2 * xA], [69 * xA], [5 * xA], p, seed=10)


@pytest.mark.parametrize("xM,p", [(256, 16), (256, 48), (256, 64), (256, 112), (512, 16), (512, 128), (512, 144)])
def test_instances_on_64_column_tiles(xM, p):
    """m = 128 and 256 (N = 2048, yN = 1024): the split inside the wave of a 64-column tile, and on a tile boundary"""
    import torch

    core = core_of(11.0, 2048, xM, 1024)
    m = core.xM_yN_size
    assert m == xM // 2
    fstep, sstep = core.facet_off_step, core.subgrid_off_step
    check_bits(core, torch.complex64, [0, 3 * fstep, -5 * fstep], [0, 7 * sstep], [300 * sstep], [-200 * sstep], p, seed=11)


@pytest.mark.parametrize("case", ["m64", "complex128"])
def test_a_case_without_an_instance_takes_one_launch_per_piece(case):
    """m = 64 (the configuration of smoke()) and complex128 storage have no two-source instance: same bits, no error"""
    import torch

    if case == "m64":
        core = core_of(11.0, 512, 128, 256)
        assert core.xM_yN_size == 64
        fstep, sstep = core.facet_off_step, core.subgrid_off_step
        check_bits(core, torch.complex64, [0, 3 * fstep], [0, 7 * sstep], [90 * sstep], [-60 * sstep], 16, seed=12)
    else:
        core, off0s, sub_off0s = small_problem()
        check_bits(core, torch.complex128, off0s, sub_off0s, [69 * xA], [5 * xA], 272, seed=13)
