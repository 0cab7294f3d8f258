"""
The persistent form of the column kernel group_finish (csrc/swiftly_groupfinish.h: group_finish_kernel_persistent; switch
swiftly_hip_group_finish_persistent) against the one-workgroup-per-tile form: the same tiles, walked by fewer workgroups
with the next tile's first facet requested early, must give the same bits.

What can go wrong is the walk and what is carried from one tile to the next, so the inputs are the small problems of
test_hip_group_finish_gpu.py (imported, not copied): two subgrids whose crops wrap, four facets in two groups of one and
three facets (the early request crosses a change of facet count), both masks, one and two pieces with different row maps
and NaN where a piece holds no column: 32 tiles at (m, xM) = (128, 256), 128 at (512, 1024).  Grids capped at 2, 3, 5 and
7 workgroups make every workgroup walk many tiles -- 3, 5 and 7 do not divide the tile count, so some workgroups do one
tile more, and consecutive tiles of a workgroup cross the piece boundary, a subgrid change and a group change; at 1 (one
workgroup per compute unit) the grid reaches the tile count and every workgroup does one tile.  (A cap of ONE workgroup
cannot be asked for: 1 is the value that selects the compute-unit count.)

The oracle-facing bounds are those of test_hip_group_finish_gpu.py and test_hip_group_finish_consistency_gpu.py, which run
whatever form is the default.
"""
import pytest

from test_hip_group_finish_gpu import CASES, pieces, problem, run  # noqa: F401  (pieces: part of the shared fixture)

pytestmark = pytest.mark.gpu

CAPS = (2, 3, 5, 7)


def tiles(d):
    return ((d["m"] + 15) // 16) * len(d["subs"]) * len(d["groups"])


def one_run(d, n_pieces, stages, setting):
    """(rows of T the kernel writes, final output or None, grid of the launch) with the switch at ``setting``"""
    import torch

    from ska_sdp_exec_swiftly_amd import _lib

    lib = _lib.load()
    lib.swiftly_hip_group_finish_persistent(setting)
    G, S = len(d["groups"]), len(d["subs"])
    t_work = torch.full((G, S, d["xM"], d["m"]), float("nan"), dtype=torch.complex64, device="cuda")  # unwritten shows
    out = run(d, n_pieces, stages, t_work=t_work.view(-1))
    torch.cuda.synchronize()
    return t_work[:, :, : d["xA"]].clone(), (out.clone() if stages == 3 else None), lib.swiftly_hip_group_finish_persistent(-2)


@pytest.mark.parametrize("stages", [1, 3])
@pytest.mark.parametrize("n_pieces", [1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_persistent_walk_gives_the_bits_of_one_workgroup_per_tile(name, n_pieces, stages):
    import torch

    from ska_sdp_exec_swiftly_amd import _lib

    d = problem(name)
    lib = _lib.load()
    old = lib.swiftly_hip_group_finish_persistent(-1)
    try:
        T0, out0, grid0 = one_run(d, n_pieces, stages, 0)
        assert grid0 == 0  # the one-workgroup-per-tile kernel ran
        assert not torch.isnan(T0.real).any() and not torch.isnan(T0.imag).any()
        cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
        for setting in CAPS + (1,):
            T, out, grid = one_run(d, n_pieces, stages, setting)
            assert grid == min(tiles(d), cus if setting == 1 else setting), (setting, grid)  # the persistent kernel, that grid
            assert torch.equal(T, T0), (name, n_pieces, stages, setting)
            if stages == 3:
                assert torch.equal(out, out0), (name, n_pieces, stages, setting)
    finally:
        lib.swiftly_hip_group_finish_persistent(old)


def test_switch_selects_the_kernel():
    """the setting is process-wide, returned by the setter and by the query; the launch record follows it: 0 = one workgroup
    per tile, else the persistent grid -- a launcher that fell back to one form would pass every equality above"""
    from ska_sdp_exec_swiftly_amd import _lib

    d = problem("128-256")
    lib = _lib.load()
    old = lib.swiftly_hip_group_finish_persistent(-1)
    try:
        assert lib.swiftly_hip_group_finish_persistent(5) == old
        assert lib.swiftly_hip_group_finish_persistent(-1) == 5
        assert one_run(d, 1, 1, 5)[2] == 5
        assert one_run(d, 1, 1, 0)[2] == 0
        assert lib.swiftly_hip_group_finish_persistent(-1) == 0
        assert one_run(d, 1, 1, 1)[2] == tiles(d) == 32  # fewer tiles than compute units: one tile per workgroup
    finally:
        lib.swiftly_hip_group_finish_persistent(old)
