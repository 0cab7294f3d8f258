"""CPU tests of the column-slab bookkeeping of forward K2 (ska_sdp_exec_swiftly_amd/slabs.py): which slab and which
positions a wave's window lies in, which slabs a plan touches, the slab row-map unions, and the figures of the default
64k-sparse plan."""
import numpy

from ska_sdp_exec_swiftly_amd import slabs

N, yN, m, xA = 65536, 32768, 512, 928


def _window_columns(off1):
    """padded-axis column of every position of the wave's Q (core.py:243-253 with the rotation of the column gather)"""
    s = off1 * yN // N
    cols = (yN // 2 - m // 2 + s + numpy.arange(m)) % yN
    pos = (cols - (yN // 2 - m // 2)) % m
    out = numpy.empty(m, dtype=int)
    out[pos] = cols
    return out


def _slab_columns(j):
    return (yN // 2 - m // 2 + j * m + numpy.arange(m)) % yN


def test_window_slab_and_pieces_hold_the_windows_columns_at_their_positions():
    for i1 in (0, 32, 3, 4, 5, 9, 70, 1, 12, 59):
        off1 = i1 * xA
        j, p = slabs.window_slab(N, yN, m, off1)
        s = off1 * yN // N
        assert (j, p) == ((s // m) % (yN // m), s % m) and p % 16 == 0
        want = _window_columns(off1)
        got = numpy.full(m, -1)
        pieces = slabs.wave_pieces(N, yN, m, off1)
        assert sum(count for _, _, count in pieces) == m and all(count > 0 for _, _, count in pieces)
        for slab, first, count in pieces:
            got[first:first + count] = _slab_columns(slab)[first:first + count]
        assert numpy.array_equal(got, want), i1
        assert len(pieces) == (1 if p == 0 else 2)
    assert slabs.window_slab(N, yN, m, 3 * xA) == (2, 368)
    assert slabs.window_slab(N, yN, m, 70 * xA) == (63, 224)  # s = 32480 = -288: the wrap across the cyclic axis
    assert slabs.wave_pieces(N, yN, m, 70 * xA) == [(63, 224, 288), (0, 0, 224)]
    # a slab is the Q of the pseudo-wave at slab_off1
    for j in (0, 5, 63):
        assert slabs.window_slab(N, yN, m, slabs.slab_off1(N, yN, m, j)) == (j, 0)
        assert numpy.array_equal(_window_columns(slabs.slab_off1(N, yN, m, j)), _slab_columns(j))


def test_supported():
    assert slabs.supported(N, yN, m, [i * xA for i in range(71)])
    assert not slabs.supported(N, yN, m, [2])  # s = 1: the window boundary is not on a 128-byte line
    assert not slabs.supported(N, 3 * 8192, m, [0])  # slab offsets would not be whole image offsets
    assert not slabs.supported(N, m, m, [0])  # a single slab
    assert slabs.supported(32768, 8192, 1024, [2048, 3 * 2048])


def test_plan_slabs_ranges_and_row_unions():
    plan = {0: (0, 2), 32: (0, 2), 3: (0, 2, 69), 4: (0, 2), 5: (0,), 9: (0, 2, 69), 70: (0, 2, 69), 1: (0, 2)}
    sp = slabs.SlabPlan(N, yN, m, [(i0 * xA, i1 * xA) for i1, i0s in plan.items() for i0 in i0s])
    # 0 / 1: slabs 0, 1; 3 / 4 / 5: slabs 2 .. 5; 9: 8, 9; 32: 29; 70: 63 and 0 -- the slabs between 5 and 9 are not touched
    assert sorted(sp.ranges) == [0, 1, 2, 3, 4, 5, 8, 9, 29, 63]
    full = [(0, m)]
    assert sp.ranges[0] == full and sp.ranges[3] == full and sp.ranges[4] == full and sp.ranges[29] == full
    assert sp.ranges[1] == [(0, 464)] and sp.ranges[2] == [(368, 144)] and sp.ranges[5] == [(0, 272)]
    assert sp.ranges[8] == [(80, 432)] and sp.ranges[9] == [(0, 80)] and sp.ranges[63] == [(224, 288)]
    # every planned window column is computed exactly once
    cols = numpy.concatenate([_slab_columns(j)[f:f + c] for j, r in sp.ranges.items() for f, c in r])
    want = numpy.unique(numpy.concatenate([_window_columns(i1 * xA) for i1 in plan]))
    assert cols.size == sp.columns() == want.size and numpy.array_equal(numpy.sort(cols), want)
    # row maps: the union over every planned wave that meets the slab
    rows = lambda i0s: [i * xA for i in i0s]
    assert sp.off0s[0] == rows((0, 2, 69))   # waves 0, 1 and the wrapped 70
    assert sp.off0s[1] == rows((0, 2))       # wave 1
    assert sp.off0s[3] == rows((0, 2, 69))   # waves 3 and 4
    assert sp.off0s[4] == rows((0, 2))       # waves 4 and 5
    assert sp.off0s[5] == rows((0,))         # wave 5
    assert sp.off0s[63] == rows((0, 2, 69))
    for i1, i0s in plan.items():
        for j, _, _ in sp.pieces(i1 * xA):
            assert set(rows(i0s)) <= set(sp.off0s[j])


def test_ranges_with_a_gap_stay_apart():
    """two waves that meet one slab from its two ends without touching: the gap is not computed"""
    sp = slabs.SlabPlan(N, yN, m, [(0, 1 * xA), (0, 3 * xA)])  # slab 1: [0, 464) of wave 1; slab 2: [0, ..) none, [368, 512)
    assert sp.ranges[1] == [(0, 464)] and sp.ranges[2] == [(368, 144)] and sp.ranges[3] == [(0, 368)]
    sp = slabs.SlabPlan(1024, 1024, 64, [(0, 16), (0, 96)])  # s = 16: [16, 64) + [0, 16); s = 96: slab 1 [32, 64), slab 2 [0, 32)
    assert sp.ranges == {0: [(16, 48)], 1: [(0, 16), (32, 32)], 2: [(0, 32)]}
    assert slabs._merge([(0, 16), (16, 16), (8, 4), (48, 16)]) == [(0, 32), (48, 16)]


def test_default_plan_of_the_64k_sparse_workload():
    """subgrid columns i1 in {0..12} + {59..70}: 23 slabs, 21 of them full, 272 and 448 columns at the two ends; 11 472
    columns per facet and pass instead of 25 x 512 = 12 800"""
    i1s = list(range(13)) + list(range(59, 71))
    sp = slabs.SlabPlan(N, yN, m, [(0, i1 * xA) for i1 in i1s])
    assert len(sp.ranges) == 23 and sp.columns() == 11472 and len(i1s) * m == 12800
    signed = sorted((j + 11) % 64 - 11 for j in sp.ranges)
    assert signed == list(range(-11, 12))
    partial = {j: r for j, r in sp.ranges.items() if r != [(0, m)]}
    assert partial == {53: [(240, 272)], 11: [(0, 448)]}
