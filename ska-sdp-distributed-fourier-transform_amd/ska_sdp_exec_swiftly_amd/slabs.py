"""
Column slabs of the padded facet axis for K2 of the contiguous-axis-first forward pipeline: pure
bookkeeping, no device work.

``Q`` of a wave keeps window column ``c`` of the padded axis at position ``(c - base) mod m`` with ``base = yN/2 - m/2``,
whatever the wave.  The cyclic axis is therefore cut into ``yN / m`` slabs: slab ``j`` holds the columns ``(base + j*m +
[0, m)) mod yN`` at positions ``0 .. m-1`` and is exactly the ``Q`` of a pseudo-wave with ``s = j*m``, i.e. ``off1 =
j*m*N/yN``.  A real wave with ``s = off1*yN // N`` and ``p = s mod m`` finds the positions ``[p, m)`` of its window in
slab ``s // m`` and the positions ``[0, p)`` in the next one; neighbouring waves, whose windows overlap, share slabs, so
that no band column goes through K2 twice.
"""


def supported(N, yN, m, off1s):
    """can the windows of these waves be served from slabs?  (whole slabs on the axis, slab offsets that are whole
    image offsets, and every window boundary on a 16-column = 128-byte line)"""
    N, yN, m = int(N), int(yN), int(m)
    if m <= 0 or yN % m or yN // m < 2 or (m * N) % yN or m % 16:
        return False
    return all((int(o) * yN // N) % m % 16 == 0 for o in off1s)


def window_slab(N, yN, m, off1):
    """``(j, p)`` of the window of wave ``off1``: positions ``[p, m)`` in slab ``j``, ``[0, p)`` in slab ``j + 1``"""
    s = int(off1) * int(yN) // int(N)
    return (s // m) % (yN // m), s % m


def slab_off1(N, yN, m, j):
    """the ``off1`` of the pseudo-wave whose ``Q`` is slab ``j``"""
    return int(j) * int(m) * int(N) // int(yN)


def wave_pieces(N, yN, m, off1):
    """``[(slab, first position, number of positions)]`` of the window of wave ``off1``, empty pieces dropped"""
    j, p = window_slab(N, yN, m, off1)
    pieces = [(j, p, m - p), ((j + 1) % (yN // m), 0, p)]
    return [pc for pc in pieces if pc[2] > 0]


def _merge(ranges):
    """sorted, disjoint ``(first, count)`` ranges covering the same positions (touching ranges joined)"""
    out = []
    for first, count in sorted(ranges):
        if out and first <= out[-1][0] + out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], first + count - out[-1][0]))
        else:
            out.append((first, count))
    return out


class SlabPlan:
    """What a plan of waves needs of every slab.

    ``ranges``: ``{slab: [(first position, number of positions)]}`` -- the positions some planned window reads, as
    disjoint ranges (a full slab: ``[(0, m)]``; the slabs at the two ends of the band are partial).
    ``off0s``: ``{slab: sorted off0 of every planned subgrid of every planned wave whose window meets the slab}`` --
    the slab's row map is the row map of that union, a superset of the rows each of those waves reads.
    ``users``: ``{slab: off1 of the planned waves whose window meets it}``."""

    def __init__(self, N, yN, m, plan):
        """``plan``: iterable of ``(off0, off1)`` of the planned subgrids"""
        self.N, self.yN, self.m = int(N), int(yN), int(m)
        by_wave = {}
        for off0, off1 in plan:
            by_wave.setdefault(int(off1), set()).add(int(off0))
        ranges, off0s, users = {}, {}, {}
        for off1 in sorted(by_wave):
            for j, first, count in wave_pieces(N, yN, m, off1):
                ranges.setdefault(j, []).append((first, count))
                off0s.setdefault(j, set()).update(by_wave[off1])
                users.setdefault(j, []).append(off1)
        self.users = users
        self.ranges = {j: _merge(r) for j, r in ranges.items()}
        self.off0s = {j: sorted(v) for j, v in off0s.items()}

    def pieces(self, off1):
        """:py:func:`wave_pieces` of wave ``off1``"""
        return wave_pieces(self.N, self.yN, self.m, off1)

    def off1(self, j):
        """:py:func:`slab_off1` of slab ``j``"""
        return slab_off1(self.N, self.yN, self.m, j)

    def columns(self):
        """band columns K2 transforms per facet and pass when every slab is computed once"""
        return sum(count for r in self.ranges.values() for _, count in r)
