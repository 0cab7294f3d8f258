"""
The offset-to-index-map geometry of the native library (csrc/swiftly_geometry.h) against the oracle's closed forms, without
a GPU: ``tests/native/geometry_dump.cpp`` includes only that header and ``swiftly_caps.h`` and prints what each function
returns; this test compiles it with the compiler of the library's host code and compares.

Expectations come from ``oracle/swiftly_oracle.py`` alone.  The oracle's primitives run here with the centred transforms
replaced by the identity and the windows by ones, on index-carrying data, so what they return IS their scatter / gather
index array (``pos`` / ``src`` of prepare_facet, extract_from_facet, add_to_subgrid, finish_subgrid, prepare_subgrid,
extract_from_subgrid, add_to_facet, finish_facet) together with ``_s`` and ``_sp``.  A native map ``(a, len, c, mod)`` is
evaluated with the AxisMap rule of csrc/swiftly_rows.h -- ``q = (ci + a) mod n``, valid iff ``q < len``,
``idx = (q + c) mod mod`` -- for every centred index ``ci`` of its transform length ``n``.
"""
import os
import re
import subprocess

import numpy
import pytest

from oracle import swiftly_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ska-sdp-distributed-fourier-transform_amd", "csrc")

#: (N, yN, xM), facet sizes, subgrid sizes (both parities; the benchmark's own sizes first)
CASES = [
    ((1024, 512, 256), (416, 417), (228, 229)),  # reference test parameters
    ((8192, 2048, 2048), (1408, 1409), (1792, 1793)),
    ((65536, 32768, 1024), (22528, 22527), (928, 927)),  # the benchmark's sizes
    ((12288, 6144, 512), (4096, 4097), (448, 449)),  # yN = 3 * 2^11: m is a power of two, yN is not
]


def offsets(N, step):
    """0, +-one step, N -+ one step, and two offsets that are no multiples of the step (they pin floordiv to ``//``)"""
    odd = [7 * step + 1, -(5 * step + 1)]
    assert all(o % step for o in odd)
    return [0, step, -step, N - step, N + step] + odd


def all_offsets(N, yN, xM):
    """facet steps (N / xM), subgrid steps (N / yN), and N / 2: a window that crosses the end of the padded axis"""
    return sorted(set(offsets(N, N // xM) + offsets(N, N // yN) + [N // 2]))


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """the compiled program as a function: list of request lines -> list of answer lines"""
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC\s*\?=\s*(\S+)", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1)
    exe = str(tmp_path_factory.mktemp("geometry") / "geometry_dump")
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "native", "geometry_dump.cpp"),
                    "-o", exe], check=True, timeout=300)

    def run(requests):
        res = subprocess.run([exe], input="\n".join(requests) + "\n", stdout=subprocess.PIPE, text=True, check=True, timeout=120)
        return res.stdout.splitlines()

    return run


@pytest.fixture
def oracle_indices(monkeypatch):
    """OracleCore whose transforms are the identity and whose windows are ones: the primitives return their index arrays"""
    monkeypatch.setattr(orc, "cfft", lambda a, axis: a)
    monkeypatch.setattr(orc, "cifft", lambda a, axis: a)

    def make(N, yN, xM):
        core = object.__new__(orc.OracleCore)  # (no PSWF evaluation: only the sizes matter here)
        core.N, core.yN_size, core.xM_size, core.xM_yN_size = N, yN, xM, xM * yN // N
        core.pswf = numpy.ones(yN)
        core.Fn = numpy.ones(core.xM_yN_size)
        return core

    return make


def evaluate(m, n):
    """the AxisMap rule for every centred index of an n-point transform: (valid, idx)"""
    a, length, c, mod = m
    q = (numpy.arange(n) + a) % n
    return q < length, (q + c) % mod


def check_scatter(m, n, placed):
    """`placed`: what an oracle scatter of 1, 2, ... leaves in the n centred positions (0 = nothing)"""
    valid, idx = evaluate(m, n)
    assert numpy.array_equal(valid, placed != 0)
    assert numpy.array_equal(idx[valid], placed[valid].astype(int) - 1)


def check_gather(m, n, src):
    """`src`: the centred index an oracle gather reads for each memory index"""
    valid, idx = evaluate(m, n)
    assert valid.sum() == len(src) and valid[src].all()
    assert numpy.array_equal(idx[src], numpy.arange(len(src)))


def ints(line):
    return [int(x) for x in line.split()]


@pytest.mark.parametrize("sizes,yBs,xAs", CASES, ids=lambda v: "-".join(map(str, v)))
def test_maps_against_the_oracle(dump, oracle_indices, sizes, yBs, xAs):
    N, yN, xM = sizes
    m = xM * yN // N
    core = oracle_indices(N, yN, xM)
    cases = [(yB, xA, off) for yB, xA in zip(yBs, xAs) for off in all_offsets(N, yN, xM)]
    answers = dump([f"maps {N} {yN} {xM} {yB} {xA} {off}" for yB, xA, off in cases])
    assert len(answers) == len(cases)
    for (yB, xA, off), line in zip(cases, answers):
        v = ints(line)
        lo, facet, contrib, (sp, start), subgrid = v[0], v[1:5], v[5:9], v[9:11], v[11:15]
        # the facet in the padded facet: prepare_facet scatters, finish_facet gathers; lo from facet_window
        ramp = object.__new__(orc.OracleCore)
        ramp.yN_size, ramp.pswf = yN, numpy.arange(1.0, yN + 1)
        assert lo == round(1.0 / ramp.facet_window(yB)[0]) - 1
        check_scatter(facet, yN, core.prepare_facet(numpy.arange(1.0, yB + 1), off, 0).real)
        check_gather(facet, yN, core.finish_facet(numpy.arange(yN), off, yB, 0).astype(int))
        # the contribution in the padded subgrid: add_to_subgrid scatters element (k + sp) mod m, extract_from_subgrid
        # gathers into it
        assert sp == core._sp(off)
        valid, idx = evaluate(contrib, m)
        assert valid.all()
        res = core.add_to_subgrid(numpy.arange(1.0, m + 1), off, 0)
        assert numpy.count_nonzero(res) == m and numpy.array_equal(res[idx], numpy.arange(1.0, m + 1))
        assert numpy.array_equal(core.extract_from_subgrid(numpy.arange(xM), off, 0).astype(int), idx)
        assert start == idx[(0 - contrib[0]) % m] == contrib[2]  # where element q = 0 lands
        # the subgrid in the padded subgrid: prepare_subgrid scatters, finish_subgrid gathers
        check_scatter(subgrid, xM, core.prepare_subgrid(numpy.arange(1.0, xA + 1), off).real)
        check_gather(subgrid, xM, core.finish_subgrid(numpy.arange(xM), off, xA).astype(int))


def in_band(cols, yN, start, length):
    return (cols - start) % yN < length


@pytest.mark.parametrize("sizes", [c[0] for c in CASES], ids=lambda v: "-".join(map(str, v)))
def test_window_and_bands_against_the_oracle(dump, oracle_indices, sizes):
    N, yN, xM = sizes
    m = xM * yN // N
    core = oracle_indices(N, yN, xM)
    offs = all_offsets(N, yN, xM)
    answers = dump([f"window {N} {yN} {xM} {off}" for off in offs])
    assert len(answers) == 2 * len(offs)
    ranges = [(0, m), (0, 16), (16, 32), (m - 16, 16), (m // 2, m // 4)]
    requests, expected = [], []
    for i, off in enumerate(offs):
        s, rot, base = ints(answers[2 * i])
        cols = numpy.array(ints(answers[2 * i + 1]))
        # extract_from_facet gathers position q from src[q]; add_to_facet scatters it back there
        src = core.extract_from_facet(numpy.arange(yN), off, 0)
        assert s == core._s(off) and rot == (-s) % m
        assert numpy.array_equal(cols, src)
        assert base == src[s % m]  # (the position with (q + rot) mod m = 0)
        back = core.add_to_facet(numpy.arange(1.0, m + 1), off, 0)
        assert numpy.count_nonzero(back) == m and numpy.array_equal(back[cols], numpy.arange(1.0, m + 1))
        # bands around the window [c0, c0 + m): it ends exactly at the window's last column / is one column short / starts
        # one column late / wraps over the end of the padded axis / is the window itself
        c0 = int(base)
        bands = [((c0 - 3) % yN, m + 3), ((c0 - 3) % yN, m + 2), ((c0 + 1) % yN, m + 7), (yN - m // 4, m), (yN - m // 4, m // 4 + c0 + m),
                 (c0, m)]
        for start, length in bands:
            # shorter than the axis: only then is membership of every column the same as the range test asserted below (a
            # band of all yN columns holds a window that crosses its start too: test_whole_axis_band_holds_every_window)
            length = min(length, yN - 1)
            for first, count in ranges:
                requests.append(f"inband {N} {yN} {xM} {off} {first} {count} {start} {length}")
                outside = numpy.flatnonzero(~in_band(cols[first : first + count], yN, start, length))
                want = first + int(outside[0]) if len(outside) else -1
                if (first, count) == (0, m):  # the range test of the whole window
                    assert (want == -1) == ((c0 - start) % yN + m <= length)
                expected.append(want)
    got = [int(x) for x in dump(requests)]
    assert got == expected
    assert -1 in expected and any(e >= 0 for e in expected)


def test_band_maps_and_offset_predicate(dump):
    N, yN, xM = 1024, 512, 256
    bands = [(0, yN), (0, 1), (yN - 1, yN), (100, 300), (500, 40), (511, 1)]
    bad = [(0, 0), (0, yN + 1), (-1, 10), (yN, 10)]
    answers = dump([f"bandmap {N} {yN} {xM} {s} {n}" for s, n in bands + bad])
    for (start, length), line in zip(bands, answers):
        v = ints(line)
        assert v[0] == 1
        # element d of a band row is column (start + d) mod yN of the padded axis
        valid, idx = evaluate(v[1:5], yN)
        d = (numpy.arange(yN) - start) % yN
        assert numpy.array_equal(valid, d < length) and numpy.array_equal(idx[valid], d[valid])
    assert [ints(line)[0] for line in answers[len(bands):]] == [0] * len(bad)
    fits = [(65536, 65535, 0, 1), (65536, 65536, 0, 0), (65535, 65536, 65535, 1), (65535, 65536, 65536, 0), (1, 1 << 32, 0, 0),
            (22528, 190651, 0, 0), (22528, 190650, 0, 1)]
    assert [int(x) for x in dump([f"fits {c} {s} {e}" for c, s, e, _ in fits])] == [want for *_, want in fits]


def test_whole_axis_band_holds_every_window(dump):
    """The one case where membership and the range test differ: a band of all yN columns holds every column, also those of
    a window that crosses the band's start, where ``(c0 - band_start) mod yN + m`` exceeds ``band_len``.  window_in_band is
    membership (the kernels map each column through the band on its own), so it accepts."""
    N, yN, xM = 65536, 32768, 1024
    m = xM * yN // N
    c0 = int(dump([f"window {N} {yN} {xM} {N // 2}"])[0].split()[2])
    assert c0 + m > yN  # the window crosses the end of the padded axis
    assert dump([f"inband {N} {yN} {xM} {N // 2} 0 {m} 0 {yN}", f"inband {N} {yN} {xM} {N // 2} 0 {m} 0 {yN - 1}"]) == ["-1", str(yN - 1 - c0)]
