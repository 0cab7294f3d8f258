"""Host side of the device point-source truths (ska_sdp_exec_swiftly_amd/device_sources.py): the normalised source
table the kernels assume (coordinates reduced, one record per pixel), the per-row lists of the facet check, and the
declarations of the four entry points (tests/test_abi_symbols.py then checks that they are exported).  No GPU."""
import os
import re

import numpy
import pytest

from oracle import swiftly_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def table_of(sources, N):
    from ska_sdp_exec_swiftly_amd.device_sources import source_table

    return source_table(sources, N)


def as_dict(table):
    return {(int(r["c0"]), int(r["c1"])): complex(r["re"], r["im"]) for r in table}


def test_record_layout():
    from ska_sdp_exec_swiftly_amd.device_sources import SOURCE_DTYPE

    assert SOURCE_DTYPE.itemsize == 24
    assert [SOURCE_DTYPE.fields[n][1] for n in ("re", "im", "c0", "c1")] == [0, 8, 16, 20]
    text = open(os.path.join(ROOT, "ska-sdp-distributed-fourier-transform_amd", "csrc", "swiftly_sources.h")).read()
    assert re.search(r"struct SourceRec \{\s*double re, im;[^\n]*\n\s*int32_t c0, c1;", text)


def test_wraps_coordinates():
    N = 1024
    t = table_of([(1, 512, -513), (2, -512 - 1024, 511 + 3 * 1024), (3, 0, 2048 + 5), (4, 511, -512)], N)
    # +N/2 wraps to -N/2, -N/2 - 1 to N/2 - 1; anything beyond N comes back by whole periods
    assert as_dict(t) == {(-512, 511): 3 + 0j, (0, 5): 3 + 0j, (511, -512): 4 + 0j}
    assert t["c0"].min() >= -N // 2 and t["c0"].max() < N // 2 and t["c1"].min() >= -N // 2 and t["c1"].max() < N // 2


def test_merges_duplicates_in_order():
    t = table_of([(1, 3, 4), (0.25, 7, 7), (2.5, 3, 4), (1j, 3 - 64, 4 + 128)], 64)
    assert len(t) == 2
    assert as_dict(t) == {(3, 4): 3.5 + 1j, (7, 7): 0.25 + 0j}
    assert [int(c) for c in t["c0"]] == [3, 7]  # first appearance keeps its place


def test_keeps_complex_intensities():
    t = table_of([(1.5 - 2j, 1, 2), (numpy.complex128(3j), -1, -2), (numpy.float32(0.5), 5, 5)], 32)
    assert as_dict(t) == {(1, 2): 1.5 - 2j, (-1, -2): 3j, (5, 5): 0.5 + 0j}
    assert t.dtype["re"] == numpy.float64 and t.dtype["c0"] == numpy.int32


def test_integer_valued_floats_and_numpy_integers_are_coordinates():
    assert as_dict(table_of([(1, 3.0, numpy.int64(-2))], 16)) == {(3, -2): 1 + 0j}


@pytest.mark.parametrize("bad", [[(1, 0.5, 0)], [(1, 0, 1e-9)], [(1, 3)], [(1, 1, 2, 3)]])
def test_refuses_what_a_facet_cannot_hold(bad):
    with pytest.raises(ValueError):
        table_of(bad, 64)


def test_refuses_image_sizes_beyond_the_integer_phase():
    with pytest.raises(ValueError):
        table_of([(1, 0, 0)], 2**31 + 1)
    assert len(table_of([(1, 2**30, -(2**30))], 2**31)) == 1
    assert len(table_of([], 64)) == 0


def test_row_lists_match_the_oracle_facet():
    """the per-row lists name exactly the pixels the oracle's facet holds, ascending in their column"""
    from ska_sdp_exec_swiftly_amd.device_sources import facet_row_lists

    N, size, off0, off1 = 256, 45, -60, 256 + 31
    rng = numpy.random.default_rng(3)
    sources = [(1 + k, int(a), int(b)) for k, (a, b) in enumerate(rng.integers(-N // 2, N // 2, size=(400, 2)))]
    sources += [(9, off0 - size // 2, off1 - size // 2), (7, off0 - size // 2 + size - 1, off1 - size // 2 + size - 1 - N)]
    t = table_of(sources, N)
    start, srcs = facet_row_lists(t, N, size, off0, off1)
    want = orc.make_facet_from_sources(sources, N, size, [off0, off1])
    got = numpy.zeros((size, size), dtype=complex)
    assert start[0] == 0 and start[-1] == len(srcs) == numpy.count_nonzero(want)
    for r in range(size):
        cols = []
        for s in srcs[start[r]:start[r + 1]]:
            assert (int(t["c0"][s]) - (off0 - size // 2)) % N == r
            cols.append((int(t["c1"][s]) - (off1 - size // 2)) % N)
            got[r, cols[-1]] = complex(t["re"][s], t["im"][s])
        assert cols == sorted(cols)
    assert numpy.array_equal(got, want)


def test_entry_points_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "swiftly_hip.h")).read()
    names = ["swiftly_hip_subgrids_from_sources", "swiftly_hip_check_subgrids_from_sources",
             "swiftly_hip_facet_from_sources", "swiftly_hip_check_facet_from_sources"]
    from ska_sdp_exec_swiftly_amd import _lib

    lib = _lib.load()
    for name in names:
        assert re.search(r"\bint " + name + r"\s*\(", text), name
        assert getattr(lib, name).argtypes is not None, name


def test_entry_points_refuse_bad_parameters_before_any_device_work():
    import ctypes

    from ska_sdp_exec_swiftly_amd import _lib

    lib = _lib.load()
    off = (ctypes.c_int64 * 1)(0)
    sub = lib.swiftly_hip_subgrids_from_sources
    assert sub(_lib.C128, None, 0, 2**31 + 1, 4, off, off, 1, None, None, None, 0, 4, None) == _lib.ERR_PARAM
    assert sub(7, None, 0, 1024, 4, off, off, 1, None, None, None, 0, 4, None) == _lib.ERR_PARAM
    assert sub(_lib.C128, None, 0, 1024, 0, off, off, 1, None, None, None, 0, 4, None) == _lib.ERR_PARAM
    assert sub(_lib.C128, None, 0, 1024, 4, off, off, 1, None, None, None, 0, 4, None) == _lib.ERR_PARAM  # null out
    assert sub(_lib.C128, None, 3, 1024, 4, off, off, 1, None, None, None, 0, 4, None) == _lib.ERR_PARAM  # null table
    chk = lib.swiftly_hip_check_subgrids_from_sources
    assert chk(_lib.C64, None, 0, 1024, 4, off, off, 1, None, None, None, 0, 4, None, None) == _lib.ERR_PARAM
    assert lib.swiftly_hip_facet_from_sources(_lib.C64, None, 0, 0, 4, 0, 0, None, None, None, 4, None) == _lib.ERR_PARAM
    assert lib.swiftly_hip_check_facet_from_sources(
        _lib.C64, None, 0, 1024, 4, 0, 0, None, None, None, 4, None, None, None, None) == _lib.ERR_PARAM


def test_package_exports_device_sources():
    import ska_sdp_exec_swiftly_amd as sw

    assert "DeviceSources" in sw.__all__ and sw.DeviceSources.__module__.endswith("device_sources")
