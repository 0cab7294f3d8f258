"""
The instance tables of the fused subgrid-side kernels stay in step (no GPU needed): the capability table of the built
library (``swiftly_hip_supports``, csrc/swiftly_caps.h -- ``SF_PAIRS`` and ``SF_PAIRS_C128``, the tables the kernels of
csrc/sum_finish.hip are instantiated from), the pair tables of the instance sweep (tests/test_hip_instance_sweep_gpu.py)
and the pairs named in the complex128 refusal text.  Adding an instance without adding it to the sweep fails here.

The same for the facet side: the length lists of tests/test_hip_facet_sweep_gpu.py are what ``swiftly_hip_supports`` answers
over ``log2 yN = 0 .. 20``, so a gate widened later without a sweep entry fails here, on the CPU.
"""
import os
import re

import test_hip_facet_sweep_gpu as facets
import test_hip_instance_sweep_gpu as sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ska-sdp-distributed-fourier-transform_amd", "csrc")


def _macro_pairs(text, macro):
    """the ``X(a, b)`` entries of ``#define <macro>(X) ...`` (one logical line)"""
    found = re.findall(r"^#define\s+" + macro + r"\(X\)((?:\s*X\(\s*\d+\s*,\s*\d+\s*\))+)\s*$", text, flags=re.M)
    assert len(found) == 1, (macro, found)
    pairs = [(int(a), int(b)) for a, b in re.findall(r"X\(\s*(\d+)\s*,\s*(\d+)\s*\)", found[0])]
    assert pairs and len(set(pairs)) == len(pairs), (macro, pairs)
    return pairs


def test_sf_pairs_match_the_sweep_and_the_python_gates():
    from ska_sdp_exec_swiftly_amd import _lib

    c64 = sweep.library_pairs(_lib.FEATURE_FUSED_SUBGRID, _lib.C64)
    c128 = sweep.library_pairs(_lib.FEATURE_BAND_PIPELINE_EXPLICIT, _lib.C128)
    assert c128 <= c64  # (every entry point checks the complex64 table too)
    assert set(sweep.PAIRS) == c64
    assert set(sweep.PAIRS_C128) == c128
    # the sweep's cores have the sizes of their pair, with valid parameters
    for (logm, logx), p in sweep.PAIRS.items():
        assert p["xM"] == 1 << logx and p["xM"] * p["yN"] == (1 << logm) * p["N"]
        assert p["N"] % p["yN"] == 0 and p["N"] % p["xM"] == 0
    # the tables the kernels are instantiated from are the ones the library answers from
    with open(os.path.join(CSRC, "swiftly_caps.h"), encoding="utf-8") as fh:
        text = fh.read()
    assert set(_macro_pairs(text, "SF_PAIRS")) == c64 and set(_macro_pairs(text, "SF_PAIRS_C128")) == c128


def test_complex128_refusal_message_names_the_instances():
    from ska_sdp_exec_swiftly_amd import _lib

    c128 = sweep.library_pairs(_lib.FEATURE_BAND_PIPELINE_EXPLICIT, _lib.C128)
    assert (9, 11) not in c128  # (a complex64 instance without a complex128 one)
    assert not _lib.load().swiftly_hip_supports(_lib.FEATURE_BAND_PIPELINE_EXPLICIT, _lib.C128, 2048, 512, 2048, 0)
    why = _lib.last_error()
    assert "complex128" in why
    named = [(int(a), int(b)) for a, b in re.findall(r"\((\d+), (\d+)\)", why)]
    assert sorted(named) == sorted((1 << a, 1 << b) for a, b in c128)


def _accepted_lengths(feature, sizes_of):
    """log2 yN in 0 .. 20 the capability table accepts ``feature`` for in complex64, with the sizes ``sizes_of(L)``"""
    from ska_sdp_exec_swiftly_amd import _lib

    found = []
    for L in range(21):
        p = sizes_of(L)
        if p is not None and _lib.load().swiftly_hip_supports(getattr(_lib, "FEATURE_" + feature), _lib.C64, p["N"], p["yN"],
                                                              p["xM"], 0):
            found.append(L)
    return found


def test_facet_sweep_lengths_are_what_the_gates_accept():
    from ska_sdp_exec_swiftly_amd import _lib

    # the sweep's own cores: m = 128, xM = 256 (m = 64, xM = 128 at yN = 64); below that the smallest valid m
    def sweep_core(L):
        return facets.params(L) if L >= 6 else dict(N=2 << L, xM=2 << L, yN=1 << L)

    assert _accepted_lengths("BACKWARD_BAND", sweep_core) == facets.LENGTHS
    assert _accepted_lengths("BAND_PIPELINE", sweep_core) == facets.K1_LENGTHS
    assert _accepted_lengths("SPLIT_BAND", sweep_core) == facets.SPLIT_LENGTHS
    # ... and with any other (m, xM): the backward band does not depend on the pair, the forward one needs an instance
    for logm, logx in ((0, 0), (5, 5), (9, 10)):
        assert _accepted_lengths("BACKWARD_BAND", lambda L: dict(N=(1 << logx << L) >> logm, xM=1 << logx, yN=1 << L)
                                 if L >= logm else None) == [L for L in facets.LENGTHS if L >= logm]
    assert _accepted_lengths("BAND_PIPELINE", lambda L: dict(N=(1 << 10 << L) >> 9, xM=1 << 10, yN=1 << L) if L >= 9 else None) \
        == [L for L in facets.K1_LENGTHS if L >= 9]
    # the boundaries the GPU test walks are the ends of these lists
    assert facets.GATE_EDGES == {
        "BACKWARD_BAND": (facets.LENGTHS[0] - 1, facets.LENGTHS[0], facets.LENGTHS[-1], facets.LENGTHS[-1] + 1),
        "BAND_PIPELINE": (facets.K1_LENGTHS[0] - 1, facets.K1_LENGTHS[0], facets.K1_LENGTHS[-1], facets.K1_LENGTHS[-1] + 1),
    }
    for feature, edges in facets.MIXED_EDGES.items():
        ks = [k for k in range(21) if _lib.load().swiftly_hip_supports(
            getattr(_lib, "FEATURE_" + feature), _lib.C64, *(lambda p: (p["N"], p["yN"], p["xM"]))(
                facets._sizes(min(k, 6 if feature == "BACKWARD_BAND" else 7), 8, 3 << k)), 0)]
        assert [e[0] for e in edges] == [ks[0] - 1, ks[0], ks[-1], ks[-1] + 1], (feature, ks)
    # finish_axis1_rows: one sweep case per m of the fused pairs, each at a split-band length with an instance for its pair
    c64 = sweep.library_pairs(_lib.FEATURE_FUSED_SUBGRID, _lib.C64)
    assert {c[0] for c in facets.AXIS1_CASES} == {pair[0] for pair in c64}
    assert all((logm, logx) in c64 and L in facets.SPLIT_LENGTHS for logm, logx, L in facets.AXIS1_CASES)
    # the float64 column passes the sweep expects: 2^5 .. 2^9 points (col_pass_f64_supported through the complex128 gate,
    # whose m-point pass is one of them)
    c128 = sweep.library_pairs(_lib.FEATURE_BAND_PIPELINE_EXPLICIT, _lib.C128)
    assert max(pair[0] for pair in c128) == 9
    assert [L for L in facets.LENGTHS if not facets.k2_has_f64(L)] == [10]
    assert [L for L in facets.LENGTHS if not facets.acc_has_f64(L)] == [9]
