"""
The instance tables of the fused subgrid-side kernels stay in step (no GPU needed): the capability table of the built
library (``swiftly_hip_supports``, csrc/swiftly_caps.h -- ``SF_PAIRS`` and ``SF_PAIRS_C128``, the tables the kernels of
csrc/sum_finish.hip are instantiated from), the pair tables of the instance sweep (tests/test_hip_instance_sweep_gpu.py)
and the pairs named in the complex128 refusal text.  Adding an instance without adding it to the sweep fails here.
"""
import os
import re

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
