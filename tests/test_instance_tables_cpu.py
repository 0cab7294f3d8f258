"""
The instance tables of the fused subgrid-side kernels stay in step (no GPU needed): ``SF_PAIRS`` and ``SF_PAIRS_C128`` of
csrc/sum_finish.hip, the pair tables of the instance sweep (tests/test_hip_instance_sweep_gpu.py), the Python-side gates
of ``SwiftlyCoreHip`` and the pairs named in the complex128 refusal message of csrc/swiftly_abi_pipeline.hip.  Adding an
instance without adding it to the sweep fails here.
"""
import inspect
import os
import re

import test_hip_instance_sweep_gpu as sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ska-sdp-distributed-fourier-transform_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name), encoding="utf-8") as fh:
        return fh.read()


def _macro_pairs(text, macro):
    """the ``X(a, b)`` entries of ``#define <macro>(X) ...`` (one logical line)"""
    found = re.findall(r"^#define\s+" + macro + r"\(X\)((?:\s*X\(\s*\d+\s*,\s*\d+\s*\))+)\s*$", text, flags=re.M)
    assert len(found) == 1, (macro, found)
    pairs = [(int(a), int(b)) for a, b in re.findall(r"X\(\s*(\d+)\s*,\s*(\d+)\s*\)", found[0])]
    assert pairs and len(set(pairs)) == len(pairs), (macro, pairs)
    return pairs


def test_sf_pairs_match_the_sweep_and_the_python_gates():
    from ska_sdp_exec_swiftly_amd.core_hip import SwiftlyCoreHip

    text = _read("sum_finish.hip")
    c64, c128 = _macro_pairs(text, "SF_PAIRS"), _macro_pairs(text, "SF_PAIRS_C128")
    assert set(c128) <= set(c64)  # (every entry point checks the complex64 table too)
    assert sorted(sweep.PAIRS) == sorted(c64)
    assert sorted(sweep.PAIRS_C128) == sorted(c128)
    assert sorted(SwiftlyCoreHip.C128_FUSED_PAIRS) == sorted(c128)
    # the sweep's cores have the sizes of their pair, with valid parameters
    for (logm, logx), p in sweep.PAIRS.items():
        assert p["xM"] == 1 << logx and p["xM"] * p["yN"] == (1 << logm) * p["N"]
        assert p["N"] % p["yN"] == 0 and p["N"] % p["xM"] == 0
    # the literal table in supports_fused_subgrid
    src = inspect.getsource(SwiftlyCoreHip.supports_fused_subgrid)
    lit = re.search(r"pairs = \{([^}]*)\}", src)
    assert lit is not None
    assert sorted((int(a), int(b)) for a, b in re.findall(r"\((\d+),\s*(\d+)\)", lit.group(1))) == sorted(c64)


def test_complex128_refusal_message_names_the_instances():
    c128 = _macro_pairs(_read("sum_finish.hip"), "SF_PAIRS_C128")
    text = _read("swiftly_abi_pipeline.hip")
    msg = re.search(r'instances exist for \(m, xM\) = ((?:\(\d+, \d+\)(?:, )?)+)"', text)
    assert msg is not None, "the complex128 refusal message of sum_finish_facets was not found"
    named = [(int(a), int(b)) for a, b in re.findall(r"\((\d+), (\d+)\)", msg.group(1))]
    assert sorted(named) == sorted((1 << a, 1 << b) for a, b in c128)
