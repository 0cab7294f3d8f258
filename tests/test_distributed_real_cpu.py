"""
Real-valued facets in the multi-GPU classes and in ``DeviceSources`` without a device: the argument errors of
``DistributedForward(..., facet_dtype=, half_length_k1=)`` and ``DistributedBackward(..., facet_dtype=, half_length_finish=)``
(the texts of ``SwiftlyForward`` / ``SwiftlyBackward``, raised before the constructors touch a configuration), and the two
real-valued point-source entry points in the header, the library and the binding.
"""
import os
import re

import pytest
import torch

from ska_sdp_exec_swiftly_amd import _lib
from ska_sdp_exec_swiftly_amd.distributed import DistributedBackward, DistributedForward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("swiftly_hip_facet_from_sources_real", "swiftly_hip_check_facet_from_sources_real")


def test_forward_facet_dtype_must_be_float32():
    # (no configuration, no facets, no device: the refusal comes first)
    for bad in (torch.complex64, torch.float64, "complex64", 7):
        with pytest.raises(ValueError, match="facet_dtype must be float32 or None"):
            DistributedForward(None, [], [], facet_dtype=bad)
    with pytest.raises(ValueError, match="facet_dtype must be float32 or None"):
        DistributedForward(None, [], [], facet_dtype=torch.complex64, half_length_k1=True)


def test_forward_half_length_needs_float32_facets():
    with pytest.raises(ValueError, match="half_length_k1=True needs facet_dtype=float32"):
        DistributedForward(None, [], [], half_length_k1=True)
    # with float32 facets the keywords get past the parsing: the constructor then fails on the missing configuration
    for kw in (dict(facet_dtype=torch.float32), dict(facet_dtype="float32", half_length_k1=True), {}):
        with pytest.raises(AttributeError):
            DistributedForward(None, [], [], rank_world=(0, 2), **kw)


def test_backward_half_length_needs_float32_facets():
    for bad in (None, torch.complex64, torch.float64):
        with pytest.raises(ValueError, match="half_length_finish=True needs facet_dtype=float32"):
            DistributedBackward(None, [], half_length_finish=True, facet_dtype=bad)
    with pytest.raises(ValueError, match="facet_dtype must be float32, float64, complex64, complex128 or None"):
        DistributedBackward(None, [], facet_dtype=torch.float16)


def test_backward_facet_dtype_must_match_the_data():
    for facet_dtype, dtype in ((torch.float32, torch.complex128), (torch.float64, torch.complex64), (torch.float64, None),
                               (torch.complex64, torch.complex128)):
        with pytest.raises(ValueError, match="does not match"):
            DistributedBackward(None, [], facet_dtype=facet_dtype, dtype=dtype)
    # a matching pair gets past the parsing: the constructor then fails on the missing configuration
    for kw in (dict(facet_dtype=torch.float32), dict(facet_dtype=torch.float32, half_length_finish=True),
               dict(facet_dtype=torch.float64, dtype=torch.complex128), {}):
        with pytest.raises(AttributeError):
            DistributedBackward(None, [], rank_world=(0, 2), **kw)


@pytest.mark.parametrize("symbol", ENTRY_POINTS)
def test_real_source_entry_points_are_in_the_header_exported_and_bound(symbol):
    header = open(os.path.join(ROOT, "include", "swiftly_hip.h"), encoding="utf-8").read()
    assert re.search(r"\bint " + symbol + r"\(int dtype, const void\* sources, int64_t n_sources,", header)
    lib = _lib.load()
    fn = getattr(lib, symbol)  # AttributeError: not exported
    twin = getattr(lib, symbol[: -len("_real")])
    assert fn.argtypes is not None and list(fn.argtypes) == list(twin.argtypes) and fn.restype is twin.restype
