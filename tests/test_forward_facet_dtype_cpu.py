"""
``SwiftlyForward(..., facet_dtype=...)`` without a device: the keyword is parsed before anything else in the constructor --
``None``, ``torch.float32`` and whatever ``numpy.dtype`` reads as float32 are taken, every other value raises ``ValueError``
(``SwiftlyBackward(facet_dtype=...)`` parses the same way and takes more types: its facets are outputs).
"""
import numpy
import pytest
import torch

from ska_sdp_exec_swiftly_amd import SwiftlyForward
from ska_sdp_exec_swiftly_amd.facet_dtype import BACKWARD, FORWARD, parse_facet_dtype

BAD = (torch.float64, torch.complex64, torch.complex128, torch.float16, "float64", "complex64", numpy.complex64, numpy.float64,
       "real", 32, object(), True)


# (a bare object's str() carries its address, which differs from run to run: it gets a fixed id)
@pytest.mark.parametrize("value", BAD, ids=["object()" if type(v) is object else str(v)[:24] for v in BAD])
def test_constructor_refuses_other_values_before_it_touches_anything(value):
    # (no configuration, no facets, no device: the refusal comes first)
    with pytest.raises(ValueError, match="facet_dtype must be float32 or None"):
        SwiftlyForward(None, [], facet_dtype=value)


def test_accepted_values():
    assert parse_facet_dtype(None, FORWARD) is None and parse_facet_dtype(None, BACKWARD) is None
    for value in (torch.float32, "float32", numpy.float32, numpy.dtype("float32"), "f4"):
        assert parse_facet_dtype(value, FORWARD) is torch.float32, value
        # ... and they are what the backward class reads as float32 too
        assert parse_facet_dtype(value, BACKWARD) is torch.float32
    # an accepted value gets past the parsing: the constructor then fails on the missing configuration, not on the keyword
    with pytest.raises(AttributeError):
        SwiftlyForward(None, [], facet_dtype="float32")
