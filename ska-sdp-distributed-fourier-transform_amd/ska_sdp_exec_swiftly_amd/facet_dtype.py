"""
The small rules about real-valued facets that the four streaming classes share -- ``SwiftlyForward`` / ``DistributedForward``
(``facet_dtype``, ``half_length_k1``) and ``SwiftlyBackward`` / ``DistributedBackward`` (``facet_dtype``,
``half_length_finish``): how the keywords are parsed and refused, that ``facet_dtype`` has the precision of the data, which
input is a float32 facet, and which facet the half-length kernels can load or store as pairs.
"""
import numpy

from .tasks import _torch

#: the ``facet_dtype`` the forward classes take (their facets are inputs) and the backward ones (outputs)
FORWARD, BACKWARD = ("float32",), ("float32", "float64", "complex64", "complex128")
#: ... and ``SwiftlyForward`` alone: float64 facets stay float64 through a complex128 band pipeline (the multi-GPU classes
#: have no such form and keep ``FORWARD``)
FORWARD_SINGLE = FORWARD + ("float64",)


def parse_facet_dtype(facet_dtype, accepted, named=None, note=""):
    """``facet_dtype`` as given to a constructor -> ``None`` or the torch dtype: a torch dtype or anything ``numpy.dtype``
    reads as one of the names in ``accepted``; ``ValueError`` otherwise -- its sentence lists ``named`` (default: ``accepted``)
    and ends with ``note``"""
    if facet_dtype is None:
        return None
    torch = _torch()
    if not isinstance(facet_dtype, torch.dtype):
        try:
            facet_dtype = getattr(torch, numpy.dtype(facet_dtype).name, None)
        except TypeError:
            facet_dtype = None
    if facet_dtype not in [getattr(torch, name) for name in accepted]:
        raise ValueError(f"facet_dtype must be {', '.join(named or accepted)} or None{note}")
    return facet_dtype


def forward_keywords(facet_dtype, half_length_k1):
    """the keywords of the forward classes, before anything touches a configuration or a device: ``facet_dtype`` parsed"""
    parsed = parse_facet_dtype(facet_dtype, FORWARD)
    if half_length_k1 and parsed is None:
        raise ValueError("half_length_k1=True needs facet_dtype=float32")
    return parsed


#: what the refusals of ``SwiftlyForward`` add to the sentence every forward class says
_FLOAT64_NOTE = ("; SwiftlyForward also takes float64, for float64 facets kept real through the complex128 band pipeline "
                 "(wave_axis=1)")


def single_forward_keywords(facet_dtype, half_length_k1, facet_data):
    """the keywords of ``SwiftlyForward``, before anything touches a configuration or a device: those of the forward classes,
    and ``float64`` -- which is a statement about the data, so it is held against the data here: every facet must be one
    ``is_float64_facet`` accepts (then the pass is complex128), and the half-length K1 is a float32 form"""
    parsed = parse_facet_dtype(facet_dtype, FORWARD_SINGLE, named=FORWARD, note=_FLOAT64_NOTE)
    if parsed != _torch().float64:
        return forward_keywords(parsed, half_length_k1)
    if half_length_k1:
        raise ValueError("half_length_k1=True needs facet_dtype=float32")
    facet_data = list(facet_data)
    if not facet_data or not all(is_float64_facet(data) for data in facet_data):
        raise ValueError(f"facet_dtype must be {', '.join(FORWARD)} or None{_FLOAT64_NOTE}: facet_dtype=float64 needs every "
                         "facet as a row-major float64 array (and at least one)")
    return parsed


def backward_keywords(facet_dtype, half_length_finish):
    """the keywords of the backward classes, before anything touches a configuration or a device: ``facet_dtype`` parsed"""
    parsed = parse_facet_dtype(facet_dtype, BACKWARD)
    if half_length_finish and parsed != _torch().float32:
        raise ValueError("half_length_finish=True needs facet_dtype=float32: the half-length finish produces real facets "
                         f"from complex64 data, got facet_dtype={facet_dtype}")
    return parsed


def check_precision(owner, facet_dtype, data_dtype):
    """``facet_dtype`` (parsed) of the backward class named ``owner`` has the precision of the data"""
    torch = _torch()
    if facet_dtype is None:
        return
    single = data_dtype in (torch.complex64, torch.float32)
    if (facet_dtype in (torch.float32, torch.complex64)) != single:
        raise ValueError(f"{owner}(facet_dtype={facet_dtype}) does not match {data_dtype} data: "
                         "float32 / complex64 facets come from complex64 data, float64 / complex128 from complex128")


def name_of(facet_dtype):
    """a parsed ``facet_dtype`` as ``b8_form.B8Facts`` names it: None, ``"float32"``, ``"float64"`` or ``"complex"``"""
    if facet_dtype is None:
        return None
    return "complex" if facet_dtype.is_complex else str(facet_dtype).rsplit(".", 1)[-1]


def is_float32_facet(data):
    """is ``data`` a facet that can stay float32: a float32 host array, or a float32 tensor K1 could read in place (2-D, unit
    stride along its rows)?"""
    torch = _torch()
    if data is None:
        return False
    if isinstance(data, torch.Tensor):
        return data.dtype == torch.float32 and data.dim() == 2 and data.stride(-1) == 1
    return numpy.asarray(data).dtype == numpy.float32


def is_float64_facet(data):
    """is ``data`` a facet that can stay float64: a float64 host array, or a float64 tensor K1 could read in place (2-D, unit
    stride along its rows)?"""
    torch = _torch()
    if data is None:
        return False
    if isinstance(data, torch.Tensor):
        return data.dtype == torch.float64 and data.dim() == 2 and data.stride(-1) == 1
    return numpy.asarray(data).dtype == numpy.float64


def loads_as_pairs(size, off1, yN_size):
    """the pair rule of the half-length kernels (K1 loads, B8 stores aligned pairs of pixels): a facet of even size at an
    even position of the padded row"""
    return size % 2 == 0 and (int(off1) + yN_size // 2 - size // 2) % 2 == 0
