"""
The enumeration behind ``tests/golden/k1_forms.txt``: every combination of what decides a forward object's K1 form, in the
order of the file (``itertools.product`` over ``DIMS``, the last one fastest).  No import of the package: the recorder that
drove the methods this table replaced and ``tests/test_k1_form_cpu.py`` both read it.
"""
import itertools
from collections import namedtuple

YN = 32768            # the padded facet size of the stub core (``_real_rows_match_promoted`` bites above 23552 here)
DEVICE = "dev0"       # the stub core's device; a tensor anywhere else is uploaded contiguously, so never misaligned

#: one cover of two facets: what the constructor would know of it.  ``tensors``: per facet None (a host array) or
#: (device, row pitch in reals, address)
Facets = namedtuple("Facets", "name float32 sizes off1s tensors")
_OK = (DEVICE, 512, 4096)
FACETS = (
    Facets("complex", False, (512, 512), (0, 1024), (_OK, _OK)),
    Facets("float32", True, (512, 512), (0, 1024), (_OK, _OK)),
    Facets("odd_size", True, (512, 511), (0, 1024), (_OK, _OK)),
    Facets("odd_position", True, (512, 512), (0, 1023), (_OK, _OK)),
    Facets("above_23552", True, (512, 23554), (0, 1), (_OK, _OK)),
    Facets("unaligned_view", True, (512, 512), (0, 1024), (_OK, (DEVICE, 512, 4100))),
    Facets("odd_pitch", True, (512, 512), (0, 1024), (_OK, (DEVICE, 513, 4096))),
    Facets("host", True, (512, 512), (0, 1024), (None, _OK)),
    Facets("other_device", True, (512, 512), (0, 1024), (("dev1", 513, 4100), _OK)),
)

#: (name, values); ``window_rows`` / ``window_rows_real`` are ``core.supports_window_rows(band, ..., real=False / True)`` for
#: the object's own band -- for ``OTHER_BAND``, the one of the ``set_band`` columns, the stub core answers the opposite
DIMS = (
    ("wave_axis", (0, 1)),
    ("complex64", (False, True)),
    ("facets", FACETS),
    ("float32_asked", (False, True)),
    ("half_length_asked", (False, True)),
    ("keeps_real", (False, True)),
    ("axis1_first", (False, "rows", True)),
    ("axis1_fused", (False, True)),
    ("planned", (False, True)),
    ("real_facets", (False, True)),
    ("real_facets_rfft", (False, True)),
    ("window_rows", (False, True)),
    ("window_rows_real", (False, True)),
)
Case = namedtuple("Case", [name for name, _ in DIMS])
PLAN_BAND, OTHER_BAND = (10736, 11472), (4096, 2048)


def cases():
    """every case, in the order of the file"""
    return (Case(*values) for values in itertools.product(*(values for _, values in DIMS)))


def n_cases():
    n = 1
    for _, values in DIMS:
        n *= len(values)
    return n


def outcome_char(half_length, facets_real, mode):
    """the constructor's outcome as one character: ``mode + 3 * facets_real + 6 * half_length`` in base 12"""
    return "0123456789ab"[int(mode) + 3 * int(bool(facets_real)) + 6 * int(bool(half_length))]


def read_table(path):
    """[(constructor outcome, set_band mode with real residency, set_band mode with complex residency)] per case: three
    characters each, ``#`` lines and line breaks skipped"""
    with open(path, encoding="utf-8") as fh:
        text = "".join(line.strip() for line in fh if not line.startswith("#"))
    assert len(text) == 3 * n_cases(), (len(text), n_cases())
    return [(int(text[i], 12), int(text[i + 1]), int(text[i + 2])) for i in range(0, len(text), 3)]
