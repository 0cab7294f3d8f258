"""
The enumerations behind ``tests/golden/b8_forms.txt`` (what a ``SwiftlyBackward`` and a ``DistributedBackward`` decide about the
contiguous-axis finish, B8) and ``tests/golden/coop_k1_forms.txt`` (the K1 form of a cooperative row block of
``DistributedForward``): every combination of what decides them, in the order of the files (``itertools.product`` over the
dimensions, the last one fastest).  No import of the package: the recorder that drove the methods the tables replaced and
``tests/test_b8_form_cpu.py`` / ``tests/test_coop_k1_form_cpu.py`` both read it.
"""
import itertools
from collections import namedtuple

YN = 32768            # the padded facet size of the stub core
DEVICE = "dev0"       # the stub core's device

#: covers as (size, off1) per facet.  ``empty``: an object without facets (``all([])`` is True)
COVERS = {
    "even": ((512, 0), (512, 1024)),
    "odd_size": ((512, 0), (511, 1024)),
    "odd_position": ((512, 0), (512, 1023)),
    "empty": (),
}
FACET_DTYPES = (None, "float32", "float64", "complex64", "complex128")


def _product(dims):
    case = namedtuple("Case", [name for name, _ in dims])
    return [case(*values) for values in itertools.product(*(values for _, values in dims))]


# ---- SwiftlyBackward --------------------------------------------------------------------------------------------------
#: ``accumulators``: the dtype of ``_bands`` (None: no band accumulators yet)
SINGLE_DIMS = (
    ("auto_axis", (False, True)),
    ("wave_axis", (0, 1)),
    ("facet_dtype", FACET_DTYPES),
    ("half_length_asked", (False, True)),
    ("real_facets_out", (False, True)),
    ("real_facets_out_c2r", (False, True)),
    ("cover", tuple(COVERS)),
    ("accumulators", (None, "complex64", "complex128")),
)


def single_cases():
    return _product(SINGLE_DIMS)


# ---- DistributedBackward ----------------------------------------------------------------------------------------------
#: ``local``: None (a rank without a local object) or the cover of its local ``SwiftlyBackward``; ``coop``: the cooperative
#: facets as (size, off1) -- none, one even, one at an odd position, an even and an odd-sized one
COOPS = ((), ((512, 2048),), ((512, 2047),), ((512, 2048), (511, 4096)))
DIST_DIMS = (
    ("local", (None, "even", "odd_size")),
    ("wave_axis", (0, 1)),
    ("facet_dtype", FACET_DTYPES),
    ("half_length_asked", (False, True)),
    ("real_facets_out", (False, True)),
    ("real_facets_out_c2r", (False, True)),
    ("coop", COOPS),
)


def dist_cases():
    return _product(DIST_DIMS)


def read_b8_table(path):
    """``(single, dist)``: four characters per case of ``single_cases()``, then four per case of ``dist_cases()`` (the header
    of the file says what they mean); ``#`` lines and line breaks skipped"""
    with open(path, encoding="utf-8") as fh:
        text = "".join(line.strip() for line in fh if not line.startswith("#"))
    n_single, n_dist = len(single_cases()), len(dist_cases())
    assert len(text) == 4 * (n_single + n_dist), (len(text), n_single, n_dist)
    words = [text[i : i + 4] for i in range(0, len(text), 4)]
    return words[:n_single], words[n_single:]


# ---- DistributedForward: K1 of a cooperative row block ----------------------------------------------------------------
#: one block: the facet's (size, off1) and the block as (device, row pitch in reals, address).  A block that is not on the
#: core's device is uploaded contiguous, so its pitch and address never count
Block = namedtuple("Block", "name size off1 tensor")
BLOCKS = (
    Block("even", 512, 1024, (DEVICE, 512, 4096)),
    Block("odd_size", 511, 1024, (DEVICE, 512, 4096)),
    Block("odd_position", 512, 1023, (DEVICE, 512, 4096)),
    Block("above_23552", 23554, 1, (DEVICE, 23554, 4096)),
    Block("unaligned_view", 512, 1024, (DEVICE, 512, 4100)),
    Block("odd_pitch", 512, 1024, (DEVICE, 513, 4096)),
    Block("host", 512, 1024, ("cpu", 513, 4100)),
    Block("other_device", 512, 1024, ("dev1", 513, 4100)),
)
COOP_K1_DIMS = (
    ("real_asked", (False, True)),
    ("half_asked", (False, True)),
    ("complex64", (False, True)),
    ("block_float32", (False, True)),
    ("real_facets", (False, True)),
    ("real_facets_rfft", (False, True)),
    ("block", BLOCKS),
)


def coop_k1_cases():
    return _product(COOP_K1_DIMS)


def read_coop_k1_table(path):
    """``(stays float32, half-length)`` per case of ``coop_k1_cases()``: one character each, ``real + 2 * half``"""
    with open(path, encoding="utf-8") as fh:
        text = "".join(line.strip() for line in fh if not line.startswith("#"))
    assert len(text) == len(coop_k1_cases()), (len(text), len(coop_k1_cases()))
    return [(bool(int(c) & 1), bool(int(c) & 2)) for c in text]
