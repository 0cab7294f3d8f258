"""
The three roles of the backward pass -- ``SubgridSplitter`` (``splitter.py``), ``ColumnAccumulators`` and
``BandAccumulators`` (``backward.py``) -- as freshly constructed objects over a stub core, without a GPU: what a splitter
holds, and that both accumulator classes refuse a wave that does not share their wave key before they touch a device or create
any state (the stub core has neither a device nor a ``launch``: anything past the check would raise ``AttributeError``).
"""
import types

import numpy
import pytest

from ska_sdp_exec_swiftly_amd import api
from ska_sdp_exec_swiftly_amd.backward import BandAccumulators, ColumnAccumulators
from ska_sdp_exec_swiftly_amd.splitter import SubgridSplitter

CORE = types.SimpleNamespace(xM_yN_size=4, yN_size=16)
FACETS = [api.FacetConfig(0, 0, 8), api.FacetConfig(0, 8, 8), api.FacetConfig(8, 0, 8)]
PARTS = numpy.zeros((len(FACETS), 2, 4, 4), dtype=numpy.complex64)


def test_a_splitter_holds_offsets_and_workspaces_and_nothing_of_a_schedule():
    splitter = SubgridSplitter(CORE, FACETS)
    assert set(vars(splitter)) == {"core", "facet_configs", "dtype", "_off0s", "_off0_of", "_wsbuf", "_ring"}
    assert splitter.dtype is None and splitter._wsbuf == {} and splitter._ring == 0
    assert splitter._off0s == [0, 8] and splitter._off0_of == [0, 0, 1]
    for name in ("lru", "task_queue", "queue_size", "wave_axis", "_auto_axis", "_plan", "facet_dtype", "_facet_dtype",
                 "MNAF_BMNAFs_persist", "bands", "columns"):
        assert not hasattr(splitter, name), name
    assert SubgridSplitter(CORE, FACETS, "a dtype").dtype == "a dtype"


def test_band_accumulators_refuse_a_wave_that_does_not_share_off1():
    same_off0 = [api.SubgridConfig(0, 0, 8), api.SubgridConfig(0, 8, 8)]  # the reference's accumulate_column grouping
    acc, seen = BandAccumulators(CORE, FACETS), []
    with pytest.raises(ValueError, match="share off1=0, got off1=8"):
        acc.accumulate(0, [(same_off0, PARTS)], first=seen.append)
    with pytest.raises(ValueError, match="share off1"):  # (in a later chunk too)
        acc.accumulate(0, [(same_off0[:1], PARTS[:, :1]), (same_off0[1:], PARTS[:, 1:])])
    assert not seen  # (the owner hears of the dtype only once the wave is accepted)
    assert acc.band is None and acc.bands is None and acc.touched is None and acc.masks0 is None and acc.work is None
    assert acc.accumulate(0, []) is None and acc.accumulate(0, [([], PARTS[:, :0])]) is None and acc.bands is None


def test_column_accumulators_refuse_a_wave_that_does_not_share_off0():
    same_off1 = [api.SubgridConfig(0, 0, 8), api.SubgridConfig(8, 0, 8)]
    acc = ColumnAccumulators(CORE, FACETS, lru_backward=2)
    with pytest.raises(ValueError, match="share off0=0"):
        acc.accumulate_wave(same_off1, PARTS)
    assert acc.MNAF_BMNAFs_persist == [None] * len(FACETS) and not acc.lru._items and acc.lru.cache_size == 2
    assert acc.accumulate(0, []) is None and not acc.lru._items


def test_the_front_answers_reads_of_the_moved_names_from_the_roles():
    """``_band``, ``_bands``, ``_work``, ``_masks0`` and ``_wsbuf`` were attributes of ``SwiftlyBackward`` itself; callers
    written against that (the earlier versions of the GPU tests among them) read the same objects through the front, an
    attribute set on the object still wins, and an object without its roles says ``AttributeError``, not ``RecursionError``"""
    bwd = object.__new__(api.SwiftlyBackward)
    for name in ("_bands", "_wsbuf", "bands", "splitter", "_no_such_name"):
        with pytest.raises(AttributeError, match=name):
            getattr(bwd, name)
    bwd.bands, bwd.splitter = BandAccumulators(CORE, FACETS), SubgridSplitter(CORE, FACETS)
    bwd.bands.band, bwd.bands.bands, bwd.bands.work, bwd.bands.masks0 = (0, 4), "bands", "work", "masks0"
    assert (bwd._band, bwd._bands, bwd._work, bwd._masks0) == ((0, 4), "bands", "work", "masks0")
    assert bwd._wsbuf is bwd.splitter._wsbuf
    with pytest.raises(AttributeError, match="_touched"):
        bwd._touched  # pylint: disable=pointless-statement
    bwd._bands = "set by hand"
    assert bwd._bands == "set by hand" and bwd.bands.bands == "bands"
