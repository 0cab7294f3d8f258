"""
The K1 form of a cooperative row block of ``DistributedForward`` without a GPU: ``_coop_form`` gathers ``k1_form.K1Facts`` for
the block and asks ``k1_form.choose_k1``, held here to the answers RECORDED from the hand-written rule it replaced
(``tests/golden/coop_k1_forms.txt``, every case of ``tests/b8_form_cases.py``'s ``coop_k1_cases()``; the header of the file
says how it was recorded) -- through the pure chooser on facts written out here, and through the gatherer on an object made with
``__new__`` over a stub core.
"""
import collections
import os
import types

import pytest
import torch

import b8_form_cases as bc
from ska_sdp_exec_swiftly_amd.k1_form import K1Answer, K1Facts, choose_k1

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coop_k1_forms.txt")


def facts_of(case):
    """the facts of the block (the mapping of ``DistributedForward._coop_form``, with the formulas of the method the table was
    recorded from): the band comes from the exchange, so no axis-1-first mode; ``core.prepare_facet_band`` promotes a block
    above 23552 points itself, so the rows always "match"; the half-length form exists only where the real-load form does"""
    b = case.block
    here = b.tensor[0] == bc.DEVICE
    pitch, base = b.tensor[1:] if here else (b.size, 0)
    real = case.real_facets and case.complex64
    return K1Facts(
        wave_axis=1, complex64=case.complex64, all_float32=case.block_float32, float32_asked=case.real_asked,
        half_length_asked=case.half_asked, keeps_real=case.real_asked, axis1_first=False, axis1_fused=False, planned=True,
        real_facets=real, real_facets_rfft=real and case.real_facets_rfft, rows_match_promoted=True,
        even=b.size % 2 == 0 and (b.off1 + bc.YN // 2 - b.size // 2) % 2 == 0, aligned=pitch % 2 == 0 and base % 8 == 0,
    )


class _Tensor:
    """what ``_coop_form`` reads of a row block"""

    def __init__(self, dtype, device, pitch, address):
        self.dtype, self.device, self._pitch, self._address = dtype, device, pitch, address

    def stride(self, dim):
        return self._pitch if dim == 0 else 1

    def data_ptr(self):
        return self._address


def forward_of(case):
    """``(a DistributedForward as its constructor leaves it in front of _coop_form, the block)``, without a device"""
    from ska_sdp_exec_swiftly_amd.distributed import DistributedForward

    fwd = object.__new__(DistributedForward)
    fwd.core = types.SimpleNamespace(yN_size=bc.YN, device=bc.DEVICE, supports_real_facets=lambda: case.real_facets,
                                     supports_real_facets_rfft=lambda: case.real_facets_rfft)
    fwd.dtype = torch.complex64 if case.complex64 else torch.complex128
    fwd._real_asked, fwd._half_asked = case.real_asked, case.half_asked
    fwd.facet_configs = [types.SimpleNamespace(off0=0, off1=case.block.off1, size=case.block.size)]
    return fwd, _Tensor(torch.float32 if case.block_float32 else torch.complex64, *case.block.tensor)


@pytest.fixture(scope="module")
def table():
    return bc.read_coop_k1_table(GOLDEN)


def test_the_enumeration_holds_what_the_table_was_asked_to_hold():
    blocks = {b.name: b for b in bc.BLOCKS}
    assert set(blocks) == {"even", "odd_size", "odd_position", "above_23552", "unaligned_view", "odd_pitch", "host", "other_device"}
    assert blocks["odd_size"].size % 2 and blocks["odd_size"].tensor[1] % 2 == 0
    b = blocks["odd_position"]
    assert b.size % 2 == 0 and (b.off1 + bc.YN // 2 - b.size // 2) % 2
    b = blocks["above_23552"]
    assert b.size > 23552 and b.size % 2 == 0 and (b.off1 + bc.YN // 2 - b.size // 2) % 2 == 0 and b.tensor[1] % 2 == 0
    assert blocks["unaligned_view"].tensor[2] % 8 and blocks["odd_pitch"].tensor[1] % 2
    for name in ("host", "other_device"):  # (not on the core's device: uploaded contiguous, whatever they look like now)
        assert blocks[name].tensor[0] != bc.DEVICE and blocks[name].tensor[1] % 2 and blocks[name].tensor[2] % 8


def test_choose_k1_gives_the_recorded_form_for_every_block(table):
    seen, wrong = collections.Counter(), []
    for case, want in zip(bc.coop_k1_cases(), table):
        got = choose_k1(facts_of(case))
        seen[got] += 1
        if (got.facets_real, got.half_length) != want or got.axis1_mode != 0:
            wrong.append((case, got, want))
    assert not wrong, (len(wrong), wrong[:3])
    assert sum(seen.values()) == len(bc.coop_k1_cases()) == len(table)
    assert set(seen) == {K1Answer(False, False, 0), K1Answer(True, False, 0), K1Answer(True, True, 0)}


def test_coop_form_gathers_what_the_recorded_method_read(table):
    wrong = []
    for case, want in zip(bc.coop_k1_cases(), table):
        fwd, block = forward_of(case)
        got = fwd._coop_form(0, block)  # pylint: disable=protected-access
        if (got.facets_real, got.half_length) != want or got.axis1_mode != 0:
            wrong.append((case, got, want))
    assert not wrong, (len(wrong), wrong[:3])
