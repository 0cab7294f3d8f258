"""
The K1 form of a forward object (``ska_sdp_exec_swiftly_amd/k1_form.py``, ``choose_k1``), without a GPU, against the answers
RECORDED from the five methods of ``SwiftlyForward`` it replaced: ``tests/golden/k1_forms.txt`` holds, for every case of
``tests/k1_form_cases.py``, what the constructor decided (half-length K1, facets kept float32, axis-1-first mode) and the mode
``set_band`` chose for a band from outside whose window-rows answers are the opposite of the plan's, with the facets already
resident as float32 and as complex.  The header of the file says how it was recorded.

The same table holds the gatherer, ``SwiftlyForward._decide_k1`` -- the alignment scan, the evenness computation, what it asks
of the core and the hand-over of the settled residency -- driven on an object made with ``__new__`` over a stub core and a stub
``_ingest``, as the recorder drove the methods it replaced; and an object without facets (a rank of the multi-GPU pass that
owns none) decides as the parent did.
"""
import collections
import os
import types

import pytest

import k1_form_cases as kc
from ska_sdp_exec_swiftly_amd.k1_form import K1Answer, K1Facts, choose_k1

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k1_forms.txt")


def facts_of(case):
    """the facts a ``SwiftlyForward`` would gather for the case (``SwiftlyForward._decide_k1``, with the formulas of the
    methods the table was recorded from)"""
    f = case.facets
    return K1Facts(
        wave_axis=case.wave_axis, complex64=case.complex64, all_float32=f.float32, float32_asked=case.float32_asked,
        half_length_asked=case.half_length_asked, keeps_real=case.keeps_real, axis1_first=case.axis1_first,
        axis1_fused=case.axis1_fused, planned=case.planned, real_facets=case.real_facets,
        real_facets_rfft=case.real_facets_rfft, window_rows=case.window_rows, window_rows_real=case.window_rows_real,
        rows_match_promoted=all(not (kc.YN == 32768 and n > 23552) for n in f.sizes),
        even=all(n % 2 == 0 and (o + kc.YN // 2 - n // 2) % 2 == 0 for n, o in zip(f.sizes, f.off1s)),
        aligned=all(t is None or t[0] != kc.DEVICE or (t[1] % 2 == 0 and t[2] % 8 == 0) for t in f.tensors),
    )


class _Tensor:
    """what ``_decide_k1`` reads of a resident facet"""

    def __init__(self, device, pitch, address):
        self.device, self._pitch, self._address = device, pitch, address

    def stride(self, dim):
        assert dim == 0
        return self._pitch

    def data_ptr(self):
        return self._address


class _Core:
    """the stub core of the recording: the ``supports_*`` answers are the case's (the opposite for ``OTHER_BAND``)"""

    yN_size, device = kc.YN, kc.DEVICE

    def __init__(self, case):
        self.case, self.axis1_first = case, case.axis1_first

    def supports_real_facets(self):
        return self.case.real_facets

    def supports_real_facets_rfft(self):
        return self.case.real_facets_rfft

    def _real_rows_match_promoted(self, facet_size):
        from ska_sdp_exec_swiftly_amd.core_hip import SwiftlyCoreHip

        return SwiftlyCoreHip._real_rows_match_promoted(self, facet_size)  # pylint: disable=protected-access

    def band_for_offsets(self, subgrid_offs):
        assert list(subgrid_offs) == [0, 928, 1856]
        return kc.PLAN_BAND

    def supports_window_rows(self, band, facet_size, facet_off1s, n_windows=1, real=False):
        assert facet_size == self.case.facets.sizes[0] and list(facet_off1s) == list(self.case.facets.off1s) and n_windows == 3
        answer = self.case.window_rows_real if real else self.case.window_rows
        if tuple(band) == kc.OTHER_BAND:
            return not answer
        assert tuple(band) == (kc.PLAN_BAND if self.case.planned and self.case.complex64 else (0, kc.YN))
        return answer


def forward_of(case, cls=None, facets=True):
    """a forward object as the constructor leaves it in front of ``_decide_k1``, without a device"""
    import torch

    from ska_sdp_exec_swiftly_amd.forward import SwiftlyForward

    f = case.facets
    fwd = object.__new__(cls or SwiftlyForward)
    fwd.core, fwd.wave_axis = _Core(case), case.wave_axis
    fwd.dtype = torch.complex64 if case.complex64 else torch.complex128
    fwd._facet_dtype_asked = torch.float32 if case.float32_asked else None
    fwd._half_length_asked, fwd._k1 = case.half_length_asked, None
    fwd._keep_real_facets, fwd.axis1_fused = case.keeps_real, case.axis1_fused
    fwd._plan = [types.SimpleNamespace(off0=0, off1=o) for o in (0, 928, 1856)] if case.planned else None
    fwd._planned_keys = {0, 928, 1856} if case.planned else None
    fwd.facet_configs = [types.SimpleNamespace(off0=0, off1=o) for o in f.off1s] if facets else []
    fwd._facet_info = [(torch.complex64, (n, n), True) for n in f.sizes] if facets else []
    fwd._ingest = types.SimpleNamespace(all_float32=f.float32 and facets, real=False,
                                        tensors=[None if t is None else _Tensor(*t) for t in f.tensors] if facets else [])
    fwd._band, fwd.BF_Fs_persist = None, None
    return fwd


@pytest.fixture(scope="module")
def table():
    return kc.read_table(GOLDEN)


def test_the_enumeration_holds_what_the_table_was_asked_to_hold():
    names = {f.name: f for f in kc.FACETS}
    assert any(n % 2 for n in names["odd_size"].sizes)
    assert any((o + kc.YN // 2 - n // 2) % 2 for n, o in zip(names["odd_position"].sizes, names["odd_position"].off1s))
    assert max(names["above_23552"].sizes) > 23552
    assert names["unaligned_view"].tensors[1][2] % 8 and names["odd_pitch"].tensors[1][1] % 2
    assert None in names["host"].tensors
    dims = dict(kc.DIMS)
    assert dims["axis1_first"] == (False, "rows", True)
    assert dims["keeps_real"] == dims["axis1_fused"] == (False, True)


def test_choose_k1_gives_the_recorded_answer_for_every_case(table):
    """the constructor's use (residency undecided), every case; and all eight outcomes occur, the rare ones included"""
    seen = collections.Counter()
    wrong = []
    for case, (want, _, _) in zip(kc.cases(), table):
        got = choose_k1(facts_of(case))
        assert isinstance(got.facets_real, bool) and isinstance(got.half_length, bool)
        seen[got] += 1
        if int(kc.outcome_char(got.half_length, got.facets_real, got.axis1_mode), 12) != want:
            wrong.append((case, got, want))
    assert not wrong, (len(wrong), wrong[:3])
    assert sum(seen.values()) == kc.n_cases() == len(table)
    assert set(seen) == {K1Answer(r, h, m) for h, r, m in
                         [(0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 1, 0), (0, 1, 1), (0, 1, 2), (1, 1, 0), (1, 1, 1)]}
    assert seen[K1Answer(True, False, 2)] >= 4 and seen[K1Answer(True, True, 0)] >= 64


def test_choose_k1_gives_the_recorded_mode_for_a_band_from_outside(table):
    """the ``set_band`` use: residency settled (as float32, as complex), the window-rows facts those of the other band;
    residency and the half-length form pass through"""
    wrong = []
    for case, (_, want_real, want_complex) in zip(kc.cases(), table):
        facts = facts_of(case)._replace(window_rows=not case.window_rows, window_rows_real=not case.window_rows_real)
        for real, want in ((True, want_real), (False, want_complex)):
            for half in (False, True):
                got = choose_k1(facts._replace(settled=K1Answer(real, half, 0)))
                if got != K1Answer(real, half, want):
                    wrong.append((case, real, got, want))
    assert not wrong, (len(wrong), wrong[:3])


def test_decide_k1_gathers_what_the_recorded_methods_read(table):
    """``SwiftlyForward._decide_k1`` on a stubbed object, every case: the constructor's call (its own band, worked out only
    where the window rows matter), ``_axis1()`` before ``set_band``, then ``set_band`` for the band from outside with the
    residency the constructor settled -- and with the other one -- against the recorded modes"""
    wrong = []
    for case, (want, want_real, want_complex) in zip(kc.cases(), table):
        fwd = forward_of(case)
        got = fwd._decide_k1(own=True)  # pylint: disable=protected-access
        if int(kc.outcome_char(got.half_length, got.facets_real, got.axis1_mode), 12) != want or fwd._k1 is not got:
            wrong.append((case, got, want))
            continue
        stored = fwd._k1  # pylint: disable=protected-access
        active = case.wave_axis == 1 and bool(case.axis1_first) and case.complex64
        if fwd._axis1() != int(active) or fwd._k1 is not stored:  # (no band: never 2; and a getter that changes nothing)
            wrong.append((case, "_axis1 before set_band", fwd._axis1()))
        for real, want_mode in ((got.facets_real, want_real if got.facets_real else want_complex),
                                (not got.facets_real, want_complex if got.facets_real else want_real)):
            fwd._k1 = got._replace(facets_real=real)  # pylint: disable=protected-access
            if case.planned:
                mode = fwd.set_band(kc.OTHER_BAND)
                ok = fwd._axis1() == mode and (fwd._window_of is not None) == (mode == 2)  # pylint: disable=protected-access
            else:  # (set_band's window table needs the plan; the decision itself does not)
                mode, ok = fwd._decide_k1(kc.OTHER_BAND).axis1_mode, True  # pylint: disable=protected-access
            if not ok or fwd._k1 != K1Answer(real, got.half_length, want_mode):  # pylint: disable=protected-access
                wrong.append((case, real, fwd._k1, want_mode))  # pylint: disable=protected-access
    assert not wrong, (len(wrong), wrong[:3])


def test_decide_k1_of_an_object_without_facets():
    """a rank of the multi-GPU pass that owns no facet builds its forward object from an empty list: nothing is asked about
    window rows (there is no facet to ask about), the facets are "not real" and the mode is a row pass per wave where the
    axis-1-first pipeline is on -- in the constructor's call and for a band from outside"""
    from ska_sdp_exec_swiftly_amd.forward import SwiftlyForward, _PromotingForward

    for case in kc.cases():
        if case.facets.name not in ("complex", "float32") or not (case.window_rows and case.window_rows_real):
            continue
        active = case.wave_axis == 1 and bool(case.axis1_first) and case.complex64
        for cls in (SwiftlyForward, _PromotingForward):
            fwd = forward_of(case, cls, facets=False)
            if cls is _PromotingForward:
                del fwd._keep_real_facets  # (the class switch itself)
            assert fwd._decide_k1(own=True) == K1Answer(False, False, int(active)), case  # pylint: disable=protected-access
            assert fwd._axis1() == int(active)  # pylint: disable=protected-access
            assert fwd._decide_k1(kc.OTHER_BAND) == K1Answer(False, False, int(active)), case  # pylint: disable=protected-access
