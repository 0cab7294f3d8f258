"""
The form of the backward contiguous-axis finish, B8 (``ska_sdp_exec_swiftly_amd/b8_form.py``, ``choose_b8``), without a GPU,
against the answers RECORDED from the methods it replaced: ``tests/golden/b8_forms.txt`` holds, for every case of
``tests/b8_form_cases.py``, what ``SwiftlyBackward.real_finish_native`` / ``half_length_finish`` answered and what
``_finish_bands`` computed for its accumulators, and what ``DistributedBackward``'s two properties and its
``unpack_coop_finish`` did.  The header of the file says how it was recorded.

The same table holds the gatherers -- ``SwiftlyBackward._decide_b8`` and ``DistributedBackward._coop_b8`` with the one pair
rule, what they ask of the core and how the answers of the local object and of the cooperative facets are combined --, driven
on objects made with ``__new__`` over a stub core, as the recorder drove the methods they replaced.
"""
import collections
import os
import types

import pytest
import torch

import b8_form_cases as bc
from ska_sdp_exec_swiftly_amd.b8_form import B8Answer, B8Facts, choose_b8

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "b8_forms.txt")
REFUSAL = "half_length_finish=True needs facet_dtype=float32"


def torch_dtype(name):
    return None if name is None else getattr(torch, name)


def pairs(cover):
    """every facet of the cover has an even size at an even position of the padded row (the formula of the methods the table
    was recorded from)"""
    return all(size % 2 == 0 and (bc.YN // 2 - size // 2 + off1) % 2 == 0 for size, off1 in cover)


def facts_of(case, cover, accumulators=None, resolved=True):
    """the facts a backward object would gather for the case"""
    dtype = case.facet_dtype
    return B8Facts(resolved=resolved, wave_axis=case.wave_axis, facet_dtype="complex" if dtype in ("complex64", "complex128") else dtype,
                   half_length_asked=case.half_length_asked, real_facets_out=case.real_facets_out,
                   real_facets_out_c2r=case.real_facets_out_c2r, pairs=pairs(cover),
                   accumulators_complex64=None if accumulators is None else accumulators == "complex64")


def native_char(native):
    return "N" if native is None else "01"[bool(native)]


class _Core:
    """the stub core of the recording: the two ``supports_*`` answers are the case's; ``finish_facet_band`` notes what it was
    asked for"""

    yN_size, device = bc.YN, "cpu"

    def __init__(self, case):
        self.case, self.finished = case, []

    def supports_real_facets_out(self):
        return self.case.real_facets_out

    def supports_real_facets_out_c2r(self):
        return self.case.real_facets_out_c2r

    def finish_facet_band(self, band_acc, band, facet_off, facet_size, mask=None, real=False, half_length=False):
        self.finished.append((bool(real), bool(half_length)))
        return torch.zeros((band_acc.shape[0], facet_size), dtype=torch.float32 if real else band_acc.dtype)


def configs(cover):
    return [types.SimpleNamespace(off0=0, off1=off1, size=size, mask0=None, mask1=None) for size, off1 in cover]


def backward_of(case, cover, core=None, auto_axis=None, accumulators=None):
    """a ``SwiftlyBackward`` as its constructor leaves it (and, with ``accumulators``, as the first wave does), without a device"""
    from ska_sdp_exec_swiftly_amd.backward import BandAccumulators, SwiftlyBackward

    bwd = object.__new__(SwiftlyBackward)
    bwd.core = core or _Core(case)
    bwd._auto_axis, bwd.wave_axis = bool(auto_axis), case.wave_axis
    bwd._facet_dtype, bwd._want_half_length = torch_dtype(case.facet_dtype), case.half_length_asked
    bwd.facets_config_list = configs(cover)
    bwd.bands = BandAccumulators(bwd.core, bwd.facets_config_list)
    bwd.bands.bands = None if accumulators is None else torch.empty((len(cover), 2, 4), dtype=torch_dtype(accumulators))
    return bwd


def refused(cls, case, **kw):
    """does the constructor refuse the case's keywords -- before it touches its (missing) configuration?"""
    try:
        cls(None, [], facet_dtype=torch_dtype(case.facet_dtype), half_length_finish=case.half_length_asked, **kw)
    except ValueError as err:
        assert REFUSAL in str(err), err
        return True
    except AttributeError:
        return False
    raise AssertionError("the constructor got past a missing configuration")


def pass_dtype(case):
    """the complex dtype of a multi-GPU pass whose precision ``facet_dtype`` matches"""
    return torch.complex128 if case.facet_dtype in ("float64", "complex128") else torch.complex64


def distributed_of(case):
    """a ``DistributedBackward`` as its constructor leaves it, without a device or a process group: one virtual rank that
    holds two rows of every cooperative facet, over a band of four columns"""
    from ska_sdp_exec_swiftly_amd.distributed import DistributedBackward

    core = _Core(case)
    dist = object.__new__(DistributedBackward)
    dist.core, dist.wave_axis, dist.dtype, dist.rank, dist.world = core, case.wave_axis, pass_dtype(case), 0, 1
    dist._facet_dtype, dist._want_half_length = torch_dtype(case.facet_dtype), case.half_length_asked
    dist.facet_configs = configs(case.coop)
    dist.sharding = types.SimpleNamespace(coop=list(range(len(case.coop))), coop_rows=lambda size, rank=None: (0, 2))
    dist.local = None if case.local is None else backward_of(case, bc.COVERS[case.local], core)
    dist._coop_band, dist._coop_sub = (0, 4), [(0, 4)]
    return dist


def coop_chars(dist):
    """what ``unpack_coop_finish`` asks of the core for each of (up to) two cooperative facets: ``-`` no such facet, else
    ``real + 2 * half_length``"""
    chars = ""
    for j in range(2):
        if j >= len(dist.facet_configs):
            chars += "-"
            continue
        del dist.core.finished[:]
        k, row0, out = dist.unpack_coop_finish(j, torch.zeros(8, dtype=dist.dtype))
        (real, half), = dist.core.finished
        assert (k, row0) == (j, 0) and out.dtype == dist.facet_dtype and tuple(out.shape) == (2, dist.facet_configs[j].size)
        chars += str(int(real) + 2 * int(half))
    return chars


@pytest.fixture(scope="module")
def tables():
    return bc.read_b8_table(GOLDEN)


def test_the_enumeration_holds_what_the_table_was_asked_to_hold():
    assert pairs(bc.COVERS["even"]) and pairs(bc.COVERS["empty"]) and bc.COVERS["empty"] == ()
    assert any(size % 2 for size, _ in bc.COVERS["odd_size"]) and not pairs(bc.COVERS["odd_size"])
    assert all(size % 2 == 0 for size, _ in bc.COVERS["odd_position"]) and not pairs(bc.COVERS["odd_position"])
    single, dist = dict(bc.SINGLE_DIMS), dict(bc.DIST_DIMS)
    assert single["facet_dtype"] == dist["facet_dtype"] == (None, "float32", "float64", "complex64", "complex128")
    assert single["accumulators"] == (None, "complex64", "complex128") and set(single["cover"]) == set(bc.COVERS)
    assert dist["local"][0] is None and sorted(len(c) for c in dist["coop"]) == [0, 1, 1, 2]
    assert [pairs(c) for c in dist["coop"]] == [True, True, False, False] and pairs(dist["coop"][3][:1])


def test_choose_b8_gives_the_recorded_answer_for_every_case(tables):
    """the pure chooser, every case of a ``SwiftlyBackward``: the properties' use (no accumulators in the facts) and that of
    ``_finish_bands``; every outcome occurs"""
    seen, wrong = collections.Counter(), []
    for case, want in zip(bc.single_cases(), tables[0]):
        cover = bc.COVERS[case.cover]
        if want == "RRRR":
            assert case.half_length_asked and case.facet_dtype != "float32", case
            continue
        assert not (case.half_length_asked and case.facet_dtype != "float32"), case
        prop = choose_b8(facts_of(case, cover, resolved=not case.auto_axis))
        got = native_char(prop.native) + "01"[prop.half_length]
        assert isinstance(prop.half_length, bool) and isinstance(prop.real_facets, bool)
        assert prop.real_facets == (case.facet_dtype in ("float32", "float64"))
        if case.accumulators is None:
            got += "--"
        else:
            fin = choose_b8(facts_of(case, cover, case.accumulators, resolved=not case.auto_axis))
            got += "01"[bool(fin.native)] + "01"[fin.half_length]
        seen[got] += 1
        if got != want:
            wrong.append((case, got, want))
    assert not wrong, (len(wrong), wrong[:3])
    assert sum(seen.values()) + tables[0].count("RRRR") == len(bc.single_cases()) == len(tables[0])
    assert {w[:2] for w in seen} == {"N0", "00", "10", "11"} and {w[2:] for w in seen} == {"--", "00", "10", "11"}
    assert seen["1100"] > 0  # (the properties answer for the object, ``_finish_bands`` for complex128 accumulators)


def test_decide_b8_gathers_what_the_recorded_methods_read(tables):
    """``SwiftlyBackward`` on a stubbed object, every case: the constructor's refusal, the two properties (fields of
    ``_decide_b8()``) and the answer ``_finish_bands`` reads for its accumulators"""
    from ska_sdp_exec_swiftly_amd.backward import SwiftlyBackward

    wrong = []
    for case, want in zip(bc.single_cases(), tables[0]):
        if refused(SwiftlyBackward, case):
            got = "RRRR"
        else:
            bwd = backward_of(case, bc.COVERS[case.cover], auto_axis=case.auto_axis, accumulators=case.accumulators)
            got = native_char(bwd.real_finish_native) + "01"[bwd.half_length_finish]
            assert bwd.real_finish_native in (None, False, True) and bwd.half_length_finish in (False, True)
            if bwd.bands.bands is None:
                got += "--"
            else:
                fin = bwd._decide_b8(bwd.bands.bands)  # pylint: disable=protected-access
                got += "01"[bool(fin.native)] + "01"[bool(fin.half_length)]
        if got != want:
            wrong.append((case, got, want))
    assert not wrong, (len(wrong), wrong[:3])


def test_finish_bands_runs_the_form_it_decided():
    """``_finish_bands`` hands the answer for its accumulators to ``core.finish_facet_band`` for every facet, and finishes
    complex (then copies the real part out) where the answer is not native"""
    for case in bc.single_cases():
        if case.auto_axis or case.wave_axis != 1 or case.accumulators is None or case.cover == "empty":
            continue
        if (case.half_length_asked and case.facet_dtype != "float32") or pass_dtype(case) != torch_dtype(case.accumulators):
            continue
        bwd = backward_of(case, bc.COVERS[case.cover], accumulators=case.accumulators)
        bwd.core.band_zero_untouched = lambda bands, touched: None
        bwd.bands.band, bwd.bands.touched, bwd.bands.work = (0, 4), None, None
        want = bwd._decide_b8(bwd.bands.bands)  # pylint: disable=protected-access
        out = bwd._finish_bands()  # pylint: disable=protected-access
        assert bwd.core.finished == [(bool(want.native), want.half_length)] * len(out), case
        assert all(t.dtype == (bwd._facet_dtype or torch_dtype(case.accumulators)) for t in out), case  # pylint: disable=protected-access
        assert bwd.bands.bands is None


def test_distributed_backward_gives_the_recorded_answers(tables):
    """``DistributedBackward`` on a stubbed object, every case: the refusal, the two properties -- the local object's answer
    and those of the cooperative facets combined, a rank without a local object included -- and the form
    ``unpack_coop_finish`` asks of the core for each cooperative facet; and ``choose_b8`` on the facts of each such facet"""
    from ska_sdp_exec_swiftly_amd.distributed import DistributedBackward

    seen, wrong = collections.Counter(), []
    for case, want in zip(bc.dist_cases(), tables[1]):
        if refused(DistributedBackward, case, dtype=pass_dtype(case)):
            got = "RRRR"
        else:
            dist = distributed_of(case)
            got = native_char(dist.real_finish_native) + "01"[dist.half_length_finish] + coop_chars(dist)
            assert dist.half_length_finish in (False, True)
            for facet, char in zip(case.coop, want[2:]):
                answer = choose_b8(facts_of(case._replace(wave_axis=1), (facet,)))
                if case.wave_axis == 1 and int(bool(answer.native)) + 2 * int(answer.half_length) != int(char):
                    wrong.append((case, facet, answer, char))
        seen[got] += 1
        if got != want:
            wrong.append((case, got, want))
    assert not wrong, (len(wrong), wrong[:3])
    assert sum(seen.values()) == len(bc.dist_cases()) == len(tables[1])
    # (all ranks' rows half-length; the local object's are not; an even and an odd cooperative facet; a rank whose rows only are)
    assert {"11--", "113-", "103-", "1031", "101-", "000-"} <= set(seen), sorted(seen)


def test_chooser_is_pure():
    """no torch, no library, no package import in the chooser's module"""
    import ska_sdp_exec_swiftly_amd.b8_form as mod

    with open(mod.__file__, encoding="utf-8") as fh:
        source = fh.read()
    assert "import torch" not in source and "_lib" not in source and "from ." not in source
    assert choose_b8(B8Facts(True, 1, "float32", True, True, True, True, None)) == B8Answer(True, True, True)
