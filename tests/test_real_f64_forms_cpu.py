"""
The float64 rules of the two pure choosers, without a GPU: ``k1_form.choose_k1`` with the facts ``all_float64`` /
``float64_asked`` / ``real_facets_f64`` and ``b8_form.choose_b8`` with ``real_facets_out_f64`` -- every combination of the new
facts with what they depend on, written out as the rule of the issue; that the new facts at their defaults change no answer
of the cases of ``tests/k1_form_cases.py`` and ``tests/b8_form_cases.py`` (whose recorded tables ``tests/test_k1_form_cpu.py``
and ``tests/test_b8_form_cpu.py`` hold); that the gatherers read a core without the new ``supports_*`` methods as "no such
form"; and that both choosers stay pure.
"""
import ast
import itertools
import os

import b8_form_cases as bc
import k1_form_cases as kc
import test_b8_form_cpu as b8t
import test_k1_form_cpu as k1t
from ska_sdp_exec_swiftly_amd import b8_form, k1_form
from ska_sdp_exec_swiftly_amd.b8_form import B8Answer, B8Facts, choose_b8
from ska_sdp_exec_swiftly_amd.k1_form import K1Answer, K1Facts, choose_k1

BOOLS = (False, True)


# ------------------------------------------------------------------------------------------------------------ choose_k1
def test_k1_facts_append_the_new_ones_with_defaults_that_say_no():
    assert K1Facts._fields[-4:] == ("settled", "all_float64", "float64_asked", "real_facets_f64")
    f = K1Facts(wave_axis=1, complex64=False, all_float32=False, float32_asked=False, half_length_asked=False, keeps_real=True,
                axis1_first=False, axis1_fused=True, planned=True, real_facets=True, real_facets_rfft=True)
    assert (f.all_float64, f.float64_asked, f.real_facets_f64) == (False, False, False)
    assert choose_k1(f) == K1Answer(False, False, 0)


def test_choose_k1_float64_rule_every_combination():
    """``facets_real`` for float64 needs ``keeps_real``, ``wave_axis == 1``, a complex128 pass, ``all_float64``,
    ``float64_asked`` and ``real_facets_f64``; then ``half_length`` is False and ``axis1_mode`` 0 -- whatever the axis-1-first
    switches, the plan, the half-length keyword and the float32 facts of the library say.  (A float64 pass has no float32
    facets: ``all_float32`` False.)"""
    n = 0
    for keeps, axis, c64, all64, asked, lib in itertools.product(BOOLS, (0, 1), BOOLS, BOOLS, BOOLS, BOOLS):
        for a1, fused, planned, half_asked, real32, rfft in itertools.product((False, "rows", True), BOOLS, BOOLS, BOOLS, BOOLS, BOOLS):
            f = K1Facts(wave_axis=axis, complex64=c64, all_float32=False, float32_asked=False, half_length_asked=half_asked,
                        keeps_real=keeps, axis1_first=a1, axis1_fused=fused, planned=planned, real_facets=real32,
                        real_facets_rfft=rfft, window_rows=True, window_rows_real=True, all_float64=all64, float64_asked=asked,
                        real_facets_f64=lib)
            want_real = keeps and axis == 1 and not c64 and all64 and asked and lib
            got = choose_k1(f)
            assert got.facets_real is bool(want_real) and got.half_length is False, f
            if want_real:
                assert got.axis1_mode == 0, f
            else:  # exactly what the facts say without the new ones
                assert got == choose_k1(f._replace(all_float64=False, float64_asked=False, real_facets_f64=False)), f
            n += 1
    assert n == 64 * 96


def test_choose_k1_settled_residency_passes_through():
    """``set_band``'s use: the residency the constructor settled stays, and a complex128 pass runs the default order"""
    f = K1Facts(wave_axis=1, complex64=False, all_float32=False, float32_asked=False, half_length_asked=False, keeps_real=True,
                axis1_first=True, axis1_fused=True, planned=True, real_facets=False, real_facets_rfft=False, all_float64=True,
                float64_asked=True, real_facets_f64=True)
    assert choose_k1(f) == K1Answer(True, False, 0)
    for real in BOOLS:
        assert choose_k1(f._replace(settled=K1Answer(real, False, 0))) == K1Answer(real, False, 0)


def test_choose_k1_defaults_change_no_recorded_case():
    """every case of ``tests/k1_form_cases.py``: the facts as ``tests/test_k1_form_cpu.py`` builds them leave the new ones at
    their defaults, and stating the defaults -- or float64 facts that do not apply to a pass with float32 / complex facets --
    gives the same answer"""
    n = 0
    for case in kc.cases():
        facts = k1t.facts_of(case)
        assert (facts.all_float64, facts.float64_asked, facts.real_facets_f64) == (False, False, False)
        base = choose_k1(facts)
        assert choose_k1(facts._replace(all_float64=False, float64_asked=False, real_facets_f64=False)) == base
        # the library having the float64 K1 changes nothing for a caller who did not ask or has no float64 facets
        assert choose_k1(facts._replace(real_facets_f64=True)) == base
        assert choose_k1(facts._replace(real_facets_f64=True, float64_asked=True)) == base
        assert choose_k1(facts._replace(real_facets_f64=True, all_float64=True)) == base
        n += 1
    assert n == kc.n_cases()


def test_decide_k1_reads_a_stub_without_the_new_names_as_no():
    """``SwiftlyForward._decide_k1`` on the stubs of ``tests/test_k1_form_cpu.py`` (an ``_ingest`` without ``all_float64``, a
    core without ``supports_real_facets_f64``): the answers of the recorded table"""
    table = kc.read_table(k1t.GOLDEN)
    for case, (want, _, _) in list(zip(kc.cases(), table))[:: 37]:
        fwd = k1t.forward_of(case)
        assert not hasattr(fwd.core, "supports_real_facets_f64") and not hasattr(fwd._ingest, "all_float64")
        got = fwd._decide_k1(own=True)  # pylint: disable=protected-access
        assert int(kc.outcome_char(got.half_length, got.facets_real, got.axis1_mode), 12) == want, case


# ------------------------------------------------------------------------------------------------------------ choose_b8
def test_b8_facts_append_the_new_one_with_a_default_that_says_no():
    assert B8Facts._fields[-2:] == ("accumulators_complex64", "real_facets_out_f64")
    f = B8Facts(resolved=True, wave_axis=1, facet_dtype="float64", half_length_asked=False, real_facets_out=True,
                real_facets_out_c2r=True, pairs=True)
    assert f.accumulators_complex64 is None and f.real_facets_out_f64 is False
    assert choose_b8(f) == B8Answer(True, False, False)


def test_choose_b8_float64_rule_every_combination():
    """``native`` is also true for ``facet_dtype == "float64"`` when ``real_facets_out_f64`` holds, ``wave_axis == 1`` and the
    accumulators are not complex64; the half-length form stays a float32 form; every other ``facet_dtype`` answers as without
    the new fact"""
    n = 0
    dims = (BOOLS, (0, 1), (None, "float32", "float64", "complex"), BOOLS, BOOLS, BOOLS, BOOLS, (None, False, True), BOOLS)
    for resolved, axis, dtype, half_asked, out32, c2r, pairs, acc64, out64 in itertools.product(*dims):
        f = B8Facts(resolved=resolved, wave_axis=axis, facet_dtype=dtype, half_length_asked=half_asked, real_facets_out=out32,
                    real_facets_out_c2r=c2r, pairs=pairs, accumulators_complex64=acc64, real_facets_out_f64=out64)
        got = choose_b8(f)
        if dtype == "float64":
            assert got.real_facets is True and got.half_length is False, f
            if not resolved:
                assert got.native is None, f
            else:
                assert got.native is bool(out64 and axis == 1 and acc64 is not True), f
        else:
            assert got == choose_b8(f._replace(real_facets_out_f64=False)), f
        n += 1
    assert n == 2 * 2 * 4 * 16 * 3 * 2


def test_choose_b8_default_changes_no_recorded_case():
    """every case of ``tests/b8_form_cases.py``, with the facts as ``tests/test_b8_form_cpu.py`` builds them: the new fact is
    at its default, stating it gives the same answer, and float64 facets without it are finished complex as before"""
    n = 0
    for case in bc.single_cases():
        cover = bc.COVERS[case.cover]
        for resolved in BOOLS:
            facts = b8t.facts_of(case, cover, case.accumulators, resolved=resolved)
            assert facts.real_facets_out_f64 is False
            base = choose_b8(facts)
            assert choose_b8(facts._replace(real_facets_out_f64=False)) == base
            if case.facet_dtype == "float64":
                assert base == B8Answer(True, False if resolved else None, False)
            else:
                assert choose_b8(facts._replace(real_facets_out_f64=True)) == base
        n += 1
    assert n == len(bc.single_cases())


def test_decide_b8_reads_a_core_without_the_new_method_as_no():
    """``SwiftlyBackward._decide_b8`` over the stub core of ``tests/test_b8_form_cpu.py`` (no ``supports_real_facets_out_f64``):
    float64 facets on the band schedule are not native; a core that has the method is asked only where it matters"""
    import torch

    asked = []

    class WithMethod(b8t._Core):  # pylint: disable=protected-access
        def supports_real_facets_out_f64(self):
            asked.append(1)
            return True

    for case in bc.single_cases():
        if case.cover != "even" or case.accumulators is not None or case.half_length_asked:
            continue
        cover = bc.COVERS[case.cover]
        bwd = b8t.backward_of(case, cover, auto_axis=case.auto_axis)
        assert not hasattr(bwd.core, "supports_real_facets_out_f64")
        base = bwd._decide_b8()  # pylint: disable=protected-access
        if case.facet_dtype == "float64":
            assert base.native in (None, False)
        del asked[:]
        got = b8t.backward_of(case, cover, core=WithMethod(case), auto_axis=case.auto_axis)._decide_b8()  # pylint: disable=protected-access
        applies = case.facet_dtype == "float64" and case.wave_axis == 1 and not case.auto_axis
        assert bool(asked) == applies, case
        assert got == (base._replace(native=True) if applies else base), case
        if applies:  # ... and not from complex64 accumulators
            bands = torch.empty((2, 2, 4), dtype=torch.complex64)
            assert b8t.backward_of(case, cover, core=WithMethod(case))._decide_b8(bands).native is False  # pylint: disable=protected-access
            assert b8t.backward_of(case, cover, core=WithMethod(case))._decide_b8(bands.to(torch.complex128)).native is True  # pylint: disable=protected-access


# --------------------------------------------------------------------------------------------------------------- purity
def test_both_choosers_stay_pure():
    """no torch, no native library, nothing of the package: the modules import ``collections.namedtuple`` alone"""
    for module in (k1_form, b8_form):
        tree = ast.parse(open(module.__file__, encoding="utf-8").read())
        imported = set()
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                imported.update(alias.name for alias in node.names)
            elif isinstance(node, ast.ImportFrom):
                imported.add(("." * node.level) + (node.module or ""))
        assert imported == {"collections"}, (os.path.basename(module.__file__), imported)
