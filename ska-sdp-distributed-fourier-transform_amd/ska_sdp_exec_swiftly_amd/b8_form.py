"""
Which B8 -- the contiguous-axis finish of the backward band pass -- a ``SwiftlyBackward`` runs ("The B8
form"): one pure function from a record of facts to the answer -- do the facets come back real, do the row kernels store
float32 themselves, does the finish take the half-length form.  No torch, no native library, no question to the core:
``SwiftlyBackward._decide_b8`` gathers the facts for its facets, ``DistributedBackward._coop_b8`` for one cooperative facet;
``tests/test_b8_form_cpu.py`` holds the function and both gatherers to the answers recorded from the code they replaced.
"""
from collections import namedtuple

#: what the object decided: the facets come back real / the row kernels store float32 and no complex facet is allocated
#: (``None`` while the schedule is unresolved) / the finish is the half-length form
B8Answer = namedtuple("B8Answer", "real_facets native half_length")

#: the facts.  ``resolved``: the schedule is fixed (``not _auto_axis``); ``facet_dtype``: what was asked for -- None, "float32",
#: "float64" or "complex"; ``real_facets_out`` / ``real_facets_out_c2r``: ``core.supports_*``; ``pairs``: EVERY facet in
#: question has an even size at an even position of the padded row (``facet_dtype.loads_as_pairs``);
#: ``accumulators_complex64``: of the band accumulators a finish is about to read -- None (open) for the properties, which
#: answer for the object before, between and after its accumulators; ``real_facets_out_f64``:
#: ``core.supports_real_facets_out_f64`` (the float64 store of the complex128 finish)
B8Facts = namedtuple("B8Facts", "resolved wave_axis facet_dtype half_length_asked real_facets_out real_facets_out_c2r pairs "
                     "accumulators_complex64 real_facets_out_f64", defaults=(None, False))


def choose_b8(f):
    """``B8Facts`` -> ``B8Answer``.  Real facets are stored by the row kernels on the band schedule, for float32 from
    complex64 accumulators and for float64 from complex128 ones, where the library has the real-store form; everywhere else
    each facet is finished complex and its real part copied out.  The half-length form for a caller who asked, where the finish is native, the library has the form
    and every facet can be stored as pairs."""
    real = f.facet_dtype in ("float32", "float64")
    if not f.resolved:
        return B8Answer(real, None, False)
    native = bool(f.wave_axis == 1 and (
        (f.facet_dtype == "float32" and f.real_facets_out and f.accumulators_complex64 is not False) or
        (f.facet_dtype == "float64" and f.real_facets_out_f64 and f.accumulators_complex64 is not True)))
    half = bool(native and f.facet_dtype == "float32" and f.half_length_asked and f.real_facets_out_c2r and f.pairs)
    return B8Answer(real, native, half)
