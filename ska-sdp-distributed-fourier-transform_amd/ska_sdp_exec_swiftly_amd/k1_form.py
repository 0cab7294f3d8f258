"""
Which K1 a ``SwiftlyForward`` runs ("The K1 form"): one pure function from a record of facts to the
answer -- do the float32 (in a complex128 pass: float64) facets stay real, does K1 run the half-length transform of real rows,
and what is the axis-1-first mode.  No torch, no native library, no question to the core: ``SwiftlyForward._decide_k1`` gathers the facts,
``tests/test_k1_form_cpu.py`` holds the function to the answers recorded from the code it replaced.
"""
from collections import namedtuple

#: what the object decided: float32 facets stay float32 (float64 facets float64) / K1 is the half-length transform of real rows / the axis-1-first
#: mode -- 0: default order; 1: a row pass per wave (``core.finish_axis1_rows``); 2: the finish in the epilogue of the
#: whole-row K1 (``core.prepare_facet_window_rows``)
K1Answer = namedtuple("K1Answer", "facets_real half_length axis1_mode")

#: the facts.  ``axis1_first``: ``core.axis1_first`` (False / "rows" / True); ``keeps_real`` / ``axis1_fused``: the class
#: switches of ``SwiftlyForward``; ``real_facets`` / ``real_facets_rfft``: ``core.supports_*``; ``window_rows`` /
#: ``window_rows_real``: ``core.supports_window_rows`` of the band in question for complex / float32 rows;
#: ``rows_match_promoted`` / ``even`` / ``aligned``: of EVERY facet -- ``core._real_rows_match_promoted``, an even size at an
#: even position of the padded row, device rows 8-byte aligned at an even pitch; ``settled``: the answer the facets were
#: made resident by (None before that: the constructor's question); ``all_float64`` / ``float64_asked`` / ``real_facets_f64``:
#: the float64 twins of ``all_float32`` / ``float32_asked`` / ``real_facets`` (``core.supports_real_facets_f64``) -- at their
#: defaults the answers are those of the float32 facts alone
K1Facts = namedtuple("K1Facts", "wave_axis complex64 all_float32 float32_asked half_length_asked keeps_real axis1_first "
                     "axis1_fused planned real_facets real_facets_rfft window_rows window_rows_real rows_match_promoted even "
                     "aligned settled all_float64 float64_asked real_facets_f64",
                     defaults=(False, False, True, True, True, None, False, False, False))


def axis1_active(wave_axis, axis1_first, complex64):
    """does an object send blocks finished along axis 1 (either axis-1-first mode)?  A float32 accuracy mode of the
    contiguous-axis-first pipeline: complex128 runs the default order"""
    return wave_axis == 1 and bool(axis1_first) and complex64


def may_fuse(f):
    """is mode 2 open to these facts, window rows permitting?  ``axis1_first=True`` with a plan (the windows are its waves)"""
    return axis1_active(f.wave_axis, f.axis1_first, f.complex64) and f.axis1_first is True and f.axis1_fused and f.planned


def _mode(f, real):
    """the mode with the facets resident as float32 (``real``) or complex: 2 where the window rows exist -- the whole-row K1
    loads reals only for a caller who asked (``float32_asked``) --, else 1 or 0 as the axis-1-first pipeline is on or off"""
    rows = f.window_rows_real and f.float32_asked if real else f.window_rows
    return 2 if may_fuse(f) and rows else int(axis1_active(f.wave_axis, f.axis1_first, f.complex64))


def choose_k1(f):
    """``K1Facts`` -> ``K1Answer``.  Float32 facets stay float32 where the class allows it, the object stores the band along
    the contiguous axis first and a K1 that loads reals exists: the half-length form for a caller who asked, where the
    library has it, every facet can be loaded as pairs and neither residency leads to mode 2; else the real-load form of
    the row kernel where it gives the bits of the promoted rows -- in mode 2 only for a caller who asked, with aligned rows
    and the real window rows.  With the residency settled only the mode is open.

    Float64 facets stay float64 only for a caller who asked, in a complex128 pass that stores the band along the contiguous
    axis first, where the library has the float64-load K1: its values are those of the promoted rows at every size, there is no
    half-length form and complex128 runs the default order (mode 0)."""
    if f.settled is not None:
        return f.settled._replace(axis1_mode=_mode(f, f.settled.facets_real))
    if (f.keeps_real and f.wave_axis == 1 and not f.complex64 and f.all_float64 and f.float64_asked and f.real_facets_f64):
        return K1Answer(True, False, 0)
    may_stay = f.keeps_real and f.all_float32 and f.wave_axis == 1
    mode_c, mode_r = _mode(f, False), _mode(f, True)
    half = bool(may_stay and f.half_length_asked and f.real_facets_rfft and 2 not in (mode_c, mode_r) and f.even and f.aligned)
    real = half or bool(may_stay and f.real_facets and f.rows_match_promoted and
                        (mode_c != 2 or (f.float32_asked and f.aligned and mode_r == 2)))
    return K1Answer(real, half, mode_r if real else mode_c)
