"""
The calls that run every instance of the band row kernel (``SWF_BAND_INSTANCES`` of csrc/row_pass.hip, the six whole-row
instances of csrc/row_whole.hip) through the C ABI: one table, read by tests/test_band_instance_cases_cpu.py (coverage of the
instance list and the chooser's answer for every case, without a GPU) and by tests/test_hip_band_instance_sweep_gpu.py (the
call itself against the complex128 oracle).  A plain module: no test, no fixture, no pytest setting.

A case is a dict:

``id``       name
``knob``     environment of the process that runs it: ``{}``, ``SWIFTLY_K1_WIN4`` = 0 / 1 or ``SWIFTLY_K1_WHOLE`` = 1 (read once
             per process by the library)
``kind``     the entry point: ``k1`` = swiftly_hip_prepare_facet_band(_real), ``window_rows`` =
             swiftly_hip_prepare_facet_window_rows, ``finish`` = swiftly_hip_finish_facet_band(_real), ``prepare_facet`` /
             ``prepare_subgrid`` = the plain primitives along the contiguous axis
``core``     key of ``CORES``; ``rows``; ``size`` (facet / subgrid size); ``off`` (facet / subgrid offset); ``band``; ``dtype``
             of the input rows (``c64`` / ``f32``) or ``real`` (float32 output of the finish); ``pitch`` and ``base``: the
             input rows are ``storage[rows, pitch][:, base : base + size]``; ``fold``: the window of the other axis
``call``     the ``BandCall`` (csrc/swiftly_rowinst.h) the launch site makes of these arguments, every field spelled out
``want``     the instance that must run: ``(geometry name, WIN, ST, PAIR, NSEG, CJ, W4, REAL, REAL_ST)``, or
             ``("whole", NSEG, ST)`` for the whole-row family
``seg_rot``  the rotation of the data segments the launcher must pass (``None`` where NSEG = 0)

The ``call`` of a case is written by the constructor of its kind, which restates the launch site: ``try_row_pass`` (plain
store of prepare_facet / prepare_subgrid: no window-table cache; mapped store of finish_facet_band: the handle's cache at
32768 points, none at 65536) and ``prepare_facet_k1`` (band store and window rows: the handle's cache).  A fresh
handle's cache always has a table to give (``table_available``), and compact twiddle sections exist at 32768 points only
(``has_twc``).
"""

GEOS = ["BandGeo16k", "BandGeo4", "BandGeo5", "BandGeo5Pre", "BandGeo5PreC", "BandGeo5C", "BandGeo64k", "BandGeoWhole"]

#: (W, N, xM, yN).  c15: the ``core64()`` sizes (m = 512, which the window-rows store needs); c14 / c16: ``params(14)`` /
#: ``params(16)`` of the facet sweep; s15 / s16: padded SUBGRIDS of 32768 / 65536 points, for prepare_subgrid (m = 512)
CORES = {
    "c14": (11.0, 32768, 256, 16384),
    "c15": (10.875, 65536, 1024, 32768),
    "c16": (11.0, 131072, 256, 65536),
    "s15": (11.0, 65536, 32768, 1024),
    "s16": (11.0, 131072, 65536, 1024),
}
DEFAULT, LEVEL0, LEVEL1, WHOLE = {}, {"SWIFTLY_K1_WIN4": "0"}, {"SWIFTLY_K1_WIN4": "1"}, {"SWIFTLY_K1_WHOLE": "1"}
#: row_pass_whole_stage_columns(), kWholeMaxWindows (tests/golden/band_instances.txt records them with every call)
STAGE_COLUMNS, MAX_WINDOWS = 12800, 256
#: the band and the waves of the window-rows cases: the four 512-column windows start 16 .. 4192 columns into the band
WINDOW_BAND, WINDOW_WAVES = (14720, 4736), (0, 928, -3 * 928, 6 * 928)
BAND15 = (10736, 11472)

CASES = []


def _levels(knob):
    return (int(knob.get("SWIFTLY_K1_WIN4", 2)), int(knob.get("SWIFTLY_K1_WHOLE", 0)))


def _call(knob, logn, cache, **fields):
    level, whole = _levels(knob)
    call = dict(logn=logn, ld_a=0, ld_len=0, ld_c=0, ld_mod=0, ld_win=0, band_sign=0, band_half=0, conj_ld=0, conj_st=0,
                accumulate=0, in_real=0, out_real=0, pitch_odd=0, base_align=0, win_full=0, win_logm=0, nwin=0, win_d=0,
                win_fn=0, win_tw_m=0, win_twc_m=0, win4_level=level, whole_enabled=whole, has_cache=int(cache),
                has_twc=int(cache and logn == 15), table_available=int(cache), stage_columns=STAGE_COLUMNS,
                max_windows=MAX_WINDOWS)
    assert set(fields) <= set(call)
    call.update(fields)
    return call


def _add(cid, knob, kind, want, seg_rot, call, **args):
    assert (seg_rot is not None) == (want[-2 if want[0] == "whole" else 4] != 0), cid
    assert cid not in {c["id"] for c in CASES}, cid
    CASES.append(dict(id=cid, knob=knob, kind=kind, want=tuple(want), seg_rot=seg_rot, call=call, **args))


def _facet_load(core, size, off):
    """facet_in_padded_facet (csrc/swiftly_geometry.h)"""
    yN = CORES[core][3]
    return dict(ld_a=(-(off + yN // 2 - size // 2)) % yN, ld_len=size, ld_c=0, ld_mod=size)


def band_half(length):
    return ((length + 1) // 2 + 15) // 16 * 16


def k1(cid, knob, want, seg_rot, core, size, off, dtype="c64", rows=7, band=None, pitch=None, base=0, fold=False):
    """prepare_facet_band(_real): prepare_facet_k1 -- load window, band store, both conjugations, the cache"""
    yN = CORES[core][3]
    band = band or {"c14": (5461, 5477), "c15": BAND15, "c16": (21845, 21861)}[core]
    pitch = pitch or size
    itemsize = 4 if dtype == "f32" else 8
    call = _call(knob, yN.bit_length() - 1, True, ld_win=1, band_sign=1, band_half=band_half(band[1]), conj_ld=1, conj_st=1,
                 in_real=int(dtype == "f32"), pitch_odd=pitch & 1, base_align=(base * itemsize) & 15, **_facet_load(core, size, off))
    _add(cid, knob, "k1", want, seg_rot, call, core=core, rows=rows, size=size, off=off, band=band, dtype=dtype, pitch=pitch,
         base=base, fold=fold)


def window_rows(cid, want, seg_rot, size, off, rows=7):
    """prepare_facet_window_rows on the c15 core: the k1 call with the window group"""
    call = _call(DEFAULT, 15, True, ld_win=1, band_sign=1, band_half=band_half(WINDOW_BAND[1]), conj_ld=1, conj_st=1, win_full=1,
                 win_logm=9, nwin=len(WINDOW_WAVES), win_d=1, win_fn=1, win_tw_m=1, win_twc_m=1, **_facet_load("c15", size, off))
    _add(cid, DEFAULT, "window_rows", want, seg_rot, call, core="c15", rows=rows, size=size, off=off, band=WINDOW_BAND,
         waves=WINDOW_WAVES, dtype="c64", pitch=size, base=0, fold=False)


def finish(cid, knob, want, seg_rot, core, band, real=False, rows=7, size=None, off=0):
    """finish_facet_band(_real): try_row_pass -- band_as_load_map, no load window, mapped store, no conjugation; contiguous
    band rows (pitch = band length)"""
    yN = CORES[core][3]
    logn = yN.bit_length() - 1
    size = size or 11 * yN // 16
    call = _call(knob, logn, logn == 15, ld_a=(-band[0]) % yN, ld_len=band[1], ld_c=0, ld_mod=band[1], band_sign=-1,
                 out_real=int(real), pitch_odd=band[1] & 1)
    _add(cid, knob, "finish", want, seg_rot, call, core=core, rows=rows, size=size, off=off, band=band, real=real)


def prepare_facet(cid, want, core, size, off, rows=7):
    """swiftly_hip_prepare_facet along the contiguous axis: try_row_pass -- load window, plain store, no cache"""
    yN = CORES[core][3]
    call = _call(DEFAULT, yN.bit_length() - 1, False, ld_win=1, conj_ld=1, conj_st=1, pitch_odd=size & 1, **_facet_load(core, size, off))
    _add(cid, DEFAULT, "prepare_facet", want, None, call, core=core, rows=rows, size=size, off=off)


def prepare_subgrid(cid, want, core, size, off, rows=7):
    """swiftly_hip_prepare_subgrid along the contiguous axis: try_row_pass on xM points -- subgrid_in_padded_subgrid, no
    window, no conjugation, plain store, no cache"""
    xM = CORES[core][2]
    call = _call(DEFAULT, xM.bit_length() - 1, False, ld_a=(-(xM // 2 - size // 2 + off)) % xM, ld_len=size, ld_c=0, ld_mod=size,
                 pitch_odd=size & 1)
    _add(cid, DEFAULT, "prepare_subgrid", want, None, call, core=core, rows=rows, size=size, off=off)


# ----------------------------------------------------------------------------------------------------------------------
# forward K1 at 32768 points with its empty segments compiled out.  The data start at transform input (off - size / 2) mod
# yN: (size, off) = (16384, 8192) / (22528, 11264) / (24576, 12288) put them at input 0 -- 16 / 22 / 24 segments from
# segment 0 --; off = 0 puts 16384 points at segment 24 and 22528 points at segment 21, both wrapping the end of the row;
# 22528 points at off = 2 start two points into segment 21 and touch 23 segments from there on.
K1_SEGMENTS = [(16, 0, 16384, 8192), (16, 24, 16384, 0), (22, 0, 22528, 11264), (22, 21, 22528, 0), (24, 0, 24576, 12288),
               (24, 21, 22528, 2)]
for ns, rot, size, off in K1_SEGMENTS:
    tag = f"{ns}-rot{rot}"
    # default: window table + compact twiddles for complex rows and for real rows that take 8-byte loads; real rows at an odd
    # pitch from a 4-byte-aligned base load 4 bytes at a time and never take the table
    k1(f"k1-prec-{tag}-c64", DEFAULT, ("BandGeo5PreC", 1, 1, 1, ns, 1, 1, 0, 0), rot, "c15", size, off,
       rows=17 if (ns, rot) == (22, 0) else 7, fold=rot == 0)
    k1(f"k1-prec-{tag}-f32", DEFAULT, ("BandGeo5PreC", 1, 1, 1, ns, 1, 1, 1, 0), rot, "c15", size, off, dtype="f32", fold=rot != 0)
    k1(f"k1-pre-{tag}-f32x4", DEFAULT, ("BandGeo5Pre", 1, 1, 1, ns, 1, 0, 2, 0), rot, "c15", size, off, dtype="f32", pitch=size + 3, base=1)
    # SWIFTLY_K1_WIN4=0: the plain window loads
    k1(f"k1-pre-{tag}-c64-level0", LEVEL0, ("BandGeo5Pre", 1, 1, 1, ns, 1, 0, 0, 0), rot, "c15", size, off,
       rows=17 if (ns, rot) == (24, 21) else 7, fold=rot != 0)
    k1(f"k1-pre-{tag}-f32-level0", LEVEL0, ("BandGeo5Pre", 1, 1, 1, ns, 1, 0, 1, 0), rot, "c15", size, off, dtype="f32")
    # SWIFTLY_K1_WIN4=1: the window table alone, a complex instance only
    k1(f"k1-pre-w4-{tag}-c64-level1", LEVEL1, ("BandGeo5Pre", 1, 1, 1, ns, 1, 1, 0, 0), rot, "c15", size, off, fold=rot == 0)
    # SWIFTLY_K1_WHOLE=1: the band store of the whole-row kernel
    k1(f"k1-whole-{tag}-c64", WHOLE, ("whole", ns, 1), rot, "c15", size, off, rows=17 if (ns, rot) == (16, 24) else 7, fold=rot == 0)
k1("k1-pre-22-rot21-f32-level1", LEVEL1, ("BandGeo5Pre", 1, 1, 1, 22, 1, 0, 1, 0), 21, "c15", 22528, 0, dtype="f32")
# ... and every segment: 26624 points cover 26 or 27 of 32; without adjacent-point loads: an odd facet shift, or complex rows
# at an odd pitch
k1("k1-all-c64", DEFAULT, ("BandGeo5", 1, 1, 1, 0, -1, 0, 0, 0), None, "c15", 26624, 0, rows=17)
k1("k1-all-c64-off666", DEFAULT, ("BandGeo5", 1, 1, 1, 0, -1, 0, 0, 0), None, "c15", 26624, 666, fold=True)
k1("k1-all-f32", DEFAULT, ("BandGeo5", 1, 1, 1, 0, -1, 0, 1, 0), None, "c15", 26624, 0, dtype="f32")
k1("k1-all-f32x4", DEFAULT, ("BandGeo5", 1, 1, 1, 0, -1, 0, 2, 0), None, "c15", 26624, 666, dtype="f32", pitch=26627, base=1)
k1("k1-odd-shift-c64", DEFAULT, ("BandGeo5", 1, 1, 0, 0, -1, 0, 0, 0), None, "c15", 22528, 11265, band=(32001, 2049))
k1("k1-odd-pitch-c64", DEFAULT, ("BandGeo5", 1, 1, 0, 0, -1, 0, 0, 0), None, "c15", 22528, 11264, pitch=22529, fold=True)
k1("k1-odd-shift-f32", DEFAULT, ("BandGeo5", 1, 1, 0, 0, -1, 0, 1, 0), None, "c15", 22528, 4097, dtype="f32", band=(0, 32768))
k1("k1-odd-shift-f32x4", DEFAULT, ("BandGeo5", 1, 1, 0, 0, -1, 0, 1, 0), None, "c15", 22528, 11265, dtype="f32", pitch=22531, base=1)

# window-rows store of the whole-row kernel: 352-point facets for 16 segments (at input 0: one segment; at off = 0 the data
# start 176 points before the end of the row: segments 31 and 0), facets of the 22528-point class for 22 and 24 -- 22532 points
# from input 0 on touch 23 segments.  The bound of this store (2.5e-6) belongs to that class: the rows hold one 512-column
# window of a transform whose float32 rounding is relative to the whole row, and the row grows with the largest 1 / PSWF of the
# facet, 85 at 22528 points and 239 at 24576.  Rounding noise of K1's size (1.9e-7 of the row's RMS) put through the oracle's
# extract_from_facet -> add_to_subgrid gives 1.6e-6 of the window rows at 22528 points and 3.3e-6 at 24576 (measured: 1.4e-6 and
# 2.7e-6), so the 24-segment instance gets its rotation 0 from 22532 points and not from the 24576 of the band-store cases.
window_rows("winrows-16-rot0", ("whole", 16, 3), 0, 352, 176)
window_rows("winrows-16-rot31", ("whole", 16, 3), 31, 352, 0, rows=17)
window_rows("winrows-22-rot0", ("whole", 22, 3), 0, 22528, 11264)
window_rows("winrows-22-rot21", ("whole", 22, 3), 21, 22528, 0)
window_rows("winrows-24-rot0", ("whole", 24, 3), 0, 22532, 11266)
window_rows("winrows-24-rot21", ("whole", 24, 3), 21, 22528, 2)

# backward finish at 32768 points.  The band's data start at transform input (yN / 2 - band start) mod yN: a band that
# starts at column 16384 puts them at input 0, one that starts at column 0 at segment 16.  11488 columns are 12 segments, 15000
# are 15; the compact twiddle sections (BandGeo5C) at the default level, the plain table at levels 0 and 1
for ns, length in ((13, 11488), (16, 15000)):
    for rot, start in ((0, 16384), (16, 0)):
        for real in (False, True):
            tag = f"{ns}-rot{rot}-{'real' if real else 'c64'}"
            finish(f"finish-5c-{tag}", DEFAULT, ("BandGeo5C", 0, 2, 1, ns, 0, 0, 0, int(real)), rot, "c15", (start, length), real=real,
                   rows=17 if (ns, rot, real) == (13, 16, False) else 7, off=22528 if rot else 0)
            finish(f"finish-5-{tag}-level0", LEVEL0, ("BandGeo5", 0, 2, 1, ns, 0, 0, 0, int(real)), rot, "c15", (start, length), real=real,
                   off=0 if rot else -22528)
finish("finish-5-13-rot16-c64-level1", LEVEL1, ("BandGeo5", 0, 2, 1, 13, 0, 0, 0, 0), 16, "c15", (0, 11488))
finish("finish-5-16-rot0-real-level1", LEVEL1, ("BandGeo5", 0, 2, 1, 16, 0, 0, 0, 1), 0, "c15", (16384, 15000), real=True)
# 13 segments: the same band from input 1000 on (segments 0 .. 12), and 12400 columns from 1022 points before the end of the row
finish("finish-5c-13-unaligned-c64", DEFAULT, ("BandGeo5C", 0, 2, 1, 13, 0, 0, 0, 0), 0, "c15", (17384, 11488), off=3 * 352)
finish("finish-5c-13-unaligned-wrap-real", DEFAULT, ("BandGeo5C", 0, 2, 1, 13, 0, 0, 0, 1), 31, "c15", (15362, 12400), real=True, off=3 * 352)
# more than 16 segments: the full band; no adjacent-point loads: an odd band start, an odd band length (= an odd pitch)
finish("finish-5-full-c64", DEFAULT, ("BandGeo5", 0, 2, 1, 0, -1, 0, 0, 0), None, "c15", (0, 32768), rows=17, off=-22528)
finish("finish-5-full-real", DEFAULT, ("BandGeo5", 0, 2, 1, 0, -1, 0, 0, 1), None, "c15", (0, 32768), real=True)
finish("finish-5-odd-start-c64", DEFAULT, ("BandGeo5", 0, 2, 0, 0, -1, 0, 0, 0), None, "c15", (8193, 15000), off=3 * 352)
finish("finish-5-odd-length-c64", DEFAULT, ("BandGeo5", 0, 2, 0, 0, -1, 0, 0, 0), None, "c15", (31744, 7169))
finish("finish-5-odd-start-real", DEFAULT, ("BandGeo5", 0, 2, 0, 0, -1, 0, 0, 1), None, "c15", (8193, 15000), real=True)
finish("finish-5-odd-length-real", DEFAULT, ("BandGeo5", 0, 2, 0, 0, -1, 0, 0, 1), None, "c15", (31744, 7169), real=True, off=22528)

# plain store at 32768 points (1024 x 16): prepare_facet with its window, prepare_subgrid -- the one primitive that loads
# through a prepare_* map without a window -- on a padded subgrid of 32768 points
prepare_facet("prepare-facet-32768", ("BandGeo4", 1, 0, 0, 0, -1, 0, 0, 0), "c15", 22528, 11264, rows=17)
prepare_facet("prepare-facet-32768-odd", ("BandGeo4", 1, 0, 0, 0, -1, 0, 0, 0), "c15", 22529, -4097)
prepare_subgrid("prepare-subgrid-32768", ("BandGeo4", 0, 0, 0, 0, -1, 0, 0, 0), "s15", 22528, 5 * 64)
prepare_subgrid("prepare-subgrid-32768-odd", ("BandGeo4", 0, 0, 0, 0, -1, 0, 0, 0), "s15", 9999, -7 * 64)

# 16384 points: the band store is the only form that reaches the band row kernel
k1("k1-16k-c64", DEFAULT, ("BandGeo16k", 1, 1, 0, 0, -1, 0, 0, 0), None, "c14", 11264, 0, rows=17, fold=True)
k1("k1-16k-c64-odd", DEFAULT, ("BandGeo16k", 1, 1, 0, 0, -1, 0, 0, 0), None, "c14", 11264, 2341, band=(0, 16384))
k1("k1-16k-f32", DEFAULT, ("BandGeo16k", 1, 1, 0, 0, -1, 0, 1, 0), None, "c14", 11264, -3072, dtype="f32")
k1("k1-16k-f32-odd-pitch", DEFAULT, ("BandGeo16k", 1, 1, 0, 0, -1, 0, 1, 0), None, "c14", 11264, 2341, dtype="f32", pitch=11267, base=1, fold=True)

# 65536 points: 45056 points at input 0 are 44 segments from segment 0, at off = 0 from segment 42 (wrapping); 47000 points are
# more than 44
for dtype, real in (("c64", 0), ("f32", 1)):
    k1(f"k1-64k-44-rot0-{dtype}", DEFAULT, ("BandGeo64k", 1, 1, 0, 44, 1, 0, real, 0), 0, "c16", 45056, 22528, dtype=dtype, fold=not real)
    k1(f"k1-64k-44-rot42-{dtype}", DEFAULT, ("BandGeo64k", 1, 1, 0, 44, 1, 0, real, 0), 42, "c16", 45056, 0, dtype=dtype,
       rows=17 if real else 7, band=(0, 65536) if real else None)
    k1(f"k1-64k-all-{dtype}", DEFAULT, ("BandGeo64k", 1, 1, 0, 0, -1, 0, real, 0), None, "c16", 47000, 512 * (3 + real), dtype=dtype, fold=bool(real))
prepare_facet("prepare-facet-65536", ("BandGeo64k", 1, 0, 0, 0, -1, 0, 0, 0), "c16", 45056, 22528)
prepare_facet("prepare-facet-65536-odd", ("BandGeo64k", 1, 0, 0, 0, -1, 0, 0, 0), "c16", 45057, -5 * 512 - 1)
prepare_subgrid("prepare-subgrid-65536", ("BandGeo64k", 0, 0, 0, 0, -1, 0, 0, 0), "s16", 45056, 3 * 128)
prepare_subgrid("prepare-subgrid-65536-odd", ("BandGeo64k", 0, 0, 0, 0, -1, 0, 0, 0), "s16", 20001, -9 * 128)
finish("finish-64k-c64", DEFAULT, ("BandGeo64k", 0, 2, 0, 0, -1, 0, 0, 0), None, "c16", (22528, 22536), off=45056)
finish("finish-64k-c64-wrap", DEFAULT, ("BandGeo64k", 0, 2, 0, 0, -1, 0, 0, 0), None, "c16", (59392, 14337), off=-512)
finish("finish-64k-real", DEFAULT, ("BandGeo64k", 0, 2, 0, 0, -1, 0, 0, 1), None, "c16", (22528, 22536), real=True)
finish("finish-64k-real-full", DEFAULT, ("BandGeo64k", 0, 2, 0, 0, -1, 0, 0, 1), None, "c16", (0, 65536), real=True, off=45056)

#: instances of SWF_BAND_INSTANCES that no exported entry point reaches, each with the launch-site condition that excludes it
#: (csrc/swiftly_abi.hip: try_row_pass sends only 32768- and 65536-point rows to the band row kernel; the one band-store call
#: site, prepare_facet_k1, always passes the facet window)
NOT_REACHABLE_THROUGH_THE_ABI = {
    ("BandGeo16k", 0, 0, 0, 0, -1, 0, 0, 0): "try_row_pass runs the plain store of 16384-point rows on the lean single-workgroup kernel (launch_row_pass)",
    ("BandGeo16k", 1, 0, 0, 0, -1, 0, 0, 0): "try_row_pass runs the plain store of 16384-point rows, windowed or not, on the lean single-workgroup kernel",
    ("BandGeo16k", 0, 2, 0, 0, -1, 0, 0, 0): "try_row_pass runs the mapped store of 16384-point rows (finish_facet_band) on the lean single-workgroup kernel",
    ("BandGeo16k", 0, 1, 0, 0, -1, 0, 0, 0): "the band store is launched by prepare_facet_k1 only, which always sets ld_win to the facet window",
    ("BandGeo5", 0, 1, 0, 0, -1, 0, 0, 0): "the band store is launched by prepare_facet_k1 only, which always sets ld_win (here: an odd shift or pitch)",
    ("BandGeo5", 0, 1, 1, 0, -1, 0, 0, 0): "the band store is launched by prepare_facet_k1 only, which always sets ld_win (here: adjacent-point loads)",
    ("BandGeo64k", 0, 1, 0, 0, -1, 0, 0, 0): "the band store is launched by prepare_facet_k1 only, which always sets ld_win (here: 65536-point rows)",
}


def instance_key(want):
    """``want`` as the CPU test names instances: TEMPLATE tuple with the geometry's number, or (nseg, st) of the whole-row family"""
    return tuple(want[1:]) if want[0] == "whole" else (GEOS.index(want[0]),) + tuple(want[1:])


def cases_of(knob):
    return [c for c in CASES if c["knob"] == knob]
