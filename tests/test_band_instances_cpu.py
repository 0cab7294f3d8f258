"""
Which instance of the band row kernel a call runs (csrc/swiftly_rowinst.h, ``choose_band_instance``), without a GPU:
``tests/native/band_instance_dump.cpp`` includes only that header and prints what it answers; this test compiles it with the
compiler of the library's host code.

Expectations: ``tests/golden/band_instances.txt`` holds calls and the answers RECORDED from the dispatch this header
replaced (the launch ladders of csrc/row_pass.hip and csrc/row_whole.hip before it, run on the CPU with a launch function that
prints the kernel's name, grid and arguments instead of launching) -- one line per distinct (knobs, cache state, row type,
instance, rotation) and per distinct refusal that a grid of 1.5 million recorded calls met.  A line is
``<the 29 BandCall fields> -> <the 18 BandInst fields>``, in the order of the dump program; a refused call's table key is
``-``: the recording does not show whether a window table was requested before the refusal.
"""
import os
import re
import subprocess

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ska-sdp-distributed-fourier-transform_amd", "csrc")

CALL = ("logn ld_a ld_len ld_c ld_mod ld_win band_sign band_half conj_ld conj_st accumulate in_real out_real pitch_odd base_align "
        "win_full win_logm nwin win_d win_fn win_tw_m win_twc_m win4_level whole_enabled has_cache has_twc table_available "
        "stage_columns max_windows").split()
INST = "status family geo win st pair nseg cj w4 real real_st seg_rot ld_win4 twc key_c key_ns key_n key_seglen".split()
#: BandGeoId, and the geometries that are BandGeo5 with another twiddle path (same factorisation, same numbers)
GEOS = ["BandGeo16k", "BandGeo4", "BandGeo5", "BandGeo5Pre", "BandGeo5PreC", "BandGeo5C", "BandGeo64k", "BandGeoWhole"]
BASE_GEO = {"BandGeo5Pre": "BandGeo5", "BandGeo5PreC": "BandGeo5", "BandGeo5C": "BandGeo5"}
TEMPLATE = ("geo", "win", "st", "pair", "nseg", "cj", "w4", "real", "real_st")


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """the compiled program as a function: list of request lines -> list of answer lines"""
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC\s*\?=\s*(\S+)", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1)
    exe = str(tmp_path_factory.mktemp("band_instances") / "band_instance_dump")
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "band_instance_dump.cpp"), "-o", exe], check=True, timeout=300)

    def run(requests):
        res = subprocess.run([exe], input="\n".join(requests) + "\n", stdout=subprocess.PIPE, text=True, check=True, timeout=120)
        return res.stdout.splitlines()

    return run


@pytest.fixture(scope="module")
def golden():
    """[(call dict, answer dict)]; a ``-`` of the file is None"""
    rows = []
    with open(os.path.join(ROOT, "tests", "golden", "band_instances.txt"), encoding="utf-8") as fh:
        for line in fh:
            call, answer = (side.split() for side in line.split("->"))
            assert len(call) == len(CALL) and len(answer) == len(INST), line
            rows.append((dict(zip(CALL, map(int, call))), {k: None if v == "-" else int(v) for k, v in zip(INST, answer)}))
    assert 1000 < len(rows) < 5000
    return rows


def choose(dump, calls):
    answers = dump(["band " + " ".join(str(c[k]) for k in CALL) for c in calls])
    assert len(answers) == len(calls)
    return [dict(zip(INST, map(int, line.split()))) for line in answers]


def instance_list():
    """the X(...) entries of SWF_BAND_INSTANCES in row_pass.hip, as TEMPLATE tuples"""
    with open(os.path.join(CSRC, "row_pass.hip"), encoding="utf-8") as fh:
        text = fh.read()
    found = re.findall(r"^#define\s+SWF_BAND_INSTANCES\(X\)((?:.*\\\n)*.*)$", text, flags=re.M)
    assert len(found) == 1
    body = re.sub(r"/\*.*?\*/", "", found[0], flags=re.S)
    entries = re.findall(r"X\(\s*(\w+)((?:\s*,\s*-?\d+){8})\s*\)", body)
    assert len(entries) == body.count("X(")
    insts = [(GEOS.index(g),) + tuple(int(v) for v in rest.split(",")[1:]) for g, rest in entries]
    assert insts and len(set(insts)) == len(insts)
    return insts


def test_golden_answers(dump, golden):
    got = choose(dump, [c for c, _ in golden])
    for (call, want), have in zip(golden, got):
        assert {k: have[k] for k, v in want.items() if v is not None} == {k: v for k, v in want.items() if v is not None}, call
        if want["status"] == 0:
            assert None not in want.values()
            # what a chosen instance implies for the launcher's arguments
            assert have["ld_win4"] == (have["key_ns"] != 0) and (have["key_ns"] == 0 or have["key_ns"] == have["nseg"])
            assert have["w4"] <= have["ld_win4"]
    # what the file has to hold: both refusals, every knob setting, a cache that is absent / answers / is full
    assert {w["status"] for _, w in golden} == {0, -1, -2}
    for status in (0, -1, -2):
        seen = {(c["win4_level"], c["whole_enabled"]) for c, w in golden if w["status"] == status}
        assert seen == {(level, whole) for level in (0, 1, 2) for whole in (0, 1)}
        caches = {(c["has_cache"], c["table_available"]) for c, w in golden if w["status"] == status}
        assert caches == {(0, 0), (1, 1), (1, 0)}
    # every distinct refusal is there on its own: a line that meets that condition and no other of its list
    runs = [int(line.split()[0]) for line in dump([f"run {c['ld_a']} {c['ld_len']} {1 << min(c['logn'], 16)} 1024" for c, _ in golden])]

    def alone(status, rows, conditions):
        for name, cond in conditions.items():
            assert any(w["status"] == status and cond(c, run) and not any(o(c, run) for k, o in conditions.items() if k != name)
                       for (c, w), run in rows), name

    alone(-1, [(g, r) for g, r in zip(golden, runs) if not g[0]["in_real"] and not g[0]["out_real"] and not g[0]["win_full"]],
          {"8192 points": lambda c, run: c["logn"] == 13, "131072 points": lambda c, run: c["logn"] == 17})
    alone(-1, [(g, r) for g, r in zip(golden, runs) if g[0]["in_real"]], {
        "no load window": lambda c, run: not c["ld_win"], "plain store": lambda c, run: c["band_sign"] == 0,
        "mapped store": lambda c, run: c["band_sign"] < 0, "window rows": lambda c, run: c["win_full"],
        "ld_c": lambda c, run: c["ld_c"] != 0, "ld_mod": lambda c, run: c["ld_mod"] != c["ld_len"],
        "8192 points": lambda c, run: c["logn"] == 13, "131072 points": lambda c, run: c["logn"] == 17})
    alone(-1, [(g, r) for g, r in zip(golden, runs) if g[0]["out_real"] and not g[0]["in_real"]], {
        "plain store": lambda c, run: c["band_sign"] == 0, "band store": lambda c, run: c["band_sign"] > 0,
        "window rows": lambda c, run: c["win_full"], "8192 points": lambda c, run: c["logn"] == 13,
        "16384 points": lambda c, run: c["logn"] == 14,  # no real store in the 16 points per lane geometry
        "131072 points": lambda c, run: c["logn"] == 17,
        "accumulate, 32768": lambda c, run: c["accumulate"] and c["logn"] != 16,
        "accumulate, 65536": lambda c, run: c["accumulate"] and c["logn"] != 15})
    alone(-2, [(g, r) for g, r in zip(golden, runs) if g[0]["win_full"] and not g[0]["in_real"] and not g[0]["out_real"]], {
        "16384 points": lambda c, run: c["logn"] < 15, "65536 points": lambda c, run: c["logn"] > 15,
        "window length": lambda c, run: c["win_logm"] != 9, "no windows": lambda c, run: c["nwin"] <= 0,
        "no window offsets": lambda c, run: not c["win_d"], "plain store": lambda c, run: c["band_sign"] == 0,
        "mapped store": lambda c, run: c["band_sign"] < 0, "odd shift": lambda c, run: c["ld_a"] & 1, "odd length": lambda c, run: c["ld_len"] & 1,
        "odd pitch": lambda c, run: c["pitch_odd"], "8-byte base": lambda c, run: c["base_align"] == 8,
        "4-byte base": lambda c, run: c["base_align"] == 4, "no load window": lambda c, run: not c["ld_win"],
        "forward transform": lambda c, run: not c["conj_ld"] and not c["conj_st"], "one conjugation": lambda c, run: c["conj_ld"] != c["conj_st"],
        "more than 24 data segments": lambda c, run: c["logn"] == 15 and run > 24, "no cache": lambda c, run: not c["has_cache"],
        "plain window loads": lambda c, run: c["win4_level"] == 0, "no compact twiddles by the knob": lambda c, run: c["win4_level"] == 1,
        "cache full": lambda c, run: c["has_cache"] and not c["table_available"],
        "no compact twiddles": lambda c, run: c["has_cache"] and not c["has_twc"],
        "too many windows": lambda c, run: c["nwin"] > c["max_windows"], "no Fn": lambda c, run: not c["win_fn"],
        "no m-point twiddles": lambda c, run: not c["win_tw_m"], "no compact m-point twiddles": lambda c, run: not c["win_twc_m"],
        "band too wide to stage": lambda c, run: 2 * c["band_half"] > c["stage_columns"]})
    assert all(c["win_full"] and not c["in_real"] and not c["out_real"] for c, w in golden if w["status"] == -2)


def test_the_instance_list_is_what_the_chooser_names(golden):
    chosen = {tuple(w[k] for k in TEMPLATE) for _, w in golden if w["status"] == 0 and w["family"] == 0}
    assert chosen == set(instance_list())
    assert len(chosen) == 54
    whole = {(w["nseg"], w["st"]) for _, w in golden if w["status"] == 0 and w["family"] == 1}
    assert whole == {(ns, st) for ns in (16, 22, 24) for st in (1, 3)}  # the instances of row_whole.hip: band store, window rows
    # the instances no call reaches are not instantiated: the 1024 x 16 geometry is the plain store's only, and only its
    assert {(i[1], i[2], i[3]) for i in instance_list() if GEOS[i[0]] == "BandGeo4"} == {(0, 0, 0), (1, 0, 0)}
    assert not [i for i in instance_list() if GEOS[i[0]] == "BandGeo5" and i[2] == 0]


def test_every_instance_has_an_oracle_case_or_a_reason():
    """tests/band_instance_cases.py (what tests/test_hip_band_instance_sweep_gpu.py runs against the oracle) leaves out no
    instance of the list and of the whole-row family, except those it names as unreachable through the C ABI"""
    import band_instance_cases as bic

    assert bic.GEOS == GEOS
    run = {bic.instance_key(c["want"]) for c in bic.CASES}
    unreachable = {bic.instance_key(k) for k in bic.NOT_REACHABLE_THROUGH_THE_ABI}
    assert all(len(why.split()) > 5 for why in bic.NOT_REACHABLE_THROUGH_THE_ABI.values())
    everything = set(instance_list()) | {(ns, st) for ns in (16, 22, 24) for st in (1, 3)}
    assert run | unreachable == everything, (sorted(everything - run - unreachable), sorted((run | unreachable) - everything))
    assert not run & unreachable
    print(f"band row kernel instances: {len(run)} with an oracle case, {len(unreachable)} unreachable, {len(everything)} in all")
    assert (len(run), len(unreachable), len(everything)) == (53, 7, 60)
    # every instance with compiled-out segments at a rotation of 0 and at another one (the data wrap the end of the row)
    for key in run:
        rots = {c["seg_rot"] for c in bic.CASES if bic.instance_key(c["want"]) == key}
        if key[4 if len(key) > 2 else 0] != 0:
            assert 0 in rots and rots - {0}, (key, rots)
        else:
            assert rots == {None}, key
    # 7 rows (not a multiple of the 8 rows of a workgroup group) everywhere, 17 rows (three groups) once per geometry
    assert {c["rows"] for c in bic.CASES} == {7, 17}
    assert {c["want"][0] for c in bic.CASES if c["rows"] == 17} == set(GEOS[:-1]) | {"whole"}
    assert {tuple(sorted(c["knob"].items())) for c in bic.CASES} == {(), (("SWIFTLY_K1_WIN4", "0"),), (("SWIFTLY_K1_WIN4", "1"),),
                                                                     (("SWIFTLY_K1_WHOLE", "1"),)}


def test_every_case_runs_the_instance_the_chooser_names(dump):
    """the expectation of every case against ``choose_band_instance`` for the BandCall the case spells out; and the maps of
    that BandCall against the closed forms of the entry point's arguments"""
    import band_instance_cases as bic

    got = choose(dump, [c["call"] for c in bic.CASES])
    for case, have in zip(bic.CASES, got):
        call, want = case["call"], case["want"]
        assert have["status"] == 0, case["id"]
        if want[0] == "whole":
            assert (have["family"], GEOS[have["geo"]], have["nseg"], have["st"]) == (1, "BandGeoWhole") + tuple(want[1:]), case["id"]
        else:
            assert have["family"] == 0 and (GEOS[have["geo"]],) + tuple(have[k] for k in TEMPLATE[1:]) == tuple(want), (case["id"], have)
        if case["seg_rot"] is not None:
            assert have["seg_rot"] == case["seg_rot"], (case["id"], have["seg_rot"])
            # the first data segment, counted on the padded row: transform input j holds element (j + n/2 + ld_a) mod n
            n = 1 << call["logn"]
            q = (numpy.arange(n) + n // 2 + call["ld_a"]) % n
            has = (q < call["ld_len"]).reshape(-1, 1024).any(axis=1)
            assert has[case["seg_rot"]] and not has[case["seg_rot"] - 1] and has.sum() <= have["nseg"], case["id"]
        # the knob level decides the window path
        level = int(case["knob"].get("SWIFTLY_K1_WIN4", 2))
        assert call["win4_level"] == level and call["whole_enabled"] == int(case["knob"].get("SWIFTLY_K1_WHOLE", 0))
        assert call["table_available"] == call["has_cache"] and call["has_twc"] == (call["has_cache"] and call["logn"] == 15)
        assert have["ld_win4"] <= (level > 0) and have["twc"] <= (level > 1)
        # the load map from the arguments: where pixel 0 of the facet / subgrid / band lies on the padded axis
        W, N, xM, yN = bic.CORES[case["core"]]
        n = xM if case["kind"] == "prepare_subgrid" else yN
        assert n == 1 << call["logn"]
        first = case["band"][0] if case["kind"] == "finish" else (n // 2 - case["size"] // 2 + case["off"]) % n
        assert (first + call["ld_a"]) % n == 0, case["id"]
        assert call["ld_len"] == (case["band"][1] if case["kind"] == "finish" else case["size"]) == call["ld_mod"]


def test_last_band_instance_without_a_launch():
    """``swiftly_hip_last_band_instance`` needs no device; the record and the counter belong to the calling thread: a
    thread that never launched reads 0 and a default BandInst"""
    import ctypes
    import threading

    from ska_sdp_exec_swiftly_amd import _lib

    lib = _lib.load()
    seen = {}

    def ask():
        for n in (18, 5, 40, 0):
            buf = (ctypes.c_int32 * 20)(*([77] * 20))
            seen[n] = (lib.swiftly_hip_last_band_instance(buf, n), list(buf))
        seen["null"] = lib.swiftly_hip_last_band_instance(None, 18)

    thread = threading.Thread(target=ask)
    thread.start()
    thread.join()
    default = dict(zip(INST, [0] * 18), cj=-1)
    assert seen["null"] == 0
    for n, (count, buf) in ((k, v) for k, v in seen.items() if k != "null"):
        assert count == 0
        assert buf[: min(n, 18)] == [default[k] for k in INST][: min(n, 18)] and set(buf[min(n, 18) :]) == {77}, (n, buf)


def test_real_rows_get_the_instance_of_the_promoted_row(dump, golden):
    """A real call -- whatever its pitch and base -- against the complex call for the same row promoted to a contiguous,
    aligned complex64 copy: same geometry, pair loads, segment count, conjugations and rotation.  The window path may
    differ in two named cases only."""
    calls = [c for c, _ in golden if not c["in_real"] and not c["out_real"] and not c["win_full"] and c["ld_win"] and c["band_sign"] > 0
             and c["ld_c"] == 0 and c["ld_mod"] == c["ld_len"] and c["logn"] in (14, 15, 16)]
    assert len(calls) > 100
    # ... real rows at an even pitch and 16-byte base, an odd pitch, a 4-byte and an 8-byte base
    calls = [dict(c, pitch_odd=po, base_align=al) for c in calls for po, al in ((0, 0), (1, 0), (0, 4), (0, 8))]
    promoted = choose(dump, [dict(c, pitch_odd=0, base_align=0, whole_enabled=0) for c in calls])
    real = choose(dump, [dict(c, in_real=1) for c in calls])
    base = lambda r: BASE_GEO.get(GEOS[r["geo"]], GEOS[r["geo"]])
    exceptions = set()
    for c, p, r in zip(calls, promoted, real):
        assert p["status"] == 0 and r["status"] == 0 and r["family"] == 0  # (real rows never run the whole-row kernel)
        assert [base(r)] + [r[k] for k in ("win", "st", "pair", "nseg", "cj", "seg_rot")] == \
               [base(p)] + [p[k] for k in ("win", "st", "pair", "nseg", "cj", "seg_rot")], c
        four_byte = r["pair"] and (c["pitch_odd"] or c["base_align"] & 7)
        assert r["real"] == (2 if four_byte else 1) and not r["real_st"]
        if (r["geo"], r["w4"], r["twc"]) != (p["geo"], p["w4"], p["twc"]):
            # the window table without compact twiddles (SWIFTLY_K1_WIN4 = 1, or an owner that has none) has a complex
            # instance and no real one; 4-byte loads never take the table
            assert p["w4"] and not r["w4"] and not r["twc"] and GEOS[r["geo"]] == "BandGeo5Pre"
            table_alone = c["win4_level"] == 1 or not c["has_twc"]
            assert table_alone or four_byte, c
            exceptions.add("table alone" if table_alone else "4-byte loads")
    assert exceptions == {"table alone", "4-byte loads"}
    # real output: the mapped store of the complex call, except with accumulate and in the 16384-point geometry
    calls = [c for c, w in golden if not c["in_real"] and not c["out_real"] and c["band_sign"] < 0 and w["status"] == 0]
    assert len(calls) > 50
    complex_, real = choose(dump, calls), choose(dump, [dict(c, out_real=1) for c in calls])
    for c, p, r in zip(calls, complex_, real):
        if c["accumulate"] or c["logn"] == 14:
            assert r["status"] == -1
        else:
            assert r == dict(p, real_st=1), c
    assert {r["status"] for r in real} == {0, -1}


def test_data_segment_run_against_a_count_on_the_padded_row(dump):
    n, seglen = 32768, 1024
    nseg = n // seglen
    shifts = numpy.arange(n)
    for length in (22528, 11488):
        answers = numpy.array([[int(v) for v in line.split()] for line in dump([f"run {a} {length} {n} {seglen}" for a in shifts])])
        # data points per segment: input j holds data when q = (j + n/2 + ld_a) mod n < length
        total = numpy.concatenate([[0], numpy.cumsum(numpy.arange(2 * n) % n < length)])
        start = ((numpy.arange(nseg) * seglen)[None, :] + n // 2 + shifts[:, None]) % n
        has = (total[start + seglen] - total[start]) > 0
        assert has.any(axis=1).all() and not has.all(axis=1).any()
        first = numpy.argmax(has & ~numpy.roll(has, 1, axis=1), axis=1)
        assert ((has & ~numpy.roll(has, 1, axis=1)).sum(axis=1) == 1).all()  # one cyclic run
        assert numpy.array_equal(answers[:, 0], has.sum(axis=1)) and numpy.array_equal(answers[:, 1], first)
        assert set(answers[:, 0]) == {-(-length // seglen), -(-length // seglen) + 1}
    assert dump([f"run 0 {n} {n} {seglen}", f"run 5 0 {n} {seglen}"]) == [f"{nseg} 0", "1 0"]  # no empty segment; no data


def test_lean_row_kernel_forms(dump):
    """real load: 8192 points, MODE 0 only; real store: 8192 / 16384 points, MODE 1 / 2, no accumulate; complex: 8192 .. 32768"""
    def form(logn, mode, in_real=0, out_real=0, accumulate=0):
        return int(dump([f"lean {logn} {mode} {in_real} {out_real} {accumulate}"])[0])

    for logn in range(11, 18):
        for mode in (0, 1, 2):
            assert form(logn, mode) == (0 if 13 <= logn <= 15 else -1)
            assert form(logn, mode, in_real=1) == (1 if (logn, mode) == (13, 0) else -1)
            assert form(logn, mode, out_real=1) == (2 if logn in (13, 14) and mode in (1, 2) else -1)
            assert form(logn, mode, out_real=1, accumulate=1) == -1
