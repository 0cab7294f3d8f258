"""
The window-rows store of REAL rows in ``choose_band_instance`` (csrc/swiftly_rowinst.h), without a GPU.  ``BandCall::whole_real``
says that the whole-row family has real window-rows instances -- a fact about the kernel family that the launcher supplies.
``tests/native/band_instance_real_windows_dump.cpp`` reads the 29 fields of ``tests/native/band_instance_dump.cpp`` plus
that one.

With the field 0 every recorded call of ``tests/golden/band_instances.txt`` answers as recorded (a real ``win_full`` call: -1).
With it 1 a real ``win_full`` call gets what the complex window-rows call for the promoted row gets, with ``real = 1`` --
provided two adjacent reals are one 8-byte load (even pitch, base aligned to 8); else -2.  There is no ``real = 2`` form.
"""
import os
import re
import subprocess

import pytest

from test_band_instances_cpu import CALL, CSRC, INST, ROOT

CALL_R = CALL + ["whole_real"]
SAME = ("family", "geo", "nseg", "st", "seg_rot", "ld_win4", "twc", "key_c", "key_ns", "key_n", "key_seglen")
WINDOW_ROWS_ST = 3  # kBandStWindowRows


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC\s*\?=\s*(\S+)", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1)
    exe = str(tmp_path_factory.mktemp("band_instances_real_windows") / "band_instance_real_windows_dump")
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "band_instance_real_windows_dump.cpp"), "-o", exe], check=True, timeout=300)

    def run(calls):
        requests = ["band " + " ".join(str(c[k]) for k in CALL_R) for c in calls]
        res = subprocess.run([exe], input="\n".join(requests) + "\n", stdout=subprocess.PIPE, text=True, check=True, timeout=120)
        lines = res.stdout.splitlines()
        assert len(lines) == len(calls)
        return [dict(zip(INST, map(int, line.split()))) for line in lines]

    return run


@pytest.fixture(scope="module")
def golden():
    rows = []
    with open(os.path.join(ROOT, "tests", "golden", "band_instances.txt"), encoding="utf-8") as fh:
        for line in fh:
            call, answer = (side.split() for side in line.split("->"))
            assert len(call) == len(CALL) and len(answer) == len(INST), line
            rows.append((dict(zip(CALL, map(int, call))), {k: None if v == "-" else int(v) for k, v in zip(INST, answer)}))
    assert 1000 < len(rows) < 5000
    return rows


def test_field_off_every_golden_call_answers_as_recorded(dump, golden):
    got = dump([dict(c, whole_real=0) for c, _ in golden])
    for (call, want), have in zip(golden, got):
        assert {k: have[k] for k, v in want.items() if v is not None} == {k: v for k, v in want.items() if v is not None}, call
    # among them: the real window-rows call, refused with -1
    assert any(c["in_real"] and c["win_full"] and w["status"] == -1 for c, w in golden)


def _window_rows_calls(golden, status):
    calls = [c for c, w in golden if c["win_full"] and not c["in_real"] and not c["out_real"] and w["status"] == status and
             (status != 0 or w["family"] == 1)]
    assert len(calls) >= 20
    return calls


def test_field_on_real_rows_get_the_window_rows_instance_of_the_promoted_row(dump, golden):
    calls = _window_rows_calls(golden, 0)
    complex_ = dump([dict(c, whole_real=1) for c in calls])
    assert {p["nseg"] for p in complex_} == {16, 22, 24}
    for align in (0, 8):
        real = dump([dict(c, in_real=1, pitch_odd=0, base_align=align, whole_real=1) for c in calls])
        for c, p, r in zip(calls, complex_, real):
            assert p["status"] == 0 and p["family"] == 1 and p["st"] == WINDOW_ROWS_ST and p["real"] == 0, c
            assert r["status"] == 0, (c, align)
            assert {k: r[k] for k in SAME} == {k: p[k] for k in SAME}, (c, align)
            assert r["real"] == 1 and not r["real_st"]
            assert r == dict(p, real=1)  # nothing else differs either
    # the field changes nothing for the complex call itself
    assert complex_ == dump([dict(c, whole_real=0) for c in calls])


def test_field_on_rows_that_8_byte_loads_cannot_read_are_refused(dump, golden):
    calls = _window_rows_calls(golden, 0)
    for pitch_odd, align in ((1, 0), (0, 4), (1, 4), (1, 8), (0, 12)):
        real = dump([dict(c, in_real=1, pitch_odd=pitch_odd, base_align=align, whole_real=1) for c in calls])
        assert {r["status"] for r in real} == {-2}, (pitch_odd, align)
        assert all(r["real"] == 0 and r["family"] == 0 for r in real)  # a refusal names no instance: no real = 2 form


def test_field_on_refused_complex_calls_stay_refused_as_real(dump, golden):
    """Every recorded complex window-rows call that is refused with -2, made real, stays -2.  One kind of line needs a second
    look: a complex row on an 8-byte base at an even pitch is refused because ITS loads are 16 bytes wide, while real rows
    there are exactly what the 8-byte loads read (the test above demands status 0 for them).  The rule is the one of the
    chooser's header -- the real call answers like the complex call for the PROMOTED row (contiguous, aligned), and
    needs 8-byte loads on its own rows -- so those lines, and only those, are accepted; every other refusal stays."""
    calls = _window_rows_calls(golden, -2)
    real = dump([dict(c, in_real=1, whole_real=1) for c in calls])
    promoted = dump([dict(c, pitch_odd=0, base_align=0, whole_real=1) for c in calls])
    accepted = []
    for c, p, r in zip(calls, promoted, real):
        if p["status"] == -2 or c["pitch_odd"] or c["base_align"] & 7:
            assert r["status"] == -2, c
        else:
            accepted.append(c)
            assert r == dict(p, real=1) and p["status"] == 0 and p["st"] == WINDOW_ROWS_ST, c
    assert accepted and all(c["base_align"] == 8 and not c["pitch_odd"] for c in accepted)
    assert len(accepted) < len(calls) // 10
    # with the rows of the real call contiguous and aligned, as a promoted copy would be: every other reason still refuses
    others = [c for c in calls if not (c["pitch_odd"] or c["base_align"])]
    real = dump([dict(c, in_real=1, whole_real=1) for c in others])
    assert len(others) > 20 and {r["status"] for r in real} == {-2}


def test_calls_without_window_rows_do_not_read_the_field(dump, golden):
    calls = [c for c, _ in golden if not c["win_full"]]
    assert len(calls) > 1000 and any(c["in_real"] for c in calls) and any(c["out_real"] for c in calls)
    assert dump([dict(c, whole_real=0) for c in calls]) == dump([dict(c, whole_real=1) for c in calls])
    # real rows at every pitch / base as well
    real = [dict(c, in_real=1, out_real=0, pitch_odd=po, base_align=al) for c in calls for po, al in ((0, 0), (1, 0), (0, 4), (0, 8))]
    assert dump([dict(c, whole_real=0) for c in real]) == dump([dict(c, whole_real=1) for c in real])
