"""
Every instance of the band row kernel against the 1-D oracle, by name.

``SWF_BAND_INSTANCES`` (csrc/row_pass.hip) lists 54 instances of ``row_pass_band_kernel`` and csrc/row_whole.hip six of the
whole-row kernel; ``choose_band_instance`` (csrc/swiftly_rowinst.h) picks one per call.  tests/band_instance_cases.py holds,
for each of the 53 instances an exported entry point can reach, calls that run it (tests/test_band_instances_cpu.py checks
that table against the list and the chooser without a GPU, and names the other 7 with the launch-site condition that excludes
them).  This module makes every one of those calls and asserts, per case:

* the call made exactly ONE band row launch (the thread's counter of ``swiftly_hip_last_band_instance``): an entry point that
  took the lean kernel, the generic rows or a promoted copy instead fails here;
* the launch was not refused and ran the instance the table names, with the expected segment rotation -- the record is taken
  after the fallback of a full window-table cache;
* the sentinels around the output are intact, masked pixels are exactly zero;
* ALL output elements agree with the complex128 oracle, composed as the facet sweep composes it: ``prepare_facet`` (times
  ``facet_window`` when folded) for K1 and the plain prepare_facet, ``prepare_subgrid`` per row, ``finish_facet`` times the mask
  (``.real`` for the float32 store), and ``extract_from_facet`` -> ``add_to_subgrid`` -> index for the window rows.  No
  expected value comes from another HIP path.

Bounds (the project's own, none tuned against these kernels): relative RMSE below ``2e-6 * sqrt(min(L, 15) / 15)`` and
``max|err| <= 2e-5 * max|want|`` per row (``check`` / ``vector_peak`` of test_hip_facet_sweep_gpu.py); the window-rows store
``2.5e-6`` (test_window_rows_store_of_the_whole_row_k1_matches_the_row_pass_per_wave: its data passes two transforms and
the Fn window).

``SWIFTLY_K1_WIN4`` and ``SWIFTLY_K1_WHOLE`` are read once per process, so the cases of the three other settings run in a
fresh child process each (tests/_band_sweep_worker.py: the same ``run_case``), one after the other.

Measured on an MI355X: the worst relative RMSE over the cases of an instance (every case prints a ``BANDSWEEP`` line with its
instance, figure, bound, per-row peak, rotation and window path).  Template arguments as in ``SWF_BAND_INSTANCES``: WIN, ST,
PAIR, NSEG, CJ, W4, REAL, REAL_ST; "16 / 22 / 24" = the three segment counts of the forward K1.

  BandGeo16k   <1,1,0,0,-1,0,R,0>       R = 0: 1.65e-07   R = 1: 1.75e-07
  BandGeo4     <W,0,0,0,-1,0,0,0>       W = 1 (prepare_facet): 1.68e-07   W = 0 (prepare_subgrid): 1.63e-07
  BandGeo5     <1,1,0,0,-1,0,R,0>       R = 0: 1.74e-07   R = 1: 1.67e-07
  BandGeo5     <1,1,1,0,-1,0,R,0>       R = 0: 1.90e-07   R = 1: 1.74e-07   R = 2: 1.75e-07
  BandGeo5     <0,2,0,0,-1,0,0,S>       S = 0: 1.73e-07   S = 1: 1.66e-07
  BandGeo5     <0,2,1,0,-1,0,0,S>       S = 0: 1.82e-07   S = 1: 1.78e-07
  BandGeo5     <0,2,1,13 / 16,0,0,0,S>  S = 0: 1.78e-07 / 1.76e-07   S = 1: 1.78e-07 / 1.76e-07   (SWIFTLY_K1_WIN4 = 0, 1)
  BandGeo5C    <0,2,1,13 / 16,0,0,0,S>  S = 0: 1.81e-07 / 1.74e-07   S = 1: 1.94e-07 / 1.74e-07
  BandGeo5Pre  <1,1,1,N,1,0,0,0>        16 / 22 / 24: 1.89e-07 / 1.98e-07 / 2.05e-07   (SWIFTLY_K1_WIN4 = 0; 65th table: 2.06e-07)
  BandGeo5Pre  <1,1,1,N,1,0,1,0>        16 / 22 / 24: 1.73e-07 / 1.86e-07 / 1.84e-07   (SWIFTLY_K1_WIN4 = 0, 1)
  BandGeo5Pre  <1,1,1,N,1,0,2,0>        16 / 22 / 24: 1.73e-07 / 1.86e-07 / 1.84e-07
  BandGeo5Pre  <1,1,1,N,1,1,0,0>        16 / 22 / 24: 1.89e-07 / 1.85e-07 / 1.90e-07   (SWIFTLY_K1_WIN4 = 1)
  BandGeo5PreC <1,1,1,N,1,1,R,0>        R = 0: 1.89e-07 / 1.91e-07 / 1.90e-07   R = 1: 1.87e-07 / 2.00e-07 / 1.98e-07
  BandGeo64k   <W,0,0,0,-1,0,0,0>       W = 1: 1.79e-07   W = 0: 1.74e-07
  BandGeo64k   <0,2,0,0,-1,0,0,S>       S = 0: 1.75e-07   S = 1: 1.78e-07
  BandGeo64k   <1,1,0,0,-1,0,R,0>       R = 0: 1.77e-07   R = 1: 1.75e-07
  BandGeo64k   <1,1,0,44,1,0,R,0>       R = 0: 1.84e-07   R = 1: 1.84e-07
  whole row, band store  (SWIFTLY_K1_WHOLE = 1)   16 / 22 / 24: 1.89e-07 / 1.85e-07 / 1.90e-07
  whole row, window rows                          16 / 22 / 24: 1.82e-07 / 1.42e-06 / 1.43e-06   (bound 2.5e-06)

Bound of all but the last line: 2.0e-06 (16384 points: 1.93e-06).  Worst per-row peak (bound 2e-05): 3.6e-07, window rows 3.5e-06.
The window rows of a 352-point facet (16 segments) carry no 1 / PSWF amplification; band_instance_cases.py says why a
24576-point facet is not among the window-rows cases (2.7e-06 there, from K1's rounding alone).

Module wall time on an MI355X: 18 s for the 74 tests (pytest's own figure); the slowest are the three child processes with
3.5 s each and the first case, which builds the 32768-point core and its oracle (3.2 s).
"""
import json
import os
import subprocess
import sys

import pytest

import band_instance_cases as bic
from _band_sweep_worker import cores, instance_name, last_instance, run_case

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_band_sweep_worker.py")
KNOBS = {"level0": bic.LEVEL0, "level1": bic.LEVEL1, "whole": bic.WHOLE}


@pytest.mark.parametrize("case", bic.cases_of(bic.DEFAULT), ids=lambda c: c["id"])
def test_band_instance(case):
    """the cases of the default environment (SWIFTLY_K1_WIN4 = 2: window table and compact twiddles; no whole-row band store)"""
    for name in ("SWIFTLY_K1_WIN4", "SWIFTLY_K1_WHOLE"):
        assert name not in os.environ, f"{name} is set: this process does not run the default instances"
    run_case(case)


_children = {}  # setting -> exit status of its child


@pytest.mark.parametrize("name", list(KNOBS))
def test_other_knob_settings_in_child_processes(name):
    """SWIFTLY_K1_WIN4 = 0, SWIFTLY_K1_WIN4 = 1 and SWIFTLY_K1_WHOLE = 1: one child process per setting, three in all, one
    after the other (3.5 s each: the interpreter, the 32768-point core and its oracle).  A child that does not end with
    status 0 fails its test with the tail of its output, and no further child is started"""
    bad = {k: v for k, v in _children.items() if v != 0}
    assert not bad, f"an earlier child ended with {bad}: no further child is started"
    knob = KNOBS[name]
    ids = [c["id"] for c in bic.cases_of(knob)]
    assert ids
    env = {k: v for k, v in os.environ.items() if k not in ("SWIFTLY_K1_WIN4", "SWIFTLY_K1_WHOLE")}
    _children[name] = "started"
    res = subprocess.run([sys.executable, WORKER] + ids, env=dict(env, **knob), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=300, check=False)
    _children[name] = res.returncode
    print(res.stdout, end="")
    lines = [json.loads(line) for line in res.stdout.splitlines() if line.startswith("{")]
    assert res.returncode == 0, f"{name}: exit status {res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-3000:]}"
    assert [line["id"] for line in lines] == ids and not any("failed" in line for line in lines), name


def test_window_table_fallback():
    """``Win4Cache::kMaxEntries`` = 64 tables per handle, none is ever evicted: on a fresh 32768-point core 64 calls with
    distinct table keys each take a table, the 65th falls back to the plain window loads of BandGeo5Pre (W4 = 0) -- same
    segment count and rotation, the oracle's values -- and a repeat of the first call still finds its table"""
    assert "SWIFTLY_K1_WIN4" not in os.environ and "SWIFTLY_K1_WHOLE" not in os.environ
    core, _ = cores("c15", fresh=True)
    # 22528 points from 2 k points before input 0 on: segment 31 holds the first 2 k of them, the table key is their position
    offs = [11264 - 2 * k for k in range(66)]
    template = next(c for c in bic.CASES if c["id"] == "k1-prec-24-rot21-c64")
    keys = set()
    for k in range(64):
        case = dict(template, id=f"fallback-{k}", rows=1, off=offs[k], fold=False)
        tuned = ("BandGeo5PreC", 1, 1, 1, 22 if k == 0 else 24, 1, 1, 0, 0)
        run_case(case, core=core, want_instance=tuned, want_rot=0 if k == 0 else 31)
        rec = last_instance()[1]
        assert rec["ld_win4"] == 1 and rec["twc"] == 1 and rec["key_ns"] == tuned[4], (k, rec)
        keys.add((rec["key_c"], rec["key_ns"]))
    assert len(keys) == 64
    full = dict(template, id="fallback-65th", rows=7, off=offs[64], fold=True)
    run_case(full, core=core, want_instance=("BandGeo5Pre", 1, 1, 1, 24, 1, 0, 0, 0), want_rot=31)
    rec = last_instance()[1]
    assert (rec["ld_win4"], rec["twc"], rec["w4"], rec["key_ns"]) == (0, 0, 0, 0), rec
    print(f"the 65th table: {instance_name(rec)}")
    # real rows fall back alike
    run_case(dict(full, id="fallback-66th-f32", off=offs[65], dtype="f32"), core=core,
             want_instance=("BandGeo5Pre", 1, 1, 1, 24, 1, 0, 1, 0), want_rot=31)
    # the tables that exist stay in use
    run_case(dict(template, id="fallback-repeat-0", rows=1, off=offs[0], fold=False), core=core,
             want_instance=("BandGeo5PreC", 1, 1, 1, 22, 1, 1, 0, 0), want_rot=0)
    assert last_instance()[1]["ld_win4"] == 1
