"""Runner of tests/test_hip_band_instance_sweep_gpu.py: ``run_case`` makes the call of one case of
tests/band_instance_cases.py, asserts which instance of the band row kernel it ran (``swiftly_hip_last_band_instance``) and
compares all of its output with the complex128 oracle.  The pytest module calls it for the cases of the default
environment; the cases that need ``SWIFTLY_K1_WIN4`` / ``SWIFTLY_K1_WHOLE`` (read once per process by the library) run in a
child process that executes this file: ``python _band_sweep_worker.py <case id> ...`` prints one JSON line per case and
ends with status 0 only if every case passed."""
import ctypes
import json
import os
import sys

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ska-sdp-distributed-fourier-transform_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import band_instance_cases as bic  # noqa: E402  pylint: disable=wrong-import-position

INST = "status family geo win st pair nseg cj w4 real real_st seg_rot ld_win4 twc key_c key_ns key_n key_seglen".split()
TEMPLATE = ("win", "st", "pair", "nseg", "cj", "w4", "real", "real_st")
SENTINEL = complex(7.5, -3.25)
WINDOW_ROWS_BOUND = 2.5e-6  # test_window_rows_store_of_the_whole_row_k1_matches_the_row_pass_per_wave (measured there: 1.44e-6)
PEAK_BOUND = 2e-5

_CORES, _DATA, _WANT = {}, {}, {}


def f32_bound(stages):
    """the project's 2e-6 for one float32 transform of 15 or more stages (f32_bound of test_hip_facet_sweep_gpu.py)"""
    return 2e-6 * float(numpy.sqrt(min(stages, 15) / 15.0))


def relrms(got, want):
    return float(numpy.sqrt(numpy.mean(numpy.abs(got - want) ** 2) / numpy.mean(numpy.abs(want) ** 2)))


def vector_peak(got, want, axis):
    """largest ``max|err| / max|want|`` over the transformed vectors; a vector that must be zero must be exactly zero
    (vector_peak of test_hip_facet_sweep_gpu.py)"""
    err = numpy.abs(got - want).max(axis=axis)
    ref = numpy.abs(want).max(axis=axis)
    assert not err[ref == 0].any(), "a vector that must be zero is not"
    return float((err[ref > 0] / ref[ref > 0]).max())


def band_cols(yN, band):
    """physical column of every logical (centred) column, -1 outside the band (parity-split layout)"""
    start, length = band
    half = bic.band_half(length)
    d = (numpy.arange(yN) - start) % yN
    return numpy.where(d < length, (d & 1) * half + (d >> 1), -1)


def cores(key, fresh=False):
    """``(SwiftlyCoreHip, OracleCore)`` of ``bic.CORES[key]``, built once per process (``fresh``: a new handle, whose window
    tables are its own, with the shared oracle)"""
    from oracle import swiftly_oracle as orc
    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    W, N, xM, yN = bic.CORES[key]
    if key not in _CORES:
        _CORES[key] = (SwiftlyCoreHip(W, N, xM, yN), orc.OracleCore(W, N, xM, yN))
    if fresh:
        return SwiftlyCoreHip(W, N, xM, yN), _CORES[key][1]
    return _CORES[key]


def last_instance():
    """(band row launches of this thread so far, the record of the last one)"""
    from ska_sdp_exec_swiftly_amd import _lib

    buf = (ctypes.c_int32 * len(INST))()
    count = int(_lib.load().swiftly_hip_last_band_instance(buf, len(INST)))
    return count, dict(zip(INST, (int(v) for v in buf)))


def instance_name(rec):
    if rec["family"] == 1:
        return f"Whole<{rec['nseg']},st={rec['st']}>"
    return f"{bic.GEOS[rec['geo']]}<" + ",".join(str(rec[k]) for k in TEMPLATE) + ">"


def instance_of(rec):
    """the record as a case's ``want``"""
    if rec["family"] == 1:
        return ("whole", rec["nseg"], rec["st"])
    return (bic.GEOS[rec["geo"]],) + tuple(rec[k] for k in TEMPLATE)


def rows_of(case, length=None):
    """the input rows of a case: host array (complex64, or float32 for real rows), seeded by the shape -- shared, never changed"""
    length = length or case["size"]
    real = case.get("dtype") == "f32"
    key = (real, case["rows"], length)
    if key not in _DATA:
        rng = numpy.random.default_rng(9000 + 31 * case["rows"] + length + int(real))
        x = rng.standard_normal((case["rows"], length))
        _DATA[key] = x.astype(numpy.float32) if real else (x + 1j * rng.standard_normal(x.shape)).astype(numpy.complex64)
    return _DATA[key]


def shared(key, make):
    if key not in _WANT:
        _WANT[key] = make()
    return _WANT[key]


def on_device(case, x):
    """``x`` as ``storage[rows, pitch][:, base : base + size]`` on the device"""
    import torch

    pitch, base = case.get("pitch") or x.shape[1], case.get("base", 0)
    assert pitch >= base + x.shape[1]
    storage = torch.zeros((x.shape[0], pitch), dtype=torch.from_numpy(x).dtype, device="cuda")
    view = storage[:, base : base + x.shape[1]]
    view.copy_(torch.from_numpy(x))
    assert view.stride(0) == pitch and view.data_ptr() % 16 == (base * x.itemsize) % 16
    return view


def _k1(case, core, ref, oracle_off):
    import torch

    from ska_sdp_exec_swiftly_amd import _lib

    yN, rows, size, band = core.yN_size, case["rows"], case["size"], case["band"]
    x = rows_of(case)
    src = on_device(case, x)
    ncols = core.band_columns(band)
    obuf = torch.full((rows + 1, ncols + 16), SENTINEL, dtype=torch.complex64, device="cuda")
    out = obuf[:rows, :ncols]
    lib = _lib.load()
    entry = lib.swiftly_hip_prepare_facet_band_real if case["dtype"] == "f32" else lib.swiftly_hip_prepare_facet_band
    rc = entry(core._handle, _lib.C64, ctypes.c_void_p(src.data_ptr()), rows, size, src.stride(0),  # pylint: disable=protected-access
               ctypes.c_void_p(out.data_ptr()), out.stride(0), case["off"], band[0], band[1], int(case["fold"]), None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()

    def check_rest():
        assert bool((obuf[rows] == SENTINEL).all()) and bool((obuf[:, ncols:] == SENTINEL).all()), "prepare_facet_band wrote outside its band buffer"

    want = shared(("prepare_facet", case["core"], case["dtype"], rows, size, oracle_off),
                  lambda: ref.prepare_facet(x.astype(complex), oracle_off, 1))
    if case["fold"]:
        want = want * ref.facet_window(rows)[:, None]
    pc = band_cols(yN, band)
    keep = pc >= 0
    return out.cpu().numpy()[:, pc[keep]], want[:, keep], 1, f32_bound(yN.bit_length() - 1), check_rest


def _window_rows(case, core, ref, oracle_off):
    import torch

    yN, xM, N, m = core.yN_size, core.xM_size, core.N, core.xM_yN_size
    rows, band, waves = case["rows"], case["band"], case["waves"]
    x = rows_of(case)
    src = on_device(case, x)
    starts = core.window_starts(band, waves)
    assert min(starts) >= 0 and max(starts) + m <= band[1] and core.supports_window_rows(band, case["size"], [case["off"]], len(waves))
    sd = torch.tensor(starts, dtype=torch.int32, device="cuda")
    obuf = torch.full((len(waves), rows + 1, m + 8), SENTINEL, dtype=torch.complex64, device="cuda")
    out = obuf[:, :rows, :m]
    core.prepare_facet_window_rows(src, case["off"], band, sd, out, fold_other_axis_window=False)
    torch.cuda.synchronize()

    def check_rest():
        assert bool((obuf[:, rows] == SENTINEL).all()) and bool((obuf[:, :, m:] == SENTINEL).all()), "prepare_facet_window_rows wrote outside its window rows"

    def oracle():
        # extract_from_facet -> add_to_subgrid -> index, as test_window_rows_store_of_the_whole_row_k1_matches_the_row_pass_per_wave
        prepared = ref.prepare_facet(x.astype(complex), oracle_off, 1)
        sp = oracle_off * xM // N
        k = numpy.arange(m)
        res = []
        for off1 in waves:
            placed = ref.add_to_subgrid(ref.extract_from_facet(prepared, off1, 1), oracle_off, 1)
            Z = placed[:, (k + xM // 2 - m // 2 + sp) % xM]
            res.append(Z[:, (k + off1 * yN // N) % m])
        return numpy.stack(res)

    want = shared(("window_rows", rows, case["size"], oracle_off), oracle)
    got = out.cpu().numpy()
    k = numpy.arange(m)
    logical = numpy.empty_like(got)
    for w, start in enumerate(starts):
        wband = ((band[0] + start) % yN, m)
        cols = band_cols(yN, wband)[(wband[0] + k) % yN]
        assert sorted(cols) == list(range(m))
        logical[w] = got[w][:, cols]
    return logical, want, 2, WINDOW_ROWS_BOUND, check_rest


def _finish(case, core, ref, oracle_off):
    import torch

    yN, rows, yB, (start, length), real = core.yN_size, case["rows"], case["size"], case["band"], case["real"]
    data = rows_of(case, length)
    mask = shared(("mask", yB), lambda: (numpy.random.default_rng(yB).random(yB) > 0.15).astype(float))
    assert 0 < mask.sum() < yB

    def oracle():
        full = numpy.zeros((rows, yN), dtype=complex)
        full[:, (start + numpy.arange(length)) % yN] = data
        return ref.finish_facet(full, oracle_off, yB, axis=1) * mask[None, :]

    want = shared(("finish", case["core"], rows, start, length, yB, oracle_off), oracle)
    sentinel = SENTINEL.real if real else SENTINEL
    obuf = torch.full((rows + 1, yB + 5), sentinel, dtype=torch.float32 if real else torch.complex64, device="cuda")
    out = obuf[:rows, 1 : yB + 1] if real else obuf[:rows, :yB]
    dev = torch.from_numpy(data).cuda()
    assert dev.stride(0) == length
    res = core.finish_facet_band(dev, (start, length), case["off"], yB, mask=mask, out=out, real=real)
    assert res is out
    torch.cuda.synchronize()

    def check_rest():
        assert bool((obuf[rows] == sentinel).all()) and bool((obuf[:, yB + 1 :] == sentinel).all()) and \
            bool((obuf[:, 0 if real else yB] == sentinel).all()), "finish_facet_band wrote outside its rows"
        assert not bool((out[:, torch.from_numpy(mask == 0).cuda()] != 0).any()), "a masked pixel is not exactly zero"

    got = out.cpu().numpy()
    if real:
        got, want = got.astype(numpy.complex64), want.real
    return got, want, 1, f32_bound(yN.bit_length() - 1), check_rest


def _plain(case, core, ref, oracle_off):
    import torch

    rows, size, kind = case["rows"], case["size"], case["kind"]
    n = core.xM_size if kind == "prepare_subgrid" else core.yN_size
    x = rows_of(case)
    src = torch.from_numpy(x).cuda()
    obuf = torch.full((rows + 1, n + 8), SENTINEL, dtype=torch.complex64, device="cuda")
    out = obuf[:rows, :n]
    if kind == "prepare_facet":
        res = core.prepare_facet(src, case["off"], 1, out=out)
        want = shared(("prepare_facet", case["core"], "c64", rows, size, oracle_off), lambda: ref.prepare_facet(x.astype(complex), oracle_off, 1))
    else:
        res = core._axis_call("prepare_subgrid", src, None, n, 1, out, False, case["off"], size_arg=size)  # pylint: disable=protected-access
        want = shared(("prepare_subgrid", case["core"], rows, size, oracle_off),
                      lambda: numpy.stack([ref.prepare_subgrid(row.astype(complex), oracle_off) for row in x]))
    assert res is out
    torch.cuda.synchronize()

    def check_rest():
        assert bool((obuf[rows] == SENTINEL).all()) and bool((obuf[:, n:] == SENTINEL).all()), f"{kind} wrote outside its rows"

    return out.cpu().numpy(), want, 1, f32_bound(n.bit_length() - 1), check_rest


RUNNERS = {"k1": _k1, "window_rows": _window_rows, "finish": _finish, "prepare_facet": _plain, "prepare_subgrid": _plain}


def run_case(case, core=None, want_instance=None, want_rot=None, oracle_off=None):
    """the call of ``case`` -- exactly one band row launch -- with its instance, its sentinels and all of its output
    checked; returns the figures of its BANDSWEEP line.  ``core``: another handle of the same sizes; ``want_instance`` /
    ``want_rot``: another expectation than the table's (a full window-table cache); ``oracle_off``: the offset the oracle
    gets (the case's)"""
    shared_core, ref = cores(case["core"])
    core = core or shared_core
    want_instance = tuple(case["want"]) if want_instance is None else tuple(want_instance)
    want_rot = case["seg_rot"] if want_rot is None else want_rot
    before, _ = last_instance()
    got, want, axis, bound, check_rest = RUNNERS[case["kind"]](case, core, ref, case["off"] if oracle_off is None else oracle_off)
    after, rec = last_instance()
    assert after - before == 1, f"{case['id']}: {after - before} band row launches, not one"
    assert rec["status"] == 0, (case["id"], rec)
    assert instance_of(rec) == want_instance, f"{case['id']}: ran {instance_name(rec)}, not {want_instance}"
    if want_instance[-2 if want_instance[0] == "whole" else 4] != 0:
        assert rec["seg_rot"] == want_rot, (case["id"], rec["seg_rot"], want_rot)
    check_rest()
    assert got.shape == want.shape and got.dtype == numpy.complex64 and numpy.isfinite(got).all(), case["id"]
    err, peak = relrms(got, want), vector_peak(got, want, axis)
    print(f"BANDSWEEP {case['id']:<34s} {instance_name(rec):<44s} {err:.3e} (bound {bound:.2e}) peak {peak:.2e} rot {rec['seg_rot']} "
          f"table {rec['ld_win4']} twc {rec['twc']}", flush=True)
    assert err < bound, (case["id"], err, bound)
    assert peak <= PEAK_BOUND, (case["id"], peak)
    return dict(id=case["id"], instance=instance_name(rec), relrmse=err, bound=bound, peak=peak)


def main(ids):
    by_id = {c["id"]: c for c in bic.CASES}
    failed = 0
    for cid in ids:
        case = by_id[cid]
        for name, value in case["knob"].items():
            assert os.environ.get(name) == value, f"{cid} needs {name}={value}"
        try:
            print(json.dumps(run_case(case)), flush=True)
        except AssertionError as exc:
            failed += 1
            print(json.dumps(dict(id=cid, failed=str(exc)[:2000])), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
