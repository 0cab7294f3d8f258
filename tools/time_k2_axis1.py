"""Time the third form of the axis-1-first order, ``SwiftlyConfig(axis1_first="k2")`` -- the contiguous-axis finish inside the
first pass of K2's four-step (``swiftly_hip_prepare_facet_columns_axis1``) -- against the forms it stands beside (DESIGN.md
section 2), on the benchmarked 64k sparse workload.  One process, one build, forms interleaved, HIP events, median and
spread of ``--reps`` repeats after ``--warmups`` untimed rounds:

(a) per wave, at the workload's shape (its facets' rows, its plan's band, random band buffers -- K2 does not care what K1
    wrote): ``finish_axis1_rows`` + ``prepare_facet_columns`` (the "rows" form) against the one new call, for a wave in the
    middle of the band, with that wave's row map; the two outputs compared;
(b) the whole forward pass of the workload (its builders taken from bench.py: a fresh planned ``SwiftlyForward`` per pass,
    K1 of every facet, every wave) in the default order and with ``axis1_first`` = "rows", True and "k2", and the relative
    RMSE of picked subgrids of each against the separable oracle.

    python tools/time_k2_axis1.py [--reps 7] [--warmups 2] [--facets N] [--out profiles/r29_k2_axis1_timing.json]
"""
import argparse
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ska-sdp-distributed-fourier-transform_amd")]

FORMS = {"default": False, "rows": "rows", "True": True, "k2": "k2"}


def timed(torch, fn):
    """milliseconds of ``fn()`` between two HIP events on the current stream (ending in a device synchronise), and its result"""
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), out


def stats(ms):
    return {"median ms": round(statistics.median(ms), 3), "min ms": round(min(ms), 3), "max ms": round(max(ms), 3),
            "all ms": [round(t, 3) for t in ms]}


def interleaved(torch, forms, reps, warmups):
    """``{name: [ms] * reps}`` of the callables ``forms``, one after the other in every round"""
    times = {name: [] for name in forms}
    for rep in range(warmups + reps):
        for name, fn in forms.items():
            ms, out = timed(torch, fn)
            del out
            if rep >= warmups:
                times[name].append(ms)
    return times


def per_wave(torch, core, facet_cfgs, sg_cfgs, args):
    yN, m, F = core.yN_size, core.xM_yN_size, len(facet_cfgs)
    rows = facet_cfgs[0].size
    off1s = sorted({c.off1 for c in sg_cfgs})
    band = core.band_for_offsets(off1s)
    off1 = off1s[len(off1s) // 2]
    rowmap, n_rows = core.subgrid_column_rows([c.off0 for c in sg_cfgs if c.off1 == off1])
    gen = torch.Generator(device="cuda").manual_seed(29)
    bands = torch.view_as_complex(torch.randn((F, rows, core.band_columns(band), 2), generator=gen, device="cuda"))
    f0, f1 = [c.off0 for c in facet_cfgs], [c.off1 for c in facet_cfgs]
    w_rows = torch.empty((F, rows, m), dtype=torch.complex64, device="cuda")
    q_rows = torch.empty((F, n_rows, m), dtype=torch.complex64, device="cuda")
    q_k2 = torch.empty_like(q_rows)

    def two_calls():
        _, wband = core.finish_axis1_rows(bands, f1, band, off1, out=w_rows)
        return core.prepare_facet_columns(w_rows, f0, wband, off1, rowmap, n_rows, out=q_rows)

    times = interleaved(torch, {
        "finish_axis1_rows + prepare_facet_columns": two_calls,
        "prepare_facet_columns_axis1": lambda: core.prepare_facet_columns_axis1(bands, f0, f1, band, off1, rowmap, n_rows, out=q_k2),
        "prepare_facet_columns alone (default order, no finish)": lambda: core.prepare_facet_columns(bands, f0, band, off1, rowmap, n_rows, out=q_rows),
    }, args.reps, args.warmups)
    two_calls()
    diff = float((q_k2 - q_rows).abs().pow(2).sum().sqrt() / q_rows.abs().pow(2).sum().sqrt())
    row = {"facets": F, "rows": rows, "band": [int(band[0]), int(band[1])], "off1": int(off1), "rows kept": int(n_rows),
           "finished rows written + read by the two calls, GB": round(2 * F * rows * m * 8 / 1e9, 3),
           "new against two calls, relative RMS difference": diff}
    row.update({name: stats(t) for name, t in times.items()})
    a, b = row["finish_axis1_rows + prepare_facet_columns"], row["prepare_facet_columns_axis1"]
    row["new / two calls"] = round(b["median ms"] / a["median ms"], 3)
    row["faster beyond both spreads"] = bool(b["max ms"] < a["min ms"])
    del bands, w_rows, q_rows, q_k2
    gc.collect()
    torch.cuda.empty_cache()
    return row


def whole_pass(torch, sw, bench, sep, p, facet_cfgs, sg_cfgs, args):
    waves = {}
    for i, c in enumerate(sg_cfgs):
        waves.setdefault(c.off1, []).append(i)
    vectors = [sep.facet_vectors(1234 + j, p["yB_size"], rank=2) for j in range(len(facet_cfgs))]
    data = [bench.separable_facet(torch, vectors[j], facet_cfgs[j]) for j in range(len(facet_cfgs))]
    picks = sep.pick_subgrids(sg_cfgs, 3)
    cfgs = {name: sw.SwiftlyConfig(backend="hip", axis1_first=value, **p) for name, value in FORMS.items()}
    modes = {}

    def one_pass(name, keep=None):
        fwd = sw.SwiftlyForward(cfgs[name], list(zip(facet_cfgs, data)), lru_forward=1, subgrid_configs=sg_cfgs, wave_axis=1)
        fwd.prepare_all_facets()
        for widx in waves.values():
            res = fwd.get_wave([sg_cfgs[i] for i in widx])
            if keep is not None:
                for k, i in enumerate(widx):
                    if i in picks:
                        keep[i] = res[k].cpu().numpy()
        modes[name] = fwd._axis1()  # pylint: disable=protected-access

    times = interleaved(torch, {name: (lambda name=name: one_pass(name)) for name in FORMS}, args.reps, args.warmups)
    row = {"facets": len(facet_cfgs), "subgrids": len(sg_cfgs), "waves": len(waves)}
    for name in FORMS:
        before = cfgs[name].core.axis1_columns_issued
        kept = {}
        one_pass(name, kept)
        torch.cuda.synchronize()
        par = bench.verify_subgrids(p, facet_cfgs, vectors, sg_cfgs, kept, tol=bench.PARITY_TOL)
        row[name] = dict(stats(times[name]), **{"axis1 mode": modes[name], "rel_rmse": float(f"{par['rel_rmse']:.3e}"),
                                                "prepare_facet_columns_axis1 calls per pass": cfgs[name].core.axis1_columns_issued - before})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--facets", type=int, default=0, help="only the first N facets of the cover (0: all; a rehearsal)")
    ap.add_argument("--skip", default="", help="'a' or 'b': leave that part out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import bench
    import ska_sdp_exec_swiftly_amd as sw
    from oracle import separable as sep
    from ska_sdp_exec_swiftly_amd import _lib

    if not torch.cuda.is_available():
        raise SystemExit("time_k2_axis1: no GPU; a time is measured on the device or not at all")
    wl = bench.WORKLOADS["64k-sparse"]
    p = wl["params"]
    cfg = sw.SwiftlyConfig(backend="hip", axis1_first="k2", **p)
    if not cfg.core.supports_axis1_columns(torch.complex64):
        raise SystemExit(f"time_k2_axis1: {_lib.last_error()}")
    facet_cfgs = sw.make_full_facet_cover(cfg)
    if args.facets:
        facet_cfgs = facet_cfgs[: args.facets]
    sg_cfgs = bench.select_subgrids(sw.make_full_subgrid_cover(cfg), p["N"], p["xA_size"], wl["sparse_radius"])
    result = {"workload": wl["name"], "device": torch.cuda.get_device_name(0), "build": _lib.build_info(), "reps": args.reps,
              "warmups": args.warmups, "statistic": "median of HIP-event times; forms interleaved in one process"}
    if args.skip != "a":
        result["per wave"] = per_wave(torch, cfg.core, facet_cfgs, sg_cfgs, args)
        print(json.dumps({"per wave": result["per wave"]}), flush=True)
    del cfg
    if args.skip != "b":
        result["whole pass"] = whole_pass(torch, sw, bench, sep, p, facet_cfgs, sg_cfgs, args)
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
