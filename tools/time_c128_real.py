"""Time what keeping float64 facets real does to the complex128 band passes on the W = 13.5625 catalogue entries that need
complex128 ("Float64 facets in the complex128 band passes").

Per configuration, in one process on one build, HIP events, median of ``--reps`` after one warm-up:

* one full facet through K1: ``prepare_facet_band`` on the promoted complex128 facet against ``prepare_facet_band_float64``
  on the float64 one (the forms alternate), outputs compared bit for bit;
* one full facet through the finish: ``finish_facet_band`` against ``finish_facet_band_float64`` on one complex128 band
  accumulator over the whole padded axis, outputs compared bit for bit;
* the whole passes of ``tools/time_c128_band.py`` and ``tools/time_c128_backward.py`` (2 facets, ``--waves`` x ``--waves``
  planned subgrids, a fresh object per pass with K1 / ``finish()`` included): ``wave_axis=1`` with float64 facets,
  ``wave_axis=1`` with promoted / complex facets, ``wave_axis=0``.

    python tools/time_c128_real.py [--configs 64k[1]-n16k-1k,128k[1]-n32k-1k] [--facets 2] [--waves 4] [--reps 5]
"""
import argparse
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ska-sdp-distributed-fourier-transform_amd")]


def timed(torch, fn):
    """milliseconds of ``fn()`` between two HIP events on the current stream, and its result"""
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), out


def release(torch):
    gc.collect()
    torch.cuda.empty_cache()


def alternate(torch, forms, reps):
    """``{name: [ms] * reps}`` of the callables ``forms`` (name -> fn), alternating, after one warm-up round"""
    times = {name: [] for name in forms}
    for rep in range(reps + 1):
        for name, fn in forms.items():
            ms, out = timed(torch, fn)
            del out
            if rep:
                times[name].append(ms)
    return times


def summary(times):
    return {name: {"ms": round(statistics.median(t), 3), "all ms": [round(x, 3) for x in t]} for name, t in times.items()}


def real_facet(torch, sep, seed, yB):
    a, b = sep.facet_vectors(seed, yB)
    f = torch.zeros((yB, yB), dtype=torch.float64, device="cuda")
    for r in range(a.shape[0]):
        f.add_(torch.outer(torch.from_numpy(a[r].real.copy()).cuda(), torch.from_numpy(b[r].real.copy()).cuda()))
    return f


def one_facet(torch, sep, core, p, reps):
    """K1 and the finish of one full facet, complex128 against float64"""
    yB, yN = p["yB_size"], p["yN_size"]
    band = (0, yN)
    row = {}
    real = real_facet(torch, sep, 900, yB)
    promoted = real.to(torch.complex128)
    out = torch.empty((yB, yN), dtype=torch.complex128, device="cuda")
    out64 = torch.empty_like(out)
    times = alternate(torch, {
        "complex128": lambda: core.prepare_facet_band(promoted, yB, band, out=out),
        "float64": lambda: core.prepare_facet_band_float64(real, yB, band, out=out64),
    }, reps)
    row["K1"] = summary(times)
    row["K1"]["equal"] = bool(torch.equal(out, out64))
    row["K1"]["input GB"] = {"complex128": round(yB * yB * 16 / 1e9, 2), "float64": round(yB * yB * 8 / 1e9, 2)}
    row["K1"]["output GB"] = round(yB * yN * 16 / 1e9, 2)
    del promoted, real, out64
    release(torch)
    # the band accumulator of the finish: K1's output is as good as any (full band, every column touched)
    fin = torch.empty((yB, yB), dtype=torch.complex128, device="cuda")
    fin64 = torch.empty((yB, yB), dtype=torch.float64, device="cuda")
    times = alternate(torch, {
        "complex128": lambda: core.finish_facet_band(out, band, yB, yB, out=fin),
        "float64": lambda: core.finish_facet_band_float64(out, band, yB, yB, out=fin64),
    }, reps)
    row["finish"] = summary(times)
    row["finish"]["equal"] = bool(torch.equal(fin.real, fin64))
    row["finish"]["input GB"] = round(yB * yN * 16 / 1e9, 2)
    row["finish"]["output GB"] = {"complex128": round(yB * yB * 16 / 1e9, 2), "float64": round(yB * yB * 8 / 1e9, 2)}
    del out, fin, fin64
    release(torch)
    return row


def forward_passes(torch, sw, sep, cfg, p, args):
    yB, xA, N = p["yB_size"], p["xA_size"], p["N"]
    facet_cfgs = [sw.FacetConfig(j * yB, -j * yB, yB) for j in range(args.facets)]
    reals = [real_facet(torch, sep, 900 + j, yB) for j in range(args.facets)]
    step = N // args.waves // xA * xA
    offs = [i * step for i in range(args.waves)]
    plan = [sw.SubgridConfig(o0, o1, xA) for o1 in offs for o0 in offs]
    row, kept = {}, {}
    # (the float64 run first: the promoted copies exist only for the runs that read them)
    for name, axis, kw in (("wave_axis=1 float64", 1, dict(facet_dtype=torch.float64)), ("wave_axis=1 promoted", 1, {}),
                           ("wave_axis=0 promoted", 0, {})):
        facets = reals if kw else [f.to(torch.complex128) for f in reals]
        order = sorted(plan, key=(lambda c: (c.off1, c.off0)) if axis else (lambda c: (c.off0, c.off1)))
        times = []
        for rep in range(args.reps + 1):
            fwd = sw.SwiftlyForward(cfg, list(zip(facet_cfgs, facets)), subgrid_configs=plan, wave_axis=axis, **kw)
            assert fwd.facet_dtype == (torch.float64 if kw else torch.complex128)
            ms, out = timed(torch, lambda: fwd.get_subgrid_tasks(order))  # pylint: disable=cell-var-from-loop
            if rep:
                times.append(ms)
            if axis == 1 and rep == args.reps:
                kept[name] = [t.cpu() for t in out]
            del fwd, out
            release(torch)
        row[name] = {"ms": round(statistics.median(times), 2), "all ms": [round(t, 2) for t in times]}
        del facets
        release(torch)
    row["equal"] = all(torch.equal(a, b) for a, b in zip(kept["wave_axis=1 float64"], kept["wave_axis=1 promoted"]))
    row["ratio 0 / 1 float64"] = round(row["wave_axis=0 promoted"]["ms"] / row["wave_axis=1 float64"]["ms"], 3)
    row["ratio 0 / 1 promoted"] = round(row["wave_axis=0 promoted"]["ms"] / row["wave_axis=1 promoted"]["ms"], 3)
    return row


def backward_passes(torch, sw, sep, cfg, p, args):
    yB, xA, N = p["yB_size"], p["xA_size"], p["N"]
    facet_cfgs = [sw.FacetConfig(j * yB, -j * yB, yB) for j in range(args.facets)]
    step = N // args.waves // xA * xA
    offs = [i * step for i in range(args.waves)]
    plan = [sw.SubgridConfig(o0, o1, xA) for o1 in offs for o0 in offs]
    data = []
    for i in range(len(plan)):
        u, v = sep.subgrid_vectors(950 + i, xA)
        s = torch.zeros((xA, xA), dtype=torch.complex128, device="cuda")
        for r in range(u.shape[0]):
            s.add_(torch.outer(torch.from_numpy(u[r]).cuda(), torch.from_numpy(v[r]).cuda()))
        data.append(s)
    row, kept = {}, {}
    for name, axis, kw in (("wave_axis=1 float64", 1, dict(facet_dtype=torch.float64)), ("wave_axis=1 complex128", 1, {}),
                           ("wave_axis=0 complex128", 0, {}), ("wave_axis=0 float64", 0, dict(facet_dtype=torch.float64))):
        key = (lambda c: c.off1) if axis else (lambda c: c.off0)
        order = sorted(range(len(plan)), key=lambda i: key(plan[i]))  # pylint: disable=cell-var-from-loop
        sgs, subs = [plan[i] for i in order], [data[i] for i in order]
        times, finishes = [], []
        for rep in range(args.reps + 1):
            bwd = sw.SwiftlyBackward(cfg, facet_cfgs, subgrid_configs=plan, wave_axis=axis, dtype=torch.complex128, **kw)
            torch.cuda.synchronize()
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            marks[0].record()
            bwd.add_new_subgrid_tasks(sgs, subs)
            marks[1].record()
            out = bwd.finish()
            marks[2].record()
            torch.cuda.synchronize()
            if rep:
                times.append(marks[0].elapsed_time(marks[2]))
                finishes.append(marks[1].elapsed_time(marks[2]))
            native = bwd.real_finish_native
            if axis == 1 and rep == args.reps:
                kept[name] = out[0][:: 97].cpu()
            del bwd, out
            release(torch)
        row[name] = {"ms": round(statistics.median(times), 2), "finish ms": round(statistics.median(finishes), 2),
                     "all ms": [round(t, 2) for t in times], "real_finish_native": native}
    row["equal"] = bool(torch.equal(kept["wave_axis=1 float64"], kept["wave_axis=1 complex128"].real))
    row["ratio 0 / 1 float64"] = round(row["wave_axis=0 complex128"]["ms"] / row["wave_axis=1 float64"]["ms"], 3)
    row["ratio 0 / 1 complex128"] = round(row["wave_axis=0 complex128"]["ms"] / row["wave_axis=1 complex128"]["ms"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="64k[1]-n16k-1k,128k[1]-n32k-1k")
    ap.add_argument("--facets", type=int, default=2)
    ap.add_argument("--waves", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    import torch

    import ska_sdp_exec_swiftly_amd as sw
    from oracle import separable as sep
    from ska_sdp_exec_swiftly_amd import _lib

    results = []
    for name in args.configs.split(","):
        p = {k: sw.SWIFT_CONFIGS[name][k] for k in ("W", "fov", "N", "yB_size", "yN_size", "xA_size", "xM_size")}
        cfg = sw.SwiftlyConfig(backend="hip", **p)
        core = cfg.core
        if not (core.supports_real_facets_f64() and core.supports_real_facets_out_f64()):
            raise SystemExit(f"{name}: {_lib.last_error()}")
        row = {"config": name, "facets": args.facets, "subgrids": args.waves * args.waves, "waves": args.waves,
               "reps": args.reps, "build": _lib.build_info()}
        row["one facet"] = one_facet(torch, sep, core, p, args.reps)
        row["forward"] = forward_passes(torch, sw, sep, cfg, p, args)
        row["backward"] = backward_passes(torch, sw, sep, cfg, p, args)
        print(json.dumps(row), flush=True)
        results.append(row)
        release(torch)
    print("| configuration | stage | complex128 ms | float64 ms | float64 / complex128 | same bits |")
    print("|---|---|---|---|---|---|")
    for r in results:
        for stage in ("K1", "finish"):
            s = r["one facet"][stage]
            c, f = s["complex128"]["ms"], s["float64"]["ms"]
            print(f"| {r['config']} | {stage}, one facet | {c} | {f} | {round(f / c, 3)} | {s['equal']} |")
    print("| configuration | pass | wave_axis=0 ms | wave_axis=1 ms | wave_axis=1 float64 ms | ratio 0 / 1 | ratio 0 / 1 float64 |")
    print("|---|---|---|---|---|---|---|")
    for r in results:
        f, b = r["forward"], r["backward"]
        print(f"| {r['config']} | forward | {f['wave_axis=0 promoted']['ms']} | {f['wave_axis=1 promoted']['ms']} | "
              f"{f['wave_axis=1 float64']['ms']} | {f['ratio 0 / 1 promoted']} | {f['ratio 0 / 1 float64']} |")
        print(f"| {r['config']} | backward | {b['wave_axis=0 complex128']['ms']} | {b['wave_axis=1 complex128']['ms']} | "
              f"{b['wave_axis=1 float64']['ms']} | {b['ratio 0 / 1 complex128']} | {b['ratio 0 / 1 float64']} |")


if __name__ == "__main__":
    main()
