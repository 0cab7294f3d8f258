"""Time a complex128 SwiftlyBackward pass with the reference schedule (wave_axis=0) and the band schedule
(wave_axis=1, dtype=complex128) on the W = 13.5625 catalogue entries that need complex128 (DESIGN.md section 4,
"complex128 backward band schedule").

One pass = a fresh SwiftlyBackward that folds a planned set of device-resident subgrids (``--waves`` off1 values x
``--waves`` off0 values, whole waves in the order of the schedule's wave key) into ``--facets`` facets, ``finish()``
included, bracketed by HIP events; median of ``--reps`` passes after one warm-up pass.  The three stages of a pass
(contributions of the subgrid side, accumulation, finish) are bracketed separately.  Also prints the algorithmic bytes per
stage of one pass of each schedule (every kernel reads its input and writes its output once; the four-step scratch of the
facet-side transforms counted both ways, that of the subgrid side not counted).

    python tools/time_c128_backward.py [--configs 64k[1]-n16k-1k,128k[1]-n32k-1k] [--facets 2] [--waves 4] [--reps 5]
"""
import argparse
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ska-sdp-distributed-fourier-transform_amd")]

C = 16  # bytes per complex128 value
STAGES = ("contributions", "accumulate", "finish")


def bytes_per_pass(p, F, n_off0, n_off1, m, band_len):
    """algorithmic bytes of one pass per stage, both schedules (S = n_off0 * n_off1 subgrids)"""
    yB, yN, xM, xA = p["yB_size"], p["yN_size"], p["xM_size"], p["xA_size"]
    S = n_off0 * n_off1
    sub_side = S * (xA * xA + 2 * xM * xA + 2 * F * m * m) * C  # prepare axis 0, split_prepare_facets + its column pass in place
    w1 = {
        "contributions": sub_side,
        # per wave: the m x m blocks read once, the yN-point four-step through its scratch, m band columns written (read
        # again where an earlier wave touched them: not counted)
        "accumulate": n_off1 * F * (n_off0 * m * m + 2 * yN * m + yB * m) * C,
        "finish": F * yB * (band_len + yB) * C,  # finish_facet_band: the band rows in, the facet out
    }
    w0 = {
        "contributions": sub_side,
        # per off0 column: zero fill of [m, yN], one read-modify-write of m x m per subgrid; per evicted column the
        # contiguous-axis finish [m, yN] -> [m, yB] and its read-modify-write into the [yN, yB] accumulator (zero-filled once)
        "accumulate": F * (n_off0 * m * yN + S * 3 * m * m + n_off0 * (m * yN + m * yB + 3 * m * yB) + yN * yB) * C,
        "finish": F * (yN * yB + 2 * yN * yB + yB * yB) * C,  # strided-axis four-step over the whole accumulator
    }
    return {"wave_axis=0": w0, "wave_axis=1": w1}


def one_pass(sw, torch, cfg, facet_cfgs, plan, data, axis):
    """one pass in whole waves through the stage entry points; returns (total ms, ms per stage)"""
    kw = dict(dtype=torch.complex128) if axis else {}
    bwd = sw.SwiftlyBackward(cfg, facet_cfgs, subgrid_configs=plan, wave_axis=axis, **kw)
    key = (lambda c: c.off1) if axis else (lambda c: c.off0)
    waves = {}
    for i, c in enumerate(plan):
        waves.setdefault(key(c), []).append(i)
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True)]
    marks[0].record()
    kinds = []

    def mark(kind):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        marks.append(ev)
        kinds.append(kind)

    for k in sorted(waves):
        sgs = [plan[i] for i in waves[k]]
        parts = bwd.wave_contributions(sgs, [data[i] for i in waves[k]])
        mark("contributions")
        bwd.accumulate_wave(sgs, parts)
        mark("accumulate")
    out = bwd.finish()
    mark("finish")
    torch.cuda.synchronize()
    stage = {s: 0.0 for s in STAGES}
    for a, b, kind in zip(marks, marks[1:], kinds):
        stage[kind] += a.elapsed_time(b)
    total = marks[0].elapsed_time(marks[-1])
    band_len = bwd.bands.band[1] if axis and bwd.bands.band else 0
    del bwd, out
    return total, stage, band_len


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
        if not core.supports_backward_band(torch.complex128, explicit=True):
            raise SystemExit(f"{name}: {_lib.last_error()}")
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
        row = {"config": name, "facets": args.facets, "subgrids": len(plan), "waves": args.waves,
               "split_prepare": bool(core.supports_split_prepare(torch.complex128, args.facets))}
        band_len = 0
        for axis in (0, 1):
            times, stages = [], {s: [] for s in STAGES}
            for rep in range(args.reps + 1):
                total, stage, bl = one_pass(sw, torch, cfg, facet_cfgs, plan, data, axis)
                band_len = max(band_len, bl)
                if rep:
                    times.append(total)
                    for s in STAGES:
                        stages[s].append(stage[s])
                gc.collect()
                torch.cuda.empty_cache()
            row[f"wave_axis={axis} ms"] = round(statistics.median(times), 2)
            row[f"wave_axis={axis} all ms"] = [round(t, 2) for t in times]
            row[f"wave_axis={axis} stages ms"] = {s: round(statistics.median(stages[s]), 2) for s in STAGES}
        row["band columns"] = band_len
        row["speedup"] = round(row["wave_axis=0 ms"] / row["wave_axis=1 ms"], 3)
        row["bytes"] = bytes_per_pass(p, args.facets, args.waves, args.waves, core.xM_yN_size, band_len)
        print(json.dumps(row), flush=True)
        results.append(row)
        del data
        gc.collect()
        torch.cuda.empty_cache()
    print("| configuration | facets | subgrids | schedule | contributions ms | accumulate ms | finish ms | pass ms |")
    print("|---|---|---|---|---|---|---|---|")
    for r in results:
        for axis in (0, 1):
            st = r[f"wave_axis={axis} stages ms"]
            print(f"| {r['config']} | {r['facets']} | {r['subgrids']} | wave_axis={axis} | {st['contributions']} | "
                  f"{st['accumulate']} | {st['finish']} | {r[f'wave_axis={axis} ms']} |")
    for r in results:
        print(f"{r['config']}: wave_axis=0 / wave_axis=1 = {r['speedup']}")
        for axis in (0, 1):
            gb = {s: round(b / 1e9, 2) for s, b in r["bytes"][f"wave_axis={axis}"].items()}
            print(f"  wave_axis={axis} algorithmic GB per stage: {gb}")


if __name__ == "__main__":
    main()
