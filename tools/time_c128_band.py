"""Time a complex128 SwiftlyForward pass with the reference schedule (wave_axis=0) and the contiguous-axis-first
pipeline (wave_axis=1) on the W = 13.5625 catalogue entries that need complex128 ("complex128 at
yN = 16384 / 32768").

One pass = a fresh SwiftlyForward over device-resident facets, K1 included, serving a planned set of subgrids (all
subgrids of a few waves: ``--waves`` off1 values x ``--waves`` off0 values), bracketed by HIP events; median of
``--reps`` passes after one warm-up pass.  Also prints the algorithmic bytes per kernel group of one pass of each
pipeline (every kernel reads its input and writes its output once; four-step scratch counted both ways).

    python tools/time_c128_band.py [--configs 64k[1]-n16k-1k,128k[1]-n32k-1k] [--facets 2] [--waves 4] [--reps 5]
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


def bytes_per_pass(p, F, n_off0, n_off1, m):
    """algorithmic bytes of one pass per kernel group, both pipelines (S = n_off0 * n_off1 subgrids)"""
    yB, yN, xM, xA = p["yB_size"], p["yN_size"], p["xM_size"], p["xA_size"]
    S = n_off0 * n_off1
    rows = min(yN, n_off0 * m)  # padded-facet rows a wave keeps (row map of its subgrids)
    sub_side = S * (F * m * m + 2 * xM * xA + xA * xA) * C  # sum_finish_facets + K5b (four-step scratch not counted)
    w1 = {
        "K1 prepare_facet_band (axis 1, whole padded axis)": F * yB * (yB + yN) * C,
        "K2 prepare_facet_columns (yN four-step, per pass)": n_off1 * F * (yB * m + 2 * yN * m + rows * m) * C,
        "K3 transform_contributions": n_off1 * F * (rows * m + n_off0 * m * m) * C,
        "K4b-K5 sum_finish_facets + finish_subgrid": sub_side,
    }
    w0 = {
        "K1 prepare_facet (axis 0, four-step)": F * yB * (yB + 2 * yN + rows * n_off0 // max(n_off0, 1)) * C,
        "K2 extract_column (axis 1, per wave)": n_off0 * F * (m * yB + m * yN) * C,
        "K3-K5 (per-wave subgrid side)": S * F * (2 * m * m) * C + sub_side,
    }
    return {"wave_axis=0": w0, "wave_axis=1": w1}


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

    results = []
    for name in args.configs.split(","):
        p = {k: sw.SWIFT_CONFIGS[name][k] for k in ("W", "fov", "N", "yB_size", "yN_size", "xA_size", "xM_size")}
        cfg = sw.SwiftlyConfig(backend="hip", **p)
        yB, xA, N = p["yB_size"], p["xA_size"], p["N"]
        facet_cfgs = [sw.FacetConfig(j * yB, -j * yB, yB) for j in range(args.facets)]
        facets = []
        for j, c in enumerate(facet_cfgs):
            a, b = sep.facet_vectors(900 + j, yB)
            f = torch.zeros((yB, yB), dtype=torch.complex128, device="cuda")
            for r in range(a.shape[0]):
                f.add_(torch.outer(torch.from_numpy(a[r]).cuda(), torch.from_numpy(b[r]).cuda()))
            facets.append(f)
        step = N // args.waves // xA * xA
        offs = [i * step for i in range(args.waves)]
        plan = [sw.SubgridConfig(o0, o1, xA) for o1 in offs for o0 in offs]
        row = {"config": name, "facets": args.facets, "subgrids": len(plan), "waves": args.waves}
        for axis in (0, 1):
            order = sorted(plan, key=(lambda c: (c.off1, c.off0)) if axis else (lambda c: (c.off0, c.off1)))
            times = []
            for rep in range(args.reps + 1):
                fwd = sw.SwiftlyForward(cfg, list(zip(facet_cfgs, facets)), subgrid_configs=plan, wave_axis=axis)
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                out = fwd.get_subgrid_tasks(order)
                t1.record()
                torch.cuda.synchronize()
                if rep:
                    times.append(t0.elapsed_time(t1))
                del fwd, out
                gc.collect()
                torch.cuda.empty_cache()
            row[f"wave_axis={axis} ms"] = round(statistics.median(times), 2)
            row[f"wave_axis={axis} all ms"] = [round(t, 2) for t in times]
        row["speedup"] = round(row["wave_axis=0 ms"] / row["wave_axis=1 ms"], 3)
        row["bytes"] = bytes_per_pass(p, args.facets, args.waves, args.waves, cfg.core.xM_yN_size)
        print(json.dumps(row), flush=True)
        results.append(row)
        del facets
        gc.collect()
        torch.cuda.empty_cache()
    print("| configuration | facets | subgrids | wave_axis=0 ms | wave_axis=1 ms | speed-up |")
    print("|---|---|---|---|---|---|")
    for r in results:
        print(f"| {r['config']} | {r['facets']} | {r['subgrids']} | {r['wave_axis=0 ms']} | {r['wave_axis=1 ms']} | "
              f"{r['speedup']} |")


if __name__ == "__main__":
    main()
