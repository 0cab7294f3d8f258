"""Time the device point-source check (``DeviceSources.check_subgrids``) over the 505 subgrids of the 64k-sparse plan
(bench.py's default workload: N = 65536, xA = 928) against the host ``check_subgrid`` of ``api_helper`` on ONE of those
subgrids ("point-source checks").

The approximation is the device truth itself in complex64, resident on the device; one timed call checks all 505
subgrids (one launch of the rank-S kernel, the phase tables included), bracketed by HIP events, median of ``--reps``
calls after a warm-up.  The host time is one ``check_subgrid`` call on a subgrid already copied to the host (the copy
is timed separately).

    python tools/time_sources.py [--sources 13,1000] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ska-sdp-distributed-fourier-transform_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", default="13,1000")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    import numpy
    import torch

    import bench
    import ska_sdp_exec_swiftly_amd as sw
    from ska_sdp_exec_swiftly_amd.config import make_full_cover_config

    wl = bench.WORKLOADS["64k-sparse"]
    N, xA = wl["params"]["N"], wl["params"]["xA_size"]
    plan = bench.select_subgrids(make_full_cover_config(N, xA, sw.SubgridConfig), N, xA, wl["sparse_radius"])
    rows = []
    for S in (int(s) for s in args.sources.split(",")):
        rng = numpy.random.default_rng(S)
        sources = [(float(rng.uniform(0.5, 1.5)), int(a), int(b)) for a, b in rng.integers(-N // 2, N // 2, size=(S, 2))]
        dsrc = sw.DeviceSources(sources, N)
        approx = dsrc.subgrids(plan, dtype=torch.complex64)
        times = []
        for rep in range(args.reps + 1):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            errs = dsrc.check_subgrids(plan, approx)
            t1.record()
            torch.cuda.synchronize()
            if rep:
                times.append(t0.elapsed_time(t1))
        t = time.perf_counter()
        one = approx[len(plan) // 2].cpu().numpy()
        copy_s = time.perf_counter() - t
        t = time.perf_counter()
        host_err = sw.check_subgrid(N, plan[len(plan) // 2], one, sources)
        host_s = time.perf_counter() - t
        dev_ms = statistics.median(times)
        rows.append({
            "sources": S, "records": len(dsrc), "subgrids": len(plan), "size": xA,
            "device check_subgrids ms (all subgrids)": round(dev_ms, 2), "all ms": [round(x, 2) for x in times],
            "host check_subgrid ms (one subgrid)": round(host_s * 1e3, 1), "host copy ms (one subgrid)": round(copy_s * 1e3, 2),
            "host time for all subgrids / device time": round(host_s * 1e3 * len(plan) / dev_ms, 1),
            "max RMSE device": float(errs[:, 0].max()), "RMSE host (that subgrid)": float(host_err),
            "device RMSE (that subgrid)": float(errs[len(plan) // 2, 0]),
        })
        print(json.dumps(rows[-1]), flush=True)
        del approx, dsrc
        torch.cuda.empty_cache()
    print("| sources | device, 505 subgrids (ms) | host, one subgrid (ms) | host x 505 / device |")
    print("|---|---|---|---|")
    for r in rows:
        print(f"| {r['sources']} | {r['device check_subgrids ms (all subgrids)']} | {r['host check_subgrid ms (one subgrid)']} | "
              f"{r['host time for all subgrids / device time']} |")


if __name__ == "__main__":
    main()
