"""
Times the complex128 long-row transforms (yN = 16384 / 32768) on one full facet of 64k[1]-n16k-1k and of
128k[1]-n32k-1k from seeded device data, with HIP events after warm-up (median of --reps):

  prepare_facet along axis 0 (strided four-step) and axis 1 (contiguous four-step, csrc/swiftly_rowslong.h),
  finish_facet along both axes, and one reference-schedule SwiftlyForward pass (one facet, --subgrids subgrids).

Per transform call: time, algorithmic bytes (input + output), bytes including the round trip through the four-step
scratch (written once, read once), and both rates.  A timing script, not a test.

    python tools/time_c128_long.py [--reps 5] [--warmup 2] [--subgrids 6] [--only 64k[1]-n16k-1k]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ska-sdp-distributed-fourier-transform_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

ENTRIES = {
    "64k[1]-n16k-1k": dict(W=13.5625, fov=1.0, N=65536, yB_size=13312, yN_size=16384, xA_size=896, xM_size=1024),
    "128k[1]-n32k-1k": dict(W=13.5625, fov=1.0, N=131072, yB_size=26624, yN_size=32768, xA_size=896, xM_size=1024),
}
ESZ = 16  # bytes per complex128 element


def timed(torch, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return sorted(times)[len(times) // 2]


def report(rows, name, what, ms, alg, scratch):
    tot = alg + scratch
    r = dict(entry=name, call=what, ms=round(ms, 3), alg_GB=round(alg / 1e9, 2), total_GB=round(tot / 1e9, 2),
             alg_TBps=round(alg / ms / 1e9, 2), total_TBps=round(tot / ms / 1e9, 2))
    rows.append(r)
    print(f"{name:16s} {what:26s} {ms:9.3f} ms  alg {alg / 1e9:6.2f} GB {alg / ms / 1e9:5.2f} TB/s   "
          f"with scratch {tot / 1e9:6.2f} GB {tot / ms / 1e9:5.2f} TB/s", flush=True)


def run_entry(torch, sw, name, p, args, rows):
    core = sw.SwiftlyConfig(backend="hip", **p).core
    yB, yN = p["yB_size"], p["yN_size"]
    gen = torch.Generator(device="cuda").manual_seed(11)
    facet = torch.randn((yB, yB), dtype=torch.complex128, device="cuda", generator=gen)
    off = 17 * (p["N"] // p["xM_size"])
    big = yB * yN * ESZ  # one prepared facet [yN, yB]
    scr = 2 * big        # four-step scratch: written by pass A, read by pass B
    for axis in (0, 1):
        shape = (yN, yB) if axis == 0 else (yB, yN)
        out = torch.empty(shape, dtype=torch.complex128, device="cuda")
        ms = timed(torch, lambda: core.prepare_facet(facet, off, axis=axis, out=out), args.reps, args.warmup)
        report(rows, name, f"prepare_facet axis={axis}", ms, yB * yB * ESZ + big, scr)
        res = torch.empty((yB, yB), dtype=torch.complex128, device="cuda")
        ms = timed(torch, lambda: core.finish_facet(out, off, yB, axis=axis, out=res), args.reps, args.warmup)
        report(rows, name, f"finish_facet axis={axis}", ms, big + yB * yB * ESZ, scr)
        del out, res
        torch.cuda.empty_cache()
    xA = p["xA_size"]
    sgs = [sw.SubgridConfig(k * 3 * xA, (k * 5 % 11) * xA, xA) for k in range(args.subgrids)]
    fcfg = [sw.FacetConfig(0, 0, yB)]
    cfg = sw.SwiftlyConfig(backend="hip", **p)

    def forward():
        fwd = sw.SwiftlyForward(cfg, list(zip(fcfg, [facet])), subgrid_configs=sgs)
        fwd.get_subgrid_tasks(sorted(sgs, key=lambda c: c.off0))

    ms = timed(torch, forward, max(1, args.reps // 2), 1)
    r = dict(entry=name, call=f"SwiftlyForward 1 facet x {len(sgs)} subgrids", ms=round(ms, 3))
    rows.append(r)
    print(f"{name:16s} {r['call']:26s} {ms:9.3f} ms", flush=True)
    del facet
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--subgrids", type=int, default=6)
    ap.add_argument("--only", choices=list(ENTRIES), default=None)
    args = ap.parse_args()
    import torch

    import ska_sdp_exec_swiftly_amd as sw

    rows = []
    for name, p in ENTRIES.items():
        if args.only in (None, name):
            run_entry(torch, sw, name, p, args, rows)
    print(json.dumps(dict(tool="time_c128_long", results=rows)))


if __name__ == "__main__":
    main()
