"""K1 of the axis-1-first pipeline (whole-row kernel with the window epilogue, core.prepare_facet_window_rows) on one 22528^2
facet of the 64k workload for different window counts, beside the band store of the two-workgroup kernel: what the epilogue
costs per round of eight windows.  HIP events around 5 launches, best of 5.

``--real [--repeats 7] [--calls 5] [--out FILE]``: the real-load form of that K1 (a float32 facet,
swiftly_hip_prepare_facet_window_rows_real) against the complex form (the same facet promoted to complex64) instead: the
plan's band and its 25 windows, the three offsets of the 3 x 3 cover, both forms alternating in ONE process on one build
(complex, real, complex, ...), each repeat a HIP-event pair around ``--calls`` back-to-back launches, after a warm-up of
both.  Prints one JSON line (and writes it to FILE): per offset and over all offsets the median, minimum, maximum and spread
(max - min) of the per-facet time of each form in ms, the bytes each form reads from the facet, and whether the two outputs
are equal (they must be).  The yardstick of the real form is the complex form of the same run."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-distributed-fourier-transform_amd"))
import torch  # noqa: E402

import bench  # noqa: E402
import ska_sdp_exec_swiftly_amd as sw  # noqa: E402

wl = bench.WORKLOADS["64k-sparse"]
p = wl["params"]
cfg = sw.SwiftlyConfig(backend="hip", **p)
core = cfg.core
sgs = bench.select_subgrids(sw.make_full_subgrid_cover(cfg), p["N"], p["xA_size"], wl["sparse_radius"])
keys = sorted({c.off1 for c in sgs})
band = core.band_for_offsets(keys)
yB = p["yB_size"]


def real_leg(argv):
    ap = argparse.ArgumentParser(description="real against complex window-rows K1")
    ap.add_argument("--real", action="store_true")
    ap.add_argument("--repeats", type=int, default=7, help="event pairs per form and offset (at least 7)")
    ap.add_argument("--calls", type=int, default=5, help="K1 launches inside one event pair")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    if args.repeats < 7:
        ap.error("--repeats must be at least 7")
    offsets = (0, 22528, -22528)
    if not core.supports_window_rows(band, yB, offsets, n_windows=len(keys), real=True):
        raise SystemExit("no real window-rows K1 for this plan: " + sw._lib.last_error())  # pylint: disable=protected-access
    gen = torch.Generator(device="cuda").manual_seed(7)
    real = torch.randn((yB, yB), device="cuda", dtype=torch.float32, generator=gen)
    forms = (("complex", real.to(torch.complex64)), ("real", real))
    starts = torch.tensor(core.window_starts(band, keys), dtype=torch.int32, device="cuda")
    outs = {name: torch.zeros((len(keys), yB, 512), dtype=torch.complex64, device="cuda") for name, _ in forms}

    def stats(ms):
        return dict(median=statistics.median(ms), min=min(ms), max=max(ms), spread=max(ms) - min(ms), repeats=len(ms))

    def timed(name, facet, off):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            core.prepare_facet_window_rows(facet, off, band, starts, outs[name])
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.calls

    per_offset, every, equal = {}, {name: [] for name, _ in forms}, True
    for off in offsets:
        for name, facet in forms:  # warm-up of both forms at this offset: code objects, window table, clocks
            timed(name, facet, off)
        equal = equal and bool(torch.equal(outs["real"], outs["complex"]))
        ms = {name: [] for name, _ in forms}
        for _ in range(args.repeats):
            for name, facet in forms:
                ms[name].append(timed(name, facet, off))
        per_offset[str(off)] = {name: stats(v) for name, v in ms.items()}
        for name, v in ms.items():
            every[name].extend(v)
    total = {name: stats(v) for name, v in every.items()}

    def holds(st):  # the real form's median is not above the complex form's by more than the spread of the complex repeats
        return st["real"]["median"] <= st["complex"]["median"] + st["complex"]["spread"]

    for st in per_offset.values():
        st["real_not_slower_beyond_complex_spread"] = holds(st)
    result = dict(
        tool="time_k1_window_rows --real", device=torch.cuda.get_device_name(0), build=sw._lib.build_info(),  # pylint: disable=protected-access
        shape=dict(facet=[yB, yB], yN=p["yN_size"], band=list(band), windows=len(keys), offsets=list(offsets),
                   calls_per_repeat=args.calls),
        facet_bytes=dict(real=real.numel() * 4, complex=real.numel() * 8), unit="ms per facet",
        per_offset=per_offset, all_offsets=total, outputs_equal=equal,
        real_minus_complex_median=total["real"]["median"] - total["complex"]["median"],
        real_not_slower_beyond_complex_spread=holds(total) and all(holds(st) for st in per_offset.values()),
    )
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as fh:
            fh.write(line + "\n")
    if not equal:
        raise SystemExit("the real and the complex form disagree")


if "--real" in sys.argv[1:]:
    real_leg(sys.argv[1:])
    sys.exit(0)

facet = torch.randn((yB, yB), device="cuda", dtype=torch.complex64)


def timed(fn, reps=5, rounds=5):
    best = 1e9
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / reps)
    return best


out = core.prepare_facet_band(facet, 22528, band)
print(f"band store (two workgroups per row): {timed(lambda: core.prepare_facet_band(facet, 22528, band, out=out)):.3f} ms")
for n in [int(a) for a in sys.argv[1:]] or (1, 8, 9, 16, 24, 25):
    use = (keys * 2)[:n]
    starts = torch.tensor(core.window_starts(band, use), dtype=torch.int32, device="cuda")
    rows = torch.empty((n, yB, 512) if os.environ.get("LAYOUT", "wave") == "wave" else (yB, n * 512), dtype=torch.complex64, device="cuda")
    t = timed(lambda: core.prepare_facet_window_rows(facet, 22528, band, starts, rows))
    print(f"window rows, {n:2d} windows: {t:.3f} ms")
