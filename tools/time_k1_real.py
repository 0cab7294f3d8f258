"""K1 of the contiguous-axis-first pipeline on a real-valued facet: the real-load form (float32 facet,
swiftly_hip_prepare_facet_band_real) against the complex form (the same facet promoted to complex64) at the facet shape of
the 64k workload -- a 22528^2 facet in 32768-point rows, band (10736, 11472), the three offsets of the 3 x 3 cover.

Both forms run in ONE process on one build, alternately (real, complex, real, ...), each repeat a HIP-event pair around
``--calls`` back-to-back launches, after a warm-up of both.  Prints one JSON line: per offset and over all offsets the median,
minimum, maximum and spread (max - min) of the per-facet time of each form in ms, the bytes each form reads from the facet,
and whether the two band buffers are equal (they must be).

Usage: python tools/time_k1_real.py [--repeats 7] [--calls 9] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-distributed-fourier-transform_amd"))
import torch  # noqa: E402

import ska_sdp_exec_swiftly_amd as sw  # noqa: E402

W, N, XM, YN, YB = 10.875, 65536, 1024, 32768, 22528
BAND = (10736, 11472)
OFFSETS = (0, 22528, -22528)


def stats(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), spread=max(ms) - min(ms), repeats=len(ms))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n", maxsplit=1)[0])
    ap.add_argument("--repeats", type=int, default=7, help="event pairs per form and offset (at least 5)")
    ap.add_argument("--calls", type=int, default=9, help="K1 launches inside one event pair")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    core = sw.SwiftlyCoreHip(W, N, XM, YN)
    if not core.supports_real_facets():
        raise SystemExit("no real-load K1 for this configuration: " + sw._lib.last_error())  # pylint: disable=protected-access
    gen = torch.Generator(device="cuda").manual_seed(7)
    real = torch.randn((YB, YB), device="cuda", dtype=torch.float32, generator=gen)
    cplx = real.to(torch.complex64)
    forms = (("real", real), ("complex", cplx))
    outs = {name: torch.zeros((YB, core.band_columns(BAND)), dtype=torch.complex64, device="cuda") for name, _ in forms}

    def timed(name, facet, off):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            core.prepare_facet_band(facet, off, BAND, out=outs[name])
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.calls

    per_offset, every, equal = {}, {name: [] for name, _ in forms}, True
    for off in OFFSETS:
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
    # the requirement: the real form's median is not above the complex form's by more than the spread of the complex
    # repeats -- per offset (same launch geometry) and over the pooled repeats
    def holds(st):
        return st["real"]["median"] <= st["complex"]["median"] + st["complex"]["spread"]

    for st in per_offset.values():
        st["real_not_slower_beyond_complex_spread"] = holds(st)
    result = dict(
        tool="time_k1_real", device=torch.cuda.get_device_name(0), build=sw._lib.build_info(),  # pylint: disable=protected-access
        shape=dict(facet=[YB, YB], yN=YN, band=list(BAND), offsets=list(OFFSETS), calls_per_repeat=args.calls),
        facet_bytes=dict(real=real.numel() * 4, complex=cplx.numel() * 8), unit="ms per facet",
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


if __name__ == "__main__":
    main()
