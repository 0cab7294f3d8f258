"""K1 of the contiguous-axis-first pipeline on a real-valued facet, three forms: the complex form (the facet promoted to
complex64), the real-load form (float32 facet, swiftly_hip_prepare_facet_band_real: two workgroups per row, each a
16384-point half of the 32768-point complex transform) and the half-length form (swiftly_hip_prepare_facet_band_rfft: one
workgroup per row, one 16384-point transform and a recombination) -- at the facet shape of the 64k workload, a 22528^2
facet in 32768-point rows, band (10736, 11472), the three offsets of the 3 x 3 cover.  The method of tools/time_k1_real.py.

The forms run in ONE process on one build, alternately (complex, real, half_length, complex, ...), each repeat a HIP-event
pair around ``--calls`` back-to-back launches, after a warm-up of all three.  Prints one JSON line: per offset and over all
offsets the median, minimum, maximum and spread (max - min) of the per-facet time of each form in ms, the half-length form
against the real form by the rule of DESIGN.md section 6 (a difference counts only beyond BOTH forms' spread), and the
relative RMS difference of the half-length band buffer from the real form's (they round differently; the real and the
complex form must be equal).

Usage: python tools/time_k1_rfft.py [--repeats 7] [--calls 9] [--out FILE]"""
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
FORMS = ("complex", "real", "half_length")


def stats(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), spread=max(ms) - min(ms), repeats=len(ms))


def verdict(st):
    """half-length against real: 'faster' / 'slower' when the medians differ by more than both spreads, else 'same'"""
    diff = st["half_length"]["median"] - st["real"]["median"]
    if abs(diff) <= max(st["half_length"]["spread"], st["real"]["spread"]):
        return "same"
    return "faster" if diff < 0 else "slower"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n", maxsplit=1)[0])
    ap.add_argument("--repeats", type=int, default=7, help="event pairs per form and offset (at least 5)")
    ap.add_argument("--calls", type=int, default=9, help="K1 launches inside one event pair")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    core = sw.SwiftlyCoreHip(W, N, XM, YN)
    if not core.supports_real_facets_rfft():
        raise SystemExit("no half-length K1 for this configuration: " + sw._lib.last_error())  # pylint: disable=protected-access
    gen = torch.Generator(device="cuda").manual_seed(7)
    real = torch.randn((YB, YB), device="cuda", dtype=torch.float32, generator=gen)
    facets = dict(complex=real.to(torch.complex64), real=real, half_length=real)
    outs = {name: torch.zeros((YB, core.band_columns(BAND)), dtype=torch.complex64, device="cuda") for name in FORMS}

    def timed(name, off):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            core.prepare_facet_band(facets[name], off, BAND, out=outs[name], half_length=name == "half_length")
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.calls

    per_offset, every, equal, rel = {}, {name: [] for name in FORMS}, True, 0.0
    for off in OFFSETS:
        for name in FORMS:  # warm-up of every form at this offset: code objects, window table, clocks
            timed(name, off)
        equal = equal and bool(torch.equal(outs["real"], outs["complex"]))
        diff = (outs["half_length"] - outs["real"]).abs().square().mean().sqrt() / outs["real"].abs().square().mean().sqrt()
        rel = max(rel, float(diff))
        ms = {name: [] for name in FORMS}
        for _ in range(args.repeats):
            for name in FORMS:
                ms[name].append(timed(name, off))
        per_offset[str(off)] = {name: stats(v) for name, v in ms.items()}
        per_offset[str(off)]["half_length_against_real"] = verdict(per_offset[str(off)])
        for name, v in ms.items():
            every[name].extend(v)
    total = {name: stats(v) for name, v in every.items()}
    result = dict(
        tool="time_k1_rfft", device=torch.cuda.get_device_name(0), build=sw._lib.build_info(),  # pylint: disable=protected-access
        shape=dict(facet=[YB, YB], yN=YN, band=list(BAND), offsets=list(OFFSETS), calls_per_repeat=args.calls),
        facet_bytes=dict(complex=real.numel() * 8, real=real.numel() * 4, half_length=real.numel() * 4), unit="ms per facet",
        per_offset=per_offset, all_offsets=total, real_equals_complex=equal,
        half_length_relative_rms_difference_from_real=rel,
        half_length_over_real_median=total["half_length"]["median"] / total["real"]["median"],
        half_length_against_real=verdict(total),
    )
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as fh:
            fh.write(line + "\n")
    if not equal:
        raise SystemExit("the real and the complex form disagree")
    if not rel < 1e-5:
        raise SystemExit(f"the half-length form is {rel:.2e} away from the real form")


if __name__ == "__main__":
    main()
