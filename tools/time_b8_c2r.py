"""B8 of the backward band pass (finish_facet_band: the contiguous-axis finish of a band accumulator) with real-valued
output, three forms: the complex form, the real-store form (float32 facet, swiftly_hip_finish_facet_band_real: the whole
complex transform in two workgroups per row, real part stored) and the half-length form (swiftly_hip_finish_facet_band_c2r:
one 16384-point transform in one workgroup per row) at the facet shape of the 64k workload -- one 22528^2 facet out of a
band accumulator [22528, 11472] in 32768-point rows, band (10736, 11472), the three facet offsets and cover masks of the
3 x 3 cover.

The forms run in ONE process on one build, alternately (half, real, complex, half, ...), each repeat a HIP-event pair around
``--calls`` back-to-back launches, after a warm-up of all.  Prints one JSON line: per offset and over all offsets the median,
minimum, maximum and spread (max - min) of the per-facet time of each form in ms, the bytes each form writes, the relative
RMSE of the half-length output against the real-store output (different rounding, the same quantity), and the verdict by the
rule of DESIGN.md section 6: faster only if the medians differ by more than BOTH forms' spread.

Usage: python tools/time_b8_c2r.py [--repeats 7] [--calls 5] [--out FILE]"""
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
from ska_sdp_exec_swiftly_amd.config import make_full_cover_config  # noqa: E402

W, N, XM, YN, YB = 10.875, 65536, 1024, 32768, 22528
BAND = (10736, 11472)
FORMS = ("half", "real", "complex")


def stats(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), spread=max(ms) - min(ms), repeats=len(ms))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n", maxsplit=1)[0])
    ap.add_argument("--repeats", type=int, default=7, help="event pairs per form and offset (at least 5)")
    ap.add_argument("--calls", type=int, default=5, help="finish launches inside one event pair")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    core = sw.SwiftlyCoreHip(W, N, XM, YN)
    if not core.supports_real_facets_out_c2r():
        raise SystemExit("no half-length finish for this configuration: " + sw._lib.last_error())  # pylint: disable=protected-access
    # the facets of one row of the cover: their off1 and mask1
    cover = [c for c in make_full_cover_config(N, YB, sw.FacetConfig) if c.off0 == 0]
    gen = torch.Generator(device="cuda").manual_seed(8)
    acc = torch.randn((YB, BAND[1]), device="cuda", dtype=torch.complex64, generator=gen)
    outs = dict(half=torch.zeros((YB, YB), dtype=torch.float32, device="cuda"),
                real=torch.zeros((YB, YB), dtype=torch.float32, device="cuda"),
                complex=torch.zeros((YB, YB), dtype=torch.complex64, device="cuda"))

    def timed(name, cfg):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            core.finish_facet_band(acc, BAND, cfg.off1, YB, mask=cfg.mask1, out=outs[name], real=name != "complex",
                                   half_length=name == "half")
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.calls

    per_offset, every, equal, relrmse = {}, {name: [] for name in FORMS}, True, {}
    for cfg in cover:
        for name in FORMS:  # warm-up of every form at this offset: code objects, mask upload, clocks
            timed(name, cfg)
        equal = equal and bool(torch.equal(outs["real"], outs["complex"].real))
        diff = (outs["half"].double() - outs["real"].double()).pow(2).mean().sqrt()
        relrmse[str(cfg.off1)] = float(diff / outs["real"].double().pow(2).mean().sqrt())
        ms = {name: [] for name in FORMS}
        for _ in range(args.repeats):
            for name in FORMS:
                ms[name].append(timed(name, cfg))
        per_offset[str(cfg.off1)] = {name: stats(v) for name, v in ms.items()}
        for name, v in ms.items():
            every[name].extend(v)
    total = {name: stats(v) for name, v in every.items()}

    # is the half-length form faster than the real-store one by more than both forms' spread?
    def faster(st):
        return st["half"]["median"] < st["real"]["median"] - max(st["half"]["spread"], st["real"]["spread"])

    def slower(st):
        return st["half"]["median"] > st["real"]["median"] + max(st["half"]["spread"], st["real"]["spread"])

    for st in per_offset.values():
        st["half_faster_beyond_both_spreads"] = faster(st)
        st["half_slower_beyond_both_spreads"] = slower(st)
    result = dict(
        tool="time_b8_c2r", device=torch.cuda.get_device_name(0), build=sw._lib.build_info(),  # pylint: disable=protected-access
        shape=dict(facet=[YB, YB], yN=YN, band=list(BAND), offsets=[c.off1 for c in cover], calls_per_repeat=args.calls),
        bytes_read=acc.numel() * 8, bytes_written=dict(half=YB * YB * 4, real=YB * YB * 4, complex=YB * YB * 8), unit="ms per facet",
        per_offset=per_offset, all_offsets=total, real_equals_complex_real_part=equal,
        half_relrmse_against_real=relrmse,
        half_over_real_median=total["half"]["median"] / total["real"]["median"],
        half_minus_real_median=total["half"]["median"] - total["real"]["median"],
        half_faster_beyond_both_spreads=faster(total), half_slower_beyond_both_spreads=slower(total),
    )
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as fh:
            fh.write(line + "\n")
    if not equal:
        raise SystemExit("the real-store output is not the real part of the complex one")
    if max(relrmse.values()) > 4e-6:
        raise SystemExit(f"the half-length output is not the real-store one within two transform bounds: {relrmse}")


if __name__ == "__main__":
    main()
