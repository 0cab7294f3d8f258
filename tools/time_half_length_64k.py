"""The half-length forms on 65536-point rows against the two-workgroup forms they replace, at the facet shape of the 128k
workload (128k[1]-n64k-1k: 3 x 3 facets of 45056^2 in 65536-point rows, full subgrid cover, so the band is the whole padded
axis): the 64k twin of tools/time_k1_rfft.py and tools/time_b8_c2r.py.

A 45056^2 facet with its band buffer does not leave room for several forms side by side, so every call works on a ROW
BLOCK of the facet -- ``--rows`` rows (default 4096: 16 workgroups of the one-workgroup-per-CU kernels for each of the 256
CUs) of 45056 columns -- and the per-facet time is the block's time scaled by 45056 / rows.

  k1: real (float32 rows, swiftly_hip_prepare_facet_band_rows_real: BandGeo64k, two workgroups per row, each loading and
      windowing the whole row) against half_length (swiftly_hip_prepare_facet_band_rows_rfft: one 32768-point transform in
      one workgroup per row), rows [0, rows) of a 45056-row facet, the other axis' window folded
  b8: real (swiftly_hip_finish_facet_band_real) against half (swiftly_hip_finish_facet_band_c2r) on a band accumulator
      [rows, band length] with the cover masks of the three facet columns

The forms run in ONE process on one build, alternately, each repeat a HIP-event pair around ``--calls`` back-to-back
launches, after a warm-up of both, at the three facet offsets of the 3 x 3 cover.  Prints one JSON line per kernel (k1, b8):
per offset and over all offsets the median, minimum, maximum and spread (max - min) of the per-facet time of each form in
ms, the ratio of the medians, the verdict by the rule of DESIGN.md section 6 (a difference counts only beyond BOTH forms'
spread) and the relative RMS difference of the two outputs (they round differently).

Usage: python tools/time_half_length_64k.py [--which k1 b8] [--rows 4096] [--band START LENGTH] [--repeats 7] [--calls 3] [--out FILE]"""
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

W, N, XM, YN, YB = 10.875, 131072, 1024, 65536, 45056
FORMS = ("real", "half_length")


def stats(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), spread=max(ms) - min(ms), repeats=len(ms))


def verdict(st):
    """half-length against real: 'faster' / 'slower' when the medians differ by more than both spreads, else 'same'"""
    diff = st["half_length"]["median"] - st["real"]["median"]
    if abs(diff) <= max(st["half_length"]["spread"], st["real"]["spread"]):
        return "same"
    return "faster" if diff < 0 else "slower"


def measure(args, cover, call, outs):
    """the interleaved repeats of ``call(form, facet config)`` at every offset of the cover"""
    scale = YB / args.rows

    def timed(name, cfg):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            call(name, cfg)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.calls * scale

    per_offset, every, rel = {}, {name: [] for name in FORMS}, 0.0
    for cfg in cover:
        for name in FORMS:  # warm-up of both forms at this offset: code objects, window tables, masks, clocks
            timed(name, cfg)
        a, b = outs["half_length"], outs["real"]
        diff = (a - b).abs().double().square().mean().sqrt() / b.abs().double().square().mean().sqrt()
        rel = max(rel, float(diff))
        ms = {name: [] for name in FORMS}
        for _ in range(args.repeats):
            for name in FORMS:
                ms[name].append(timed(name, cfg))
        per_offset[str(cfg.off1)] = {name: stats(v) for name, v in ms.items()}
        per_offset[str(cfg.off1)]["half_length_against_real"] = verdict(per_offset[str(cfg.off1)])
        for name, v in ms.items():
            every[name].extend(v)
    total = {name: stats(v) for name, v in every.items()}
    return dict(per_offset=per_offset, all_offsets=total, half_length_relative_rms_difference_from_real=rel,
                half_length_over_real_median=total["half_length"]["median"] / total["real"]["median"],
                half_length_against_real=verdict(total))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n", maxsplit=1)[0])
    ap.add_argument("--which", nargs="+", default=["k1", "b8"], choices=["k1", "b8"])
    ap.add_argument("--rows", type=int, default=4096, help="rows of the block every call transforms")
    ap.add_argument("--band", type=int, nargs=2, default=(0, YN), metavar=("START", "LENGTH"), help="default: the whole axis")
    ap.add_argument("--repeats", type=int, default=7, help="event pairs per form and offset (at least 5)")
    ap.add_argument("--calls", type=int, default=3, help="launches inside one event pair")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    if not 0 < args.rows <= YB:
        ap.error(f"--rows must be in [1, {YB}]")
    band = tuple(args.band)
    core = sw.SwiftlyCoreHip(W, N, XM, YN)
    if not (core.supports_real_facets_rfft() and core.supports_real_facets_out_c2r()):
        raise SystemExit("no half-length forms for this configuration: " + sw._lib.last_error())  # pylint: disable=protected-access
    cover = [c for c in make_full_cover_config(N, YB, sw.FacetConfig) if c.off0 == 0]  # one row of the cover: off1, mask1
    gen = torch.Generator(device="cuda").manual_seed(9)
    common = dict(device=torch.cuda.get_device_name(0), build=sw._lib.build_info(),  # pylint: disable=protected-access
                  swiftly_hip_build_id=sw._lib.load().swiftly_hip_build_id().decode(),  # pylint: disable=protected-access
                  shape=dict(facet=[YB, YB], row_block=[args.rows, YB], yN=YN, band=list(band), offsets=[c.off1 for c in cover],
                             calls_per_repeat=args.calls),
                  unit="ms per facet (row block time x facet rows / block rows)")
    lines = []
    if "k1" in args.which:
        rows = torch.randn((args.rows, YB), device="cuda", dtype=torch.float32, generator=gen)
        outs = {name: torch.zeros((args.rows, core.band_columns(band)), dtype=torch.complex64, device="cuda") for name in FORMS}

        def k1(name, cfg):
            core.prepare_facet_band(rows, cfg.off1, band, out=outs[name], rows_of=(YB, 0), half_length=name == "half_length")

        res = dict(tool="time_half_length_64k", kernel="k1", **common, **measure(args, cover, k1, outs))
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        del rows, outs
    if "b8" in args.which:
        acc = torch.randn((args.rows, band[1]), device="cuda", dtype=torch.complex64, generator=gen)
        outs = {name: torch.zeros((args.rows, YB), dtype=torch.float32, device="cuda") for name in FORMS}

        def b8(name, cfg):
            core.finish_facet_band(acc, band, cfg.off1, YB, mask=cfg.mask1, out=outs[name], real=True,
                                   half_length=name == "half_length")

        res = dict(tool="time_half_length_64k", kernel="b8", **common, **measure(args, cover, b8, outs))
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as fh:
            fh.write("\n".join(lines) + "\n")
    for line in lines:
        rel = json.loads(line)["half_length_relative_rms_difference_from_real"]
        if not rel < 1e-5:
            raise SystemExit(f"the half-length form is {rel:.2e} away from the real form")


if __name__ == "__main__":
    main()
