"""
bench.py as it is run for every change: a plain run (set-up, warm-up, the timed steps, one JSON line -- nothing of
`--full`) with `--dump-outputs`, whose files must hold the subgrids the timed objects computed (checked against the
separable oracle) in float32 within the size budget.
"""
import json
import os
import subprocess
import sys

import numpy
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_step(tmp_path):
    import bench
    import ska_sdp_exec_swiftly_amd as sw
    from oracle import separable as sep

    out_dir = tmp_path / "outputs"
    res = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "8k", "--steps", "2", "--warmup", "1",
         "--dump-outputs", str(out_dir)],
        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, check=False,
    )
    assert res.returncode == 0, res.stderr[-3000:]
    line = json.loads(res.stdout.strip().splitlines()[-1])
    assert line["metric"] == "facet_to_subgrid_contributions_per_s" and line["unit"] == "contributions/s"
    assert line["higher_is_better"] is True and line["steps"] == 2 and len(line["step_ms_each"]) == 2
    assert line["ms_per_step"] > 0 and line["value"] > 0
    for key in ("parity", "backward", "roundtrip", "roofline", "accurate", "high_precision"):
        assert line[key] is None, key  # measured with --full only
    assert "cpu_baseline" not in line and "other_workloads" not in line

    names = sorted(os.listdir(out_dir))
    assert names == ["subgrid_offsets.npy", "subgrids.npy"]
    subgrids = numpy.load(out_dir / "subgrids.npy")
    offsets = numpy.load(out_dir / "subgrid_offsets.npy")
    assert subgrids.dtype == numpy.float32 and offsets.dtype == numpy.float64
    assert sum(os.path.getsize(out_dir / n) for n in names) <= 64e6

    wl = bench.WORKLOADS["8k"]
    p = wl["params"]
    cfg = sw.SwiftlyConfig(backend="hip", **p)
    facet_cfgs = sw.make_full_facet_cover(cfg)
    sg_cfgs = bench.select_subgrids(sw.make_full_subgrid_cover(cfg), p["N"], p["xA_size"], wl["sparse_radius"])
    idx = bench.dump_sample(len(sg_cfgs), p["xA_size"])
    assert subgrids.shape == (len(idx), p["xA_size"], p["xA_size"], 2)
    assert offsets.tolist() == [[sg_cfgs[i].off0, sg_cfgs[i].off1] for i in idx]
    vectors = [sep.facet_vectors(1234 + j, p["yB_size"], rank=2) for j in range(len(facet_cfgs))]
    got = {i: subgrids[k, ..., 0] + 1j * subgrids[k, ..., 1] for k, i in enumerate(idx)}
    par = bench.verify_subgrids(p, facet_cfgs, vectors, sg_cfgs, got)
    assert par["ok"], par
