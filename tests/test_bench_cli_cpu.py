"""bench.py's command line and the --dump-outputs sample, without a GPU."""
import os
import subprocess
import sys
import types

import numpy

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_options_exist():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], stdout=subprocess.PIPE, text=True,
                         timeout=120, check=True).stdout
    assert "--full" in out and "--dump-outputs" in out


def test_zero_steps_refused():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=120, check=False)
    assert res.returncode == 2 and "--steps" in res.stderr


def test_dump_sample_is_fixed_and_fits():
    for name, wl in bench.WORKLOADS.items():
        xA = wl["params"]["xA_size"]
        for n in (1, 25, 505, 20164):
            idx = bench.dump_sample(n, xA)
            assert idx == bench.dump_sample(n, xA), name
            assert len(idx) == len(set(idx)) >= 1 and 0 <= min(idx) and max(idx) < n
            assert len(idx) == 1 or len(idx) * xA * xA * 8 <= bench.DUMP_BYTES


def test_write_outputs(tmp_path):
    cfgs = [types.SimpleNamespace(off0=3 * i, off1=-i) for i in range(6)]
    rng = numpy.random.default_rng(5)
    data = {i: (rng.standard_normal((16, 16)) + 1j * rng.standard_normal((16, 16))).astype(numpy.complex64) for i in (4, 1)}
    bench.write_outputs(str(tmp_path), cfgs, data)
    sg = numpy.load(tmp_path / "subgrids.npy")
    off = numpy.load(tmp_path / "subgrid_offsets.npy")
    assert sg.dtype == numpy.float32 and sg.shape == (2, 16, 16, 2)
    assert off.dtype == numpy.float64 and off.tolist() == [[3, -1], [12, -4]]
    assert numpy.array_equal(sg[1, ..., 0] + 1j * sg[1, ..., 1], data[4])
