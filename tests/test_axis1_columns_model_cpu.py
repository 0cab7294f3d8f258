"""
The dataflow of ``SwiftlyConfig(axis1_first="k2")`` in the error model (tests/accuracy_model.py, unchanged): the reordered
chain -- contiguous axis finished before the strided-axis transforms -- with the UNEVEN four-step splits the kernel that
finishes the rows inside K2's first pass needs (n1 = 16384 / m rows of the window in LDS: 32 x 1024 at the benchmarked
shape, 64 x 256 at the small one; on the probe configuration's yN = 2048 the corresponding short-by-long splits are
8 x 256 and 2 x 1024).  The split only moves the one complex64 rounding of the scratch, so the all-float32 error has to
stay inside the window tests/test_accuracy_budget_cpu.py pins for the even split (32, 64).
"""
import pytest

import accuracy_model as am

ALL32 = dict(k1=32, k2=32, k3=32, sf=32, k5=32)


@pytest.mark.parametrize("split", [(8, 256), (2, 1024)])
def test_reordered_chain_with_an_uneven_scratch_split_keeps_its_error(split):
    assert split[0] * split[1] == am.PROBE["yN"]
    err = am.chain_error(ALL32, split=split, chain=am.forward_chain_reordered)
    print(f"reordered chain, float32 everywhere, split {split}: {err:.3e}")
    assert 1.5e-6 < err < 3e-6, (split, err)  # (8, 256): 2.056e-6, (2, 1024): 2.057e-6; (32, 64): 2.074e-6
