"""
The forward subgrid side with the strided axis finished first per facet off1 group (csrc/swiftly_groupfinish.h), on the CPU
model first (tests/group_finish_model.py): the new order re-associates the facet sums, so its subgrids are not the parent's
bit for bit -- these tests pin what the difference is allowed to be before any kernel runs.

* End to end on the probe configuration of tests/accuracy_model.py the all-float32 error stays in the band the parent's
  order is pinned to (test_accuracy_budget_cpu.py: 1.0e-5 .. 1.6e-5): K2 and the m-point transform behind it, which work on
  data amplified by both facet windows, are the same arithmetic in both orders; what follows Fn is harmless in either.
* With float64 arithmetic the new order sits at or below the parent's storage floor: it stores one complex64
  intermediate fewer (G and the half-finished subgrid become T).
* The subgrid side alone, on un-amplified random windows, agrees with the oracle to a few float32 roundings per
  transform stage in float32 and to the two complex64 stores in float64.
"""
import numpy

import accuracy_model as am
import group_finish_model as gm
from oracle import swiftly_oracle as orc


def _probe_facet(seed=5):
    rng = numpy.random.default_rng(seed)
    yB = am.PROBE["yB"]
    return am._c64(rng.standard_normal((yB, yB)) + 1j * rng.standard_normal((yB, yB)))


def test_new_order_keeps_the_end_to_end_error_budget():
    P, fo, so = am.PROBE, am.PROBE_FO, am.PROBE_SO
    facet = _probe_facet()
    want = am.reference_chain(P, facet, fo, so)
    all32 = dict(k1=32, k2=32, k3=32, sf=32, k5=32)
    all64 = dict(k1=64, k2=64, k3=64, sf=64, k5=64)
    old32 = am.rel_rmse(am.forward_chain(P, facet, fo, so, all32, (32, 64)), want)
    new32 = am.rel_rmse(gm.forward_chain_group_finish(P, facet, fo, so, all32, (32, 64)), want)
    old64 = am.rel_rmse(am.forward_chain(P, facet, fo, so, all64, (32, 64)), want)
    new64 = am.rel_rmse(gm.forward_chain_group_finish(P, facet, fo, so, all64, (32, 64)), want)
    both = am.rel_rmse(gm.forward_chain_group_finish(P, facet, fo, so, all32, (32, 64)),
                       am.forward_chain(P, facet, fo, so, all32, (32, 64)))
    print(f"{old32:.3e}  parent order, float32 arithmetic everywhere")
    print(f"{new32:.3e}  strided axis first, float32 arithmetic everywhere")
    print(f"{old64:.3e}  parent order, storage floor incl. scratch")
    print(f"{new64:.3e}  strided axis first, storage floor incl. scratch")
    print(f"{both:.3e}  the two float32 chains against each other")
    assert 1.0e-5 < new32 < 1.6e-5                # the parent's band (test_accuracy_budget_cpu.py)
    assert abs(new32 - old32) < 0.05 * old32      # the stages that set the error are untouched
    assert new64 <= 1.02 * old64                  # one complex64 store fewer
    # the two orders differ by what the stages behind Fn round: far below either chain's distance from the oracle
    assert both < 0.25 * old32


def test_subgrid_side_model_against_the_oracle():
    """one group of one facet and one of three (overlapping and wrapped placement bands), a crop that wraps, both masks"""
    P = dict(W=11.0, N=1024, yN=512, xA=192, xM=256)
    c = orc.OracleCore(P["W"], P["N"], P["xM"], P["yN"])
    m, xM, xA = c.xM_yN_size, P["xM"], P["xA"]
    fstep, sstep = c.facet_off_step, c.subgrid_off_step
    f_offs = [(0, 88 * fstep), (0, 0), (40 * fstep, 0), (100 * fstep, 0)]
    sub = (96 * sstep, -33 * sstep)
    rng = numpy.random.default_rng(31)
    wins = am._c64(rng.standard_normal((4, m, m)) + 1j * rng.standard_normal((4, m, m)))
    mask0 = (rng.random(xA) > 0.2).astype(float)
    mask1 = (rng.random(xA) > 0.2).astype(float)
    acc = numpy.zeros((xM, xM), dtype=complex)
    for f, (o0, o1) in enumerate(f_offs):
        acc += c.add_to_subgrid(c.add_to_subgrid(wins[f].astype(complex), o0, 0), o1, 1)
    want = c.finish_subgrid(acc, [sub[0], sub[1]], xA) * mask0[:, None] * mask1[None, :]
    T32, out32 = gm.subgrid_side(c, wins, f_offs, sub, xA, 32, mask0, mask1)
    T64, out64 = gm.subgrid_side(c, wins, f_offs, sub, xA, 64, mask0, mask1)
    assert len(T32) == 2 and T32[0].shape == (xA, m) and out32.shape == (xA, xA)
    e32, e64 = am.rel_rmse(out32, want), am.rel_rmse(out64, want)
    print(f"{e32:.3e}  subgrid side, float32 arithmetic;  {e64:.3e}  float64 arithmetic, complex64 stores")
    assert e64 < 1.5e-7      # two complex64 stores: 2^-24 / sqrt(3) = 3.4e-8 relative rms each, summed over two groups
    assert e32 < 1e-6        # four float32 transforms of 128 / 256 points at a few 1e-7 each
    # the row step alone, from the float64 T
    _, out2 = gm.subgrid_side(c, None, f_offs, sub, xA, 32, None, mask1, stage=2, T=T64)
    assert am.rel_rmse(out2, want) < 1e-6
