"""
The in-process forward paths that own both K3 and the finish of a wave -- ``SwiftlyForward.get_wave`` on K2 slabs and on the
wave's own ``Q``, its staged twin and ``_finish_from_columns`` on the row-window layout -- switch to the grouped subgrid side
(swiftly_hip_wave_group_finish_pieces) TOGETHER: in any request order, with the prefetch on and off, they give identical
bits.  With the switch off (``swiftly_hip_group_finish(0)``, SWIFTLY_GROUP_FINISH=0) they give the bits of the paths that
never switch, K3 + wave_subgrid_side as ``wave_blocks`` / ``finish_from_blocks`` run them.

The small problem of test_hip_k2_slabs_gpu.py: yN = 32768, m = 512, xM = 1024, three facets of 352 rows in two off1 groups,
a plan of eight subgrid columns whose windows share slabs, wrap around the cyclic axis and put piece boundaries at 272, 320
and 368 columns.
"""
import numpy
import pytest

import bench
from oracle import separable as sep
from oracle import swiftly_oracle as orc

pytestmark = pytest.mark.gpu

W64, N64, xM64, yN64, yB, xA, M = 10.875, 65536, 1024, 32768, 352, 928, 512
SEED = 141
PLAN = {0: (0, 2), 1: (0, 2), 3: (0, 2, 69), 4: (0, 2), 5: (0,), 9: (0, 2, 69), 32: (0, 2), 70: (0, 2, 69)}  # i1: i0s
ORDERS = {"ascending": (0, 1, 2, 3, 4, 5, 6, 7), "descending": (7, 6, 5, 4, 3, 2, 1, 0), "shuffled": (5, 3, 2, 7, 0, 6, 4, 1)}
_cache = {}


def relrms(a, b):
    return float(numpy.sqrt(numpy.mean(numpy.abs(a - b) ** 2) / numpy.mean(numpy.abs(b) ** 2)))


def problem():
    if "p" not in _cache:
        import torch

        import ska_sdp_exec_swiftly_amd as sw

        cfg = sw.SwiftlyConfig(backend="hip", W=W64, fov=1.0, N=N64, yB_size=yB, yN_size=yN64, xA_size=xA, xM_size=xM64)
        if not cfg.core.supports_group_finish(torch.complex64, 3):
            pytest.fail("the grouped subgrid side must exist for (m, xM) = (512, 1024)")
        fstep = cfg.facet_off_step
        facet_cfgs = [sw.FacetConfig(o0, o1, yB) for o0, o1 in ((0, 0), (0, 50 * fstep), (-70 * fstep, 0))]
        vectors = [sep.facet_vectors(SEED + j, yB, rank=2) for j in range(len(facet_cfgs))]
        facets = [bench.separable_facet(torch, vectors[j], c) for j, c in enumerate(facet_cfgs)]
        plan = [sw.SubgridConfig(i0 * xA, i1 * xA, xA) for i1 in sorted(PLAN) for i0 in PLAN[i1]]
        waves = {}
        for c in plan:
            waves.setdefault(c.off1, []).append(c)
        _cache["p"] = (torch, sw, cfg, facet_cfgs, facets, plan, waves, vectors)
    return _cache["p"]


class Knobs:
    """the process-wide switches of one run, restored afterwards"""

    def __init__(self, group_finish, slabs=True, prefetch=True):
        self.want = (group_finish, slabs, prefetch)

    def __enter__(self):
        from ska_sdp_exec_swiftly_amd import _lib

        sw = problem()[1]
        self.old = (_lib.load().swiftly_hip_group_finish(int(self.want[0])), sw.api._K2_SLABS, sw.api._PREFETCH)
        sw.api._K2_SLABS, sw.api._PREFETCH = self.want[1], self.want[2]

    def __exit__(self, *exc):
        from ska_sdp_exec_swiftly_amd import _lib

        sw = problem()[1]
        _lib.load().swiftly_hip_group_finish(self.old[0])
        sw.api._K2_SLABS, sw.api._PREFETCH = self.old[1], self.old[2]


def forward():
    torch, sw, cfg, facet_cfgs, facets, plan, waves, _ = problem()
    return sw.SwiftlyForward(cfg, list(zip(facet_cfgs, facets)), subgrid_configs=plan, wave_axis=1)


def counted(core):
    """count the calls of the grouped subgrid side on this core"""
    calls = []
    inner = core.wave_group_finish_pieces

    def wrapper(*a, **k):
        calls.append(1)
        return inner(*a, **k)

    core.wave_group_finish_pieces = wrapper
    return calls, lambda: core.__dict__.pop("wave_group_finish_pieces", None)


def reference_on():
    """every planned wave through get_wave on slabs in ascending order, switch on (once)"""
    if "on" not in _cache:
        torch, sw, cfg, _, _, _, waves, _ = problem()
        calls, undo = counted(cfg.core)
        try:
            with Knobs(True):
                fwd = forward()
                _cache["on"] = {k: fwd.get_wave(waves[k]).cpu().numpy() for k in sorted(waves)}
        finally:
            undo()
        assert len(calls) == len(waves)  # the grouped side really ran, once per wave
    return _cache["on"]


def reference_off():
    """the same with the switch off (once)"""
    if "off" not in _cache:
        torch, sw, cfg, _, _, _, waves, _ = problem()
        calls, undo = counted(cfg.core)
        try:
            with Knobs(False):
                fwd = forward()
                _cache["off"] = {k: fwd.get_wave(waves[k]).cpu().numpy() for k in sorted(waves)}
        finally:
            undo()
        assert not calls
    return _cache["off"]


@pytest.mark.parametrize("prefetch", [False, True])
@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("slabs", [False, True])
def test_switched_paths_agree_bit_for_bit(slabs, order, prefetch):
    waves = problem()[6]
    want = reference_on()
    keys = [sorted(waves)[i] for i in ORDERS[order]]
    with Knobs(True, slabs, prefetch):
        fwd = forward()
        for k in keys:
            assert numpy.array_equal(fwd.get_wave(waves[k]).cpu().numpy(), want[k]), (slabs, order, prefetch, k)
        assert (fwd.prefetch_issued > 0) == prefetch
        assert bool(fwd.lru._items) != slabs  # per-wave Q without slabs, none with them


def test_staged_twin_and_finish_from_columns_agree_bit_for_bit():
    torch, sw, cfg, facet_cfgs, _, _, waves, _ = problem()
    want = reference_on()
    with Knobs(True):
        fwd = forward()
        for k in (sorted(waves)[2], sorted(waves)[7]):  # i1 = 3 (pieces split at 368) and 70 (the wrap)
            sgs = waves[k]
            assert numpy.array_equal(fwd._wave_b_staged(sgs).cpu().numpy(), want[k])
            Q, rowmap = fwd._get_wave_columns(k)
            got = sw.api._finish_from_columns(cfg.core, Q, 1, facet_cfgs, sgs, [sg.off0 for sg in sgs], rowmap=rowmap)
            assert numpy.array_equal(got.cpu().numpy(), want[k])
            # a request for part of the wave: the same subgrids
            one = fwd.get_wave(sgs[1:2]).cpu().numpy()
            assert numpy.array_equal(one[0], want[k][1])


def test_switch_off_gives_the_unswitched_paths_bits():
    """switch off: get_wave equals K3 + wave_subgrid_side as wave_blocks / finish_from_blocks run them -- the paths that hand
    G[F, S, m, m] to someone else and never switch; they give the same bits whatever the switch says"""
    torch, sw, cfg, facet_cfgs, _, _, waves, _ = problem()
    off = reference_off()
    for on in (False, True):
        with Knobs(on):
            fwd = forward()
            for k in (sorted(waves)[2], sorted(waves)[7]):
                got = sw.api.finish_from_blocks(cfg.core, fwd.wave_blocks(waves[k]), facet_cfgs, waves[k])
                assert numpy.array_equal(got.cpu().numpy(), off[k]), (on, k)


def test_switched_and_unswitched_results_agree_within_float32_rounding():
    """the two orders re-associate the facet sums: not the same bits, the same subgrids.  Bound: both chains sit within
    2e-5 of the oracle end to end; against each other the CPU model of the two float32 chains gives
    1.7e-6 on the probe configuration (tests/test_group_finish_model_cpu.py: 'the two float32 chains against each other'),
    a quarter of either chain's own error -- allowed here: a quarter of the 2e-5 end-to-end bound."""
    torch, sw, cfg, facet_cfgs, _, _, waves, vectors = problem()
    on, off = reference_on(), reference_off()
    worst = max(relrms(on[k], off[k]) for k in on)
    differ = any(not numpy.array_equal(on[k], off[k]) for k in on)
    so = sep.SeparableOracle(orc.OracleCore(W64, N64, xM64, yN64), [orc.CoverItem(c.off0, c.off1, c.size) for c in facet_cfgs],
                             vectors)
    k = sorted(waves)[7]
    c = waves[k][2]
    w = so.subgrid(orc.CoverItem(c.off0, c.off1, c.size))
    e_on, e_off = relrms(on[k][2], w), relrms(off[k][2], w)
    print(f"switched vs unswitched: worst wave {worst:.3e}; subgrid (69, 70) vs oracle: switched {e_on:.3e}, unswitched {e_off:.3e}")
    assert differ and worst < 5e-6
    assert e_on < 2e-5 and e_off < 2e-5
