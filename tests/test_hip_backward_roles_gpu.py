"""
The roles of the backward pass on the GPU, on the small seeded problem of ``tests/test_hip_band_pipeline_gpu.py``: the two
accumulate entry points of ``SwiftlyBackward`` run one fold (bit-equal facets in both schedules), and the workspace promises of
``SubgridSplitter`` that ``DistributedBackward.MAX_IN_FLIGHT`` rests on -- a result of the fused route stays untouched by the
next call, and two splitters of one ``DistributedBackward`` share no workspace.
"""
import pytest

from test_hip_band_pipeline_gpu import _small_rows_problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def problem():
    torch, sw, cfg, facet_cfgs, _, sg_cfgs = _small_rows_problem()
    gen = torch.Generator(device="cuda").manual_seed(77)
    xA = sg_cfgs[0].size
    data = [torch.randn((xA, xA), dtype=torch.complex64, device="cuda", generator=gen) for _ in sg_cfgs]
    return torch, sw, cfg, facet_cfgs, sg_cfgs, data


def waves_of(sg_cfgs, axis):
    """``{wave key: indices of its subgrids}`` in the schedule ``axis``"""
    waves = {}
    for i, c in enumerate(sg_cfgs):
        waves.setdefault(int(c.off1 if axis == 1 else c.off0), []).append(i)
    return waves


@pytest.mark.parametrize("axis", [0, 1])
def test_accumulate_wave_is_the_one_chunk_case_of_accumulate_chunks(problem, axis):
    torch, sw, cfg, facet_cfgs, sg_cfgs, data = problem
    one, two = (sw.SwiftlyBackward(cfg, facet_cfgs, wave_axis=axis, subgrid_configs=sg_cfgs) for _ in range(2))
    for key, idx in waves_of(sg_cfgs, axis).items():
        sgs = [sg_cfgs[i] for i in idx]
        parts = one.wave_contributions(sgs, [data[i] for i in idx])
        one.accumulate_wave(sgs, parts)
        two.accumulate_chunks(key, [(sgs, parts)])
    assert one.wave_axis == two.wave_axis == axis and two.dtype == torch.complex64
    got, want = two.finish(), one.finish()
    assert len(got) == len(want) == len(facet_cfgs)
    for a, b in zip(got, want):
        assert float(b.abs().max()) > 0 and torch.equal(a, b)


def test_a_fused_split_stays_valid_over_the_next_call(problem):
    torch, sw, cfg, facet_cfgs, sg_cfgs, data = problem
    assert cfg.core.supports_fused_subgrid(torch.complex64, n_facets=len(facet_cfgs))
    bwd = sw.SwiftlyBackward(cfg, facet_cfgs, wave_axis=1, subgrid_configs=sg_cfgs)
    results, kept = [], []
    for idx in list(waves_of(sg_cfgs, 1).values())[:3]:
        results.append(bwd.wave_contributions([sg_cfgs[i] for i in idx], [data[i] for i in idx]))
        kept.append(results[-1].clone())
        assert "work" in bwd.splitter._wsbuf  # the fused route
        if len(results) > 1:  # call k is unchanged after call k + 1
            assert results[-2].data_ptr() != results[-1].data_ptr() and torch.equal(results[-2], kept[-2])
    assert float(kept[0].abs().max()) > 0 and not torch.equal(kept[0], kept[2])
    assert results[2].data_ptr() == results[0].data_ptr()  # ... and gives its place to call k + 2: two slots, no more


def test_splitters_of_one_distributed_backward_share_no_workspace(problem):
    torch, _, cfg, facet_cfgs, sg_cfgs, data = problem
    from ska_sdp_exec_swiftly_amd.distributed import DistributedBackward
    from ska_sdp_exec_swiftly_amd.splitter import SubgridSplitter

    # three facets on two ranks: facet 2 is cooperative, so the arrival order depends on the rank that owns the wave
    dist = DistributedBackward(cfg, facet_cfgs, wave_axis=1, subgrid_configs=sg_cfgs, dtype=torch.complex64, rank_world=(0, 2))
    owners, sends = set(), []
    for key, idx in waves_of(sg_cfgs, 1).items():
        sgs = [sg_cfgs[i] for i in idx]
        send, _, _ = dist.pack_wave(sgs, [data[idx[k]] for k in dist.subgrids_of(sgs)])
        sends.append(send)
        owners.add(dist.sharding.key_owner[key])
    assert owners == {0, 1}
    used = [s for s in dist._splitters.values() if s._wsbuf]
    assert len(used) == 2 and all(type(s) is SubgridSplitter and s.dtype == torch.complex64 for s in dist._splitters.values())
    spans = []
    for s in used:
        assert {"work", "parts0", "parts1"} <= set(s._wsbuf)
        spans += [(buf.data_ptr(), buf.data_ptr() + buf.numel() * buf.element_size()) for buf in s._wsbuf.values()]
    spans.sort()
    assert all(end <= start for (_, end), (start, _) in zip(spans, spans[1:]))  # disjoint, not only distinct
    # every send buffer is a view of a ``parts`` slot of the splitter that made it
    assert all(any(lo <= s.data_ptr() < hi for lo, hi in spans) for s in sends if s.numel())
