"""
The forward subgrid side with the strided axis finished first (include/swiftly_hip.h: swiftly_hip_wave_group_finish_pieces;
csrc/swiftly_groupfinish.h) against the oracle: the column kernel group_finish alone, the row kernel over its output alone,
and both end to end, at both instances -- (m, xM) = (128, 256), the smallest pair of the capability table, and (512, 1024),
the pair of the benchmarked workload.

Per instance: S = 2 subgrids whose crops wrap on the padded axis, four facets in two off1 groups -- one facet alone, three
whose placement bands along axis 0 overlap and wrap -- both masks, and the wave's K2 window ``Q`` fed as one piece and as two
pieces with different row maps.  The split (48, 272 columns) is a multiple of 16, as the entry point demands, and no
multiple of 32: it lies inside a column tile of the parent's K3 and on a tile boundary of group_finish, whose 16-column
tiles never straddle a piece boundary.  Columns a piece does not hold are NaN in its buffer.

The reference operations are the oracle's extract_from_facet (the window), add_to_subgrid along axis 0, the sum over a
group, finish_subgrid per axis and the masks.  Tolerance: the parent's three-kernel side (K3, sum_finish_facets,
finish_subgrid along axis 0) runs on the same inputs against the same oracle, and the new side is allowed that error plus
the error of the CPU model of the new order in float32 arithmetic (tests/group_finish_model.py) on the same inputs: the
two orders round different intermediates, and the model's distance from the oracle is an independent measure of how much
float32 rounding of these stages amounts to.  Measured figures: profiles/r14_group_finish_accuracy.txt.
"""
import numpy
import pytest

import group_finish_model as gm
from oracle import swiftly_oracle as orc

pytestmark = pytest.mark.gpu

CASES = {
    "128-256": dict(W=11.0, N=1024, yN=512, xA=192, xM=256, split=48, sub=[(96, -33), (-17, 96)],
                    facets=[(0, 88), (0, 0), (40, 0), (100, 0)], extra_row_sub=150),
    "512-1024": dict(W=10.875, N=65536, yN=32768, xA=928, xM=1024, split=272, sub=[(3 * 464, 5 * 464), (-7 * 464, 0)],
                     facets=[(0, 352), (0, 0), (200, 0), (400, 0)], extra_row_sub=11 * 464),
}
_cache = {}


def relrms(a, b):
    return float(numpy.sqrt(numpy.mean(numpy.abs(a - b) ** 2) / numpy.mean(numpy.abs(b) ** 2)))


def problem(name):
    """Inputs, oracle results and the parent's results of one instance, computed once and shared (never modified)."""
    if name in _cache:
        return _cache[name]
    import torch

    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    P = CASES[name]
    core = SwiftlyCoreHip(P["W"], P["N"], P["xM"], P["yN"])
    ref = orc.OracleCore(P["W"], P["N"], P["xM"], P["yN"])
    m, xM, xA, yN = core.xM_yN_size, P["xM"], P["xA"], P["yN"]
    assert core.supports_group_finish(torch.complex64, 4)
    fstep, sstep = core.facet_off_step, core.subgrid_off_step
    f_offs = [(a * fstep, b * fstep) for a, b in P["facets"]]  # list order: the single facet's group sorts LAST (larger off1)
    subs = [(a * sstep, b * sstep) for a, b in P["sub"]]
    F, S = len(f_offs), len(subs)
    rng = numpy.random.default_rng(41)
    # piece A keeps exactly the rows the subgrids read, piece B those of one more subgrid column: two different row maps
    map_a, rows_a = core.subgrid_column_rows([s[0] for s in subs])
    map_b, rows_b = core.subgrid_column_rows([s[0] for s in subs] + [P["extra_row_sub"] * sstep])
    rm_a, rm_b = map_a.cpu().numpy(), map_b.cpu().numpy()
    assert rows_b > rows_a and (rm_b[rm_a >= 0] >= 0).all()
    q_b = (rng.standard_normal((F, rows_b, m)) + 1j * rng.standard_normal((F, rows_b, m))).astype(numpy.complex64)
    q_a = numpy.zeros((F, rows_a, m), dtype=numpy.complex64)
    keep = rm_a >= 0
    q_a[:, rm_a[keep]] = q_b[:, rm_b[keep]]
    # the windows through the oracle, one facet's padded axis at a time
    wins = numpy.empty((F, S, m, m), dtype=numpy.complex64)
    for f in range(F):
        full = numpy.zeros((yN, m), dtype=numpy.complex64)
        full[rm_b >= 0] = q_b[f][rm_b[rm_b >= 0]]
        for b in range(S):
            wins[f, b] = ref.extract_from_facet(full, subs[b][0], axis=0)
    mask0 = (rng.random((S, xA)) > 0.2).astype(numpy.float32)
    mask1 = (rng.random((S, xA)) > 0.2).astype(numpy.float32)
    groups = sorted({o[1] for o in f_offs})
    i = numpy.arange(xA)
    T_want = numpy.empty((len(groups), S, xA, m), dtype=complex)
    want = numpy.empty((S, xA, xA), dtype=complex)
    for b in range(S):
        total = numpy.zeros((xM, xM), dtype=complex)
        for g, g1 in enumerate(groups):
            acc = numpy.zeros((xM, m), dtype=complex)
            for f, (o0, o1) in enumerate(f_offs):
                if o1 == g1:
                    acc += ref.add_to_subgrid(wins[f, b].astype(complex), o0, axis=0)
            total += ref.add_to_subgrid(acc, g1, axis=1)
            cols = numpy.array([ref.finish_subgrid(acc[:, j], subs[b][0], xA) for j in range(m)]).T
            T_want[g, b] = cols * mask0[b][:, None]
        want[b] = ref.finish_subgrid(total, [subs[b][0], subs[b][1]], xA) * mask0[b][:, None] * mask1[b][None, :]
    # the row step on its own: from the oracle's T (complex64), per subgrid
    T_in = T_want.astype(numpy.complex64)
    want2 = numpy.empty((S, xA, xA), dtype=complex)
    for b in range(S):
        acc = numpy.zeros((xA, xM), dtype=complex)
        for g, g1 in enumerate(groups):
            acc += ref.add_to_subgrid(T_in[g, b].astype(complex), g1, axis=1)
        want2[b] = numpy.array([ref.finish_subgrid(acc[a], subs[b][1], xA) for a in range(xA)]) * mask1[b][None, :]
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    d = dict(core=core, ref=ref, f_offs=f_offs, subs=subs, groups=groups, m=m, xM=xM, xA=xA, split=P["split"],
             q_a=dev(q_a), q_b=dev(q_b), map_a=map_a, map_b=map_b, rows_a=rows_a, rows_b=rows_b, wins=wins,
             mask0=dev(mask0), mask1=dev(mask1), mask0_h=mask0, mask1_h=mask1, T_want=T_want, want=want, T_in=T_in, want2=want2)
    # the parent's three-kernel side on the same inputs, and the float32 CPU model of the new order
    G = torch.empty((F, S, m, m), dtype=torch.complex64, device="cuda")
    core.transform_contributions_pieces(pieces(d, 1), [o[0] for o in f_offs], [s[0] for s in subs], G)
    tmp = torch.empty((S, xM, xA), dtype=torch.complex64, device="cuda")
    res = torch.empty((S, xA, xA), dtype=torch.complex64, device="cuda")
    core.wave_subgrid_side(G, [o[0] for o in f_offs], [o[1] for o in f_offs], [s[0] for s in subs], [s[1] for s in subs],
                           xA, d["mask0"], d["mask1"], tmp, res)
    d["parent"] = res.cpu().numpy()
    d["err_parent"] = relrms(d["parent"], want)
    model = [gm.subgrid_side(ref, wins[:, b], f_offs, subs[b], xA, 32, mask0[b], mask1[b]) for b in range(S)]
    d["err_model"] = relrms(numpy.array([mo[1] for mo in model]), want)
    d["err_model_T"] = relrms(numpy.array([[mo[0][g] for mo in model] for g in range(len(groups))]), T_want)
    d["bound"] = d["err_parent"] + d["err_model"]
    print(f"{name}: parent three-kernel side vs oracle {d['err_parent']:.3e}, float32 model of the new order "
          f"{d['err_model']:.3e} (T: {d['err_model_T']:.3e}), bound {d['bound']:.3e}")
    _cache[name] = d
    return d


def pieces(d, n):
    """the wave's Q as one piece (the exact rows) or as two: B = [0, split) with the wider row map, A = the rest"""
    import torch

    m = d["m"]
    if n == 1:
        return [(d["q_a"], d["map_a"], d["rows_a"], 0, m)]
    split = d["split"]
    qa, qb = d["q_a"].clone(), d["q_b"].clone()
    qa[:, :, :split] = complex(float("nan"), float("nan"))
    qb[:, :, split:] = complex(float("nan"), float("nan"))
    assert torch.isnan(qa.real).any() and torch.isnan(qb.real).any()
    return [(qa, d["map_a"], d["rows_a"], split, m - split), (qb, d["map_b"], d["rows_b"], 0, split)]


def run(d, n_pieces, stages, t_work=None):
    import torch

    core, xA = d["core"], d["xA"]
    S = len(d["subs"])
    out = torch.empty((S, xA, xA), dtype=torch.complex64, device="cuda") if stages & 2 else None
    f_offs, subs = d["f_offs"], d["subs"]
    return core.wave_group_finish_pieces(pieces(d, n_pieces), [o[0] for o in f_offs], [o[1] for o in f_offs],
                                         [s[0] for s in subs], [s[1] for s in subs], xA, d["mask0"], d["mask1"], out,
                                         t_work=t_work, stages=stages)


@pytest.mark.parametrize("n_pieces", [1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_group_finish_column_kernel(name, n_pieces):
    """stage 1 alone: T[g][b] = mask0 * finish_subgrid_axis0(sum over the group of add_to_subgrid_axis0(window))"""
    d = problem(name)
    T = run(d, n_pieces, 1)
    got = T[:, :, : d["xA"]].cpu().numpy()
    assert got.shape == d["T_want"].shape and numpy.isfinite(got.view(numpy.float32)).all()
    err = relrms(got, d["T_want"])
    worst = max(relrms(got[g, b], d["T_want"][g, b]) for g in range(got.shape[0]) for b in range(got.shape[1]))
    print(f"{name}, {n_pieces} piece(s): group_finish vs oracle {err:.3e} (worst group / subgrid {worst:.3e}), "
          f"bound {d['bound']:.3e}")
    assert err <= d["bound"] and worst <= 1.5 * d["bound"], (err, worst, d["bound"])
    # the masked rows are exact zeros
    for b in range(got.shape[1]):
        assert not got[:, b, d["mask0_h"][b] == 0].any()


@pytest.mark.parametrize("name", list(CASES))
def test_row_kernel_over_groups(name):
    """stage 2 alone, on the oracle's T: out[b] = mask1 * finish_subgrid_axis1(sum over the groups of add_to_subgrid_axis1(T))"""
    import torch

    d = problem(name)
    G, S = len(d["groups"]), len(d["subs"])
    t_work = torch.full((G, S, d["xM"], d["m"]), float("nan"), dtype=torch.complex64, device="cuda")  # rows >= xA: never read
    t_work[:, :, : d["xA"]] = torch.from_numpy(d["T_in"]).cuda()
    got = run(d, 1, 2, t_work=t_work.view(-1)).cpu().numpy()
    err = relrms(got, d["want2"])
    print(f"{name}: row kernel over groups vs oracle {err:.3e}, bound {d['bound']:.3e}")
    assert numpy.isfinite(got.view(numpy.float32)).all()
    assert err <= d["bound"], (err, d["bound"])


@pytest.mark.parametrize("n_pieces", [1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_both_kernels_end_to_end(name, n_pieces):
    d = problem(name)
    got = run(d, n_pieces, 3).cpu().numpy()
    err = relrms(got, d["want"])
    worst = max(relrms(got[b], d["want"][b]) for b in range(got.shape[0]))
    print(f"{name}, {n_pieces} piece(s): new side vs oracle {err:.3e} (worst subgrid {worst:.3e}); parent "
          f"{d['err_parent']:.3e}; bound {d['bound']:.3e}; new vs parent {relrms(got, d['parent']):.3e}")
    assert err <= d["bound"] and worst <= 1.5 * d["bound"], (err, worst, d["bound"])
    if n_pieces == 2:  # every column is computed from its own piece with the same arithmetic: the split changes no bit
        assert numpy.array_equal(got, run(d, 1, 3).cpu().numpy())


def test_refusals():
    """the gate answers for the sizes; the entry point refuses float64 column arithmetic and a bad stage mask"""
    import torch

    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip, _lib

    d = problem("128-256")
    core = d["core"]
    assert not core.supports_group_finish(torch.complex128, 4)
    assert not core.supports_group_finish(torch.complex64, 33)  # 33 x (xM / m = 2) row-kernel entries > 64
    assert not SwiftlyCoreHip(11.0, 2048, 512, 512).supports_group_finish(torch.complex64, 4)  # (128, 512): no instance
    with pytest.raises(ValueError, match="stages"):
        run(d, 1, 4)
    other = SwiftlyCoreHip(11.0, 1024, 256, 512, column_precision=64)
    assert not other.supports_group_finish(torch.complex64, 4)
    with pytest.raises(NotImplementedError, match="float32 column arithmetic"):
        run(dict(d, core=other), 1, 3)
    assert _lib.load().swiftly_hip_group_finish(-1) in (0, 1)
