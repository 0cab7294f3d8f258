"""
GPU parity for transform lengths that are NOT powers of two (171 of the 244 catalogue entries; VERDICT r1 missing #5,
reference tests/test_core.py:82-90 and e.g. swift_configs "1792[1]-n896-448"): every primitive along both axes and
the streaming classes, against the oracle (numpy handles any length).  Lengths Q * 2^k with Q in {3, 5, 7, 9} -- every
non-power-of-two length of the catalogue -- run natively: one radix-Q pass in front of the power-of-two kernels
(csrc/swiftly_mixed.h, r3); any other length, or SWIFTLY_NO_MIXED=1, goes through Bluestein's chirp-z identity
(csrc/swiftly_bluestein.h).  complex128 to rounding, complex64 within the float32 bounds of DESIGN.md section 2.
"""
import numpy
import pytest

from oracle import swiftly_oracle as orc

pytestmark = pytest.mark.gpu

# catalogue entries (ska_sdp_exec_swiftly_amd.swift_configs): all of yN, xM, m non-power-of-two / only yN
CFG_ALL = dict(W=10.875, N=1792, yB_size=608, yN_size=896, xA_size=392, xM_size=448)     # "1792[1]-n896-448": m = 224
CFG_YN = dict(W=11.0, N=1536, yB_size=528, yN_size=768, xA_size=448, xM_size=512)        # "1536[1]-n768-512": m = 256
# all three lengths Q = 5 (640, 320, 160) / Q = 3 (768, 384, 192): the xM = 320 / 384 and m = 160 / 192 of twelve entries
CFG_Q5 = dict(W=11.125, N=1280, yB_size=448, yN_size=640, xA_size=280, xM_size=320)      # "1280[1]-n640-320": m = 160
CFG_Q3 = dict(W=10.75, N=1536, yB_size=512, yN_size=768, xA_size=345, xM_size=384)       # "1536[1]-n768-384": m = 192


def relrms(a, b):
    return float(numpy.sqrt(numpy.mean(numpy.abs(a - b) ** 2) / numpy.mean(numpy.abs(b) ** 2)))


def cores(p):
    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    return (SwiftlyCoreHip(p["W"], p["N"], p["xM_size"], p["yN_size"]),
            orc.OracleCore(p["W"], p["N"], p["xM_size"], p["yN_size"]))


@pytest.mark.parametrize("p", [CFG_ALL, CFG_YN, CFG_Q5, CFG_Q3])
@pytest.mark.parametrize("dtype", [numpy.complex128, numpy.complex64])
@pytest.mark.parametrize("path", ["mixed", "bluestein"])
def test_primitives_nonpow2(p, dtype, path, monkeypatch):
    monkeypatch.setenv("SWIFTLY_NO_MIXED", "1" if path == "bluestein" else "0")
    core, ref = cores(p)
    tol = 1e-11 if dtype == numpy.complex128 else 3e-6
    rng = numpy.random.default_rng(41)
    yB, yN, xA, xM, m = p["yB_size"], p["yN_size"], p["xA_size"], p["xM_size"], ref.xM_yN_size
    fs, ss = core.facet_off_step, core.subgrid_off_step
    rnd = lambda *shape: (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)  # noqa: E731

    def chk(name, x, *args, exact=False):
        got = getattr(core, name)(x, *args)
        want = getattr(ref, name)(x.astype(complex), *args)
        assert got.dtype == dtype and got.shape == want.shape, (name, got.shape, want.shape)
        if exact:
            assert numpy.array_equal(got, want.astype(dtype)), name
        else:
            assert relrms(got, want) < tol, (name, args, relrms(got, want))
        return want.astype(dtype)

    facet = rnd(yB, 37)
    bf = chk("prepare_facet", facet, 5 * fs, 0)                       # strided axis
    chk("prepare_facet", rnd(23, yB - 1), -7 * fs, 1)                  # contiguous axis, odd facet size
    ex = chk("extract_from_facet", bf, 3 * ss, 0, exact=True)
    chk("prepare_facet", numpy.ascontiguousarray(ex[:, :37].T), 2 * fs, 1)
    contrib = rnd(m, m)
    a0 = chk("add_to_subgrid", contrib, 5 * fs, 0)
    a01 = chk("add_to_subgrid", a0, -9 * fs, 1)
    chk("finish_subgrid", a01, [3 * ss, -5 * ss], xA)
    chk("finish_subgrid", a01, [3 * ss, -5 * ss], xA - 1)
    sg = rnd(xA, xA)
    prep = chk("prepare_subgrid", sg, [3 * ss, -5 * ss])
    e0 = chk("extract_from_subgrid", prep, 5 * fs, 0)
    e01 = chk("extract_from_subgrid", e0, -9 * fs, 1)
    acc1 = chk("add_to_facet", e01, -5 * ss, 1, exact=True)
    chk("finish_facet", acc1, -9 * fs, yB, 1)
    chk("finish_facet", numpy.ascontiguousarray(acc1.T), 5 * fs, yB - 1, 0)
    # fused column kernel (row gather + axis-1 prepare) == the two-step form
    got = core.extract_column(bf, 3 * ss, 2 * fs)
    want = orc.extract_column(ref, bf.astype(complex), 3 * ss, 2 * fs)
    assert relrms(got, want) < tol


@pytest.mark.parametrize("dtype,ftol,btol", [(numpy.complex128, 1e-10, 1e-9), (numpy.complex64, 2e-5, 4e-5)])
def test_streaming_classes_nonpow2(dtype, ftol, btol):
    """9 facets -> 25 subgrids -> 9 facets of the catalogue entry 1792[1]-n896-448 through SwiftlyForward /
    SwiftlyBackward (general launch sequences: no fused kernels exist for these sizes) vs the oracle's serial replica
    of the reference dataflow."""
    import ska_sdp_exec_swiftly_amd as sw
    from ska_sdp_exec_swiftly_amd.swift_configs import SWIFT_CONFIGS

    params = SWIFT_CONFIGS["1792[1]-n896-448"]
    assert (params["N"], params["yN_size"], params["xM_size"]) == (1792, 896, 448)
    cfg = sw.SwiftlyConfig(backend="hip", **params)
    facet_cfgs = sw.make_full_facet_cover(cfg)
    sg_cfgs = sw.make_full_subgrid_cover(cfg)
    yB = params["yB_size"]
    facets = []
    for j, f in enumerate(facet_cfgs):
        r = numpy.random.default_rng(900 + j)
        d = (r.standard_normal((yB, yB)) + 1j * r.standard_normal((yB, yB))).astype(numpy.complex64)
        facets.append((d * f.mask0[:, None] * f.mask1[None, :]).astype(dtype))
    fwd = sw.SwiftlyForward(cfg, list(zip(facet_cfgs, facets)), lru_forward=2)
    assert fwd.wave_axis == 0
    sgs = fwd.get_subgrid_tasks(sg_cfgs)
    ref = orc.OracleCore(params["W"], params["N"], params["xM_size"], params["yN_size"])
    items = [orc.CoverItem(c.off0, c.off1, c.size, c.mask0, c.mask1) for c in facet_cfgs]
    sitems = [orc.CoverItem(c.off0, c.off1, c.size, c.mask0, c.mask1) for c in sg_cfgs]
    want = orc.forward_all(ref, items, [f.astype(complex) for f in facets], sitems)
    errs = [relrms(g.cpu().numpy(), w) for g, w in zip(sgs, want)]
    assert max(errs) < ftol, max(errs)
    bwd = sw.SwiftlyBackward(cfg, facet_cfgs, lru_backward=2)
    bwd.add_new_subgrid_tasks(sg_cfgs, sgs)
    out = [f.cpu().numpy() for f in bwd.finish()]
    want_f = orc.backward_all(ref, items, sitems, want)
    errs = [relrms(g, w) for g, w in zip(out, want_f)]
    assert max(errs) < btol, max(errs)


def test_catalogue_coverage():
    """every catalogue entry constructs (reference tests/test_core.py:82-90) and every one of its transform lengths is
    a power of two or Q * 2^k with Q in {3, 5, 7, 9}: all 244 entries are executable in complex64"""
    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip
    from ska_sdp_exec_swiftly_amd.swift_configs import SWIFT_CONFIGS

    def native(n):
        while n % 2 == 0:
            n //= 2
        return n in (1, 3, 5, 7, 9)

    ok = 0
    for key, c in SWIFT_CONFIGS.items():
        lens = (c["yN_size"], c["xM_size"], c["xM_size"] * c["yN_size"] // c["N"])
        if all(native(n) for n in lens):
            ok += 1
    assert ok == len(SWIFT_CONFIGS) == 244, ok
    # spot-construct a few of each kind (construction uploads the tables)
    for key in ("96k[1]-n48k-512", "7k[1]-n3584-448", "12k[1]-n6k-512"):
        c = SWIFT_CONFIGS[key]
        SwiftlyCoreHip(c["W"], c["N"], c["xM_size"], c["yN_size"])


# the longest lengths of the catalogue per odd factor: beyond Bluestein's reach (convolution length 131072), native only
LONG = [
    ("96k[1]-n48k-512", 49152),   # 3 * 16384
    ("80k[1]-n40k-1k", 40960),    # 5 * 8192
    ("112k[1]-n56k-512", 57344),  # 7 * 8192
    ("72k[1]-n36k-512", 36864),   # 9 * 4096
]


@pytest.mark.parametrize("key,yN", LONG)
def test_long_nonpow2_facet_axes_c64(key, yN):
    """prepare_facet / finish_facet along both axes at the catalogue's longest yN = Q * 2^k (complex64) vs the oracle:
    a few rows along the contiguous axis, a few columns along the strided axis (four-step sub-transforms)."""
    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip
    from ska_sdp_exec_swiftly_amd.swift_configs import SWIFT_CONFIGS

    c = SWIFT_CONFIGS[key]
    assert c["yN_size"] == yN
    core = SwiftlyCoreHip(c["W"], c["N"], c["xM_size"], yN)
    ref = orc.OracleCore(c["W"], c["N"], c["xM_size"], yN)
    yB, fs = c["yB_size"], core.facet_off_step
    rng = numpy.random.default_rng(yN)
    rnd = lambda *shape: (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(numpy.complex64)  # noqa: E731
    rows = rnd(3, yB)
    for off in (0, 5 * fs, -7 * fs):
        got = core.prepare_facet(rows, off, axis=1)
        want = ref.prepare_facet(rows.astype(complex), off, 1)
        assert got.shape == (3, yN) and relrms(got, want) < 3e-6, (off, relrms(got, want))
    cols = rnd(yB, 5)
    got = core.prepare_facet(cols, 3 * fs, axis=0)
    want = ref.prepare_facet(cols.astype(complex), 3 * fs, 0)
    assert got.shape == (yN, 5) and relrms(got, want) < 3e-6, relrms(got, want)
    acc = rnd(3, yN)
    got = core.finish_facet(acc, -9 * fs, yB, 1)
    want = ref.finish_facet(acc.astype(complex), -9 * fs, yB, 1)
    assert relrms(got, want) < 3e-6, relrms(got, want)
    acc0 = rnd(yN, 5)
    got = core.finish_facet(acc0, 5 * fs, yB - 1, 0)
    want = ref.finish_facet(acc0.astype(complex), 5 * fs, yB - 1, 0)
    assert relrms(got, want) < 3e-6, relrms(got, want)


def test_nonpow2_c128_beyond_bluestein():
    """complex128 at yN = 3 * 4096: Bluestein would need a 32768-point complex128 convolution (no kernel); the
    radix-3 pass + 4096-point transforms run it to rounding"""
    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    W, N, xM, yN = 11.0, 24576, 1024, 12288
    core = SwiftlyCoreHip(W, N, xM, yN)
    ref = orc.OracleCore(W, N, xM, yN)
    rng = numpy.random.default_rng(5)
    x = rng.standard_normal((4, 8448)) + 1j * rng.standard_normal((4, 8448))
    got = core.prepare_facet(x, 3 * core.facet_off_step, axis=1)
    want = ref.prepare_facet(x, 3 * core.facet_off_step, 1)
    assert relrms(got, want) < 1e-12


def test_forward_band_pipeline_nonpow2_yN():
    """The contiguous-axis-first forward pipeline (wave_axis=1) at yN = 3 * 256 (catalogue entry
    1536[1]-n768-512: xM = 512, m = 256 powers of two): K1 through the radix-3 pass of the generic row kernels, K2
    through the radix-3 pass over the window columns + column-tile sub-transforms, subgrid side unchanged -- all 9
    facets -> 16 subgrids against the oracle's serial replica of the reference dataflow, and against wave_axis=0."""
    import torch

    import ska_sdp_exec_swiftly_amd as sw
    from ska_sdp_exec_swiftly_amd.swift_configs import SWIFT_CONFIGS

    params = SWIFT_CONFIGS["1536[1]-n768-512"]
    assert (params["N"], params["yN_size"], params["xM_size"]) == (1536, 768, 512)
    cfg = sw.SwiftlyConfig(backend="hip", **params)
    assert cfg.core.supports_band_pipeline(torch.complex64, 9) and cfg.core.supports_backward_band(torch.complex64)
    assert sw.api.preferred_wave_axis(cfg, torch.complex64, n_facets=9) == 1
    facet_cfgs = sw.make_full_facet_cover(cfg)
    sg_cfgs = sw.make_full_subgrid_cover(cfg)
    yB = params["yB_size"]
    facets = []
    for j, f in enumerate(facet_cfgs):
        r = numpy.random.default_rng(700 + j)
        d = (r.standard_normal((yB, yB)) + 1j * r.standard_normal((yB, yB))).astype(numpy.complex64)
        facets.append((d * f.mask0[:, None] * f.mask1[None, :]).astype(numpy.complex64))
    fwd = sw.SwiftlyForward(cfg, list(zip(facet_cfgs, facets)), subgrid_configs=sg_cfgs)
    assert fwd.wave_axis == 1
    got = [t.cpu().numpy() for t in fwd.get_subgrid_tasks(sg_cfgs)]
    ref = orc.OracleCore(params["W"], params["N"], params["xM_size"], params["yN_size"])
    items = [orc.CoverItem(c.off0, c.off1, c.size, c.mask0, c.mask1) for c in facet_cfgs]
    sitems = [orc.CoverItem(c.off0, c.off1, c.size, c.mask0, c.mask1) for c in sg_cfgs]
    want = orc.forward_all(ref, items, [f.astype(complex) for f in facets], sitems)
    errs = [relrms(g, w) for g, w in zip(got, want)]
    assert max(errs) < 2e-5, max(errs)
    fwd0 = sw.SwiftlyForward(cfg, list(zip(facet_cfgs, facets)), wave_axis=0)
    got0 = [t.cpu().numpy() for t in fwd0.get_subgrid_tasks(sg_cfgs)]
    assert max(relrms(a, b) for a, b in zip(got, got0)) < 2e-5


def test_prepare_facet_columns_nonpow2_yN():
    """K2 primitive at yN = 6144 = 3 * 2048 (catalogue 12k[1]-n6k-512, m = 256): window gather from plain band buffers +
    strided-axis prepare_facet (four-step sub-transforms of 2048 points) for 2 facets, with and without a row map."""
    import torch

    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip

    W, N, xM, yN = 11.0, 12288, 512, 6144
    core, ref = SwiftlyCoreHip(W, N, xM, yN), orc.OracleCore(W, N, xM, yN)
    m = core.xM_yN_size
    assert m == 256 and core.band_for_offsets([0, 448]) == (0, yN)
    rng = numpy.random.default_rng(33)
    yB0, F = 176, 2
    logical = (rng.standard_normal((F, yB0, yN)) + 1j * rng.standard_normal((F, yB0, yN))).astype(numpy.complex64)
    bands = torch.from_numpy(logical).cuda()
    off0s = [0, 4224]
    for use_rowmap in (False, True):
        rowmap, n_rows = core.subgrid_column_rows([0, 3 * 448, -5 * 448]) if use_rowmap else (None, yN)
        rm = rowmap.cpu().numpy() if rowmap is not None else numpy.arange(yN)
        for off1 in (7 * 448, -11 * 448):
            got = core.prepare_facet_columns(bands, off0s, (0, yN), off1, rowmap, n_rows).cpu().numpy()
            assert got.shape == (F, n_rows, m)
            for f in range(F):
                win = ref.extract_from_facet(logical[f].astype(complex), off1, axis=1)
                want = ref.prepare_facet(win / ref.facet_window(yB0)[:, None], off0s[f], axis=0)  # window NOT applied
                keep = rm >= 0
                rel = relrms(got[f][rm[keep]], want[keep])
                assert rel < 2e-6, (use_rowmap, off1, f, rel)


def test_backward_band_schedule_nonpow2_yN():
    """SwiftlyBackward(wave_axis=1) at yN = 3 * 256 (catalogue 1536[1]-n768-512): accumulate_facet_columns through the
    radix-3 pass with the gather-sum load + column-tile sub-transforms, finish_facet_band through the radix-3 pass of
    the generic row kernels -- all 16 subgrids -> 9 facets against the oracle's serial replica, and against the
    reference schedule (wave_axis=0)."""
    import torch

    import ska_sdp_exec_swiftly_amd as sw
    from ska_sdp_exec_swiftly_amd.swift_configs import SWIFT_CONFIGS

    params = SWIFT_CONFIGS["1536[1]-n768-512"]
    cfg = sw.SwiftlyConfig(backend="hip", **params)
    facet_cfgs = sw.make_full_facet_cover(cfg)
    sg_cfgs = sw.make_full_subgrid_cover(cfg)
    xA = params["xA_size"]
    rng = numpy.random.default_rng(77)
    subgrids = []
    for c in sg_cfgs:
        d = (rng.standard_normal((xA, xA)) + 1j * rng.standard_normal((xA, xA))).astype(numpy.complex64)
        subgrids.append((d * c.mask0[:, None] * c.mask1[None, :]).astype(numpy.complex64))
    ref = orc.OracleCore(params["W"], params["N"], params["xM_size"], params["yN_size"])
    items = [orc.CoverItem(c.off0, c.off1, c.size, c.mask0, c.mask1) for c in facet_cfgs]
    sitems = [orc.CoverItem(c.off0, c.off1, c.size, c.mask0, c.mask1) for c in sg_cfgs]
    want = orc.backward_all(ref, items, sitems, [s.astype(complex) for s in subgrids])
    dev = [torch.from_numpy(s).cuda() for s in subgrids]
    bwd = sw.SwiftlyBackward(cfg, facet_cfgs, subgrid_configs=sg_cfgs)
    by1 = sorted(range(len(sg_cfgs)), key=lambda k: sg_cfgs[k].off1)
    bwd.add_new_subgrid_tasks([sg_cfgs[k] for k in by1], [dev[k] for k in by1])
    assert bwd.wave_axis == 1
    got = [f.cpu().numpy() for f in bwd.finish()]
    errs = [relrms(g, w) for g, w in zip(got, want)]
    assert max(errs) < 4e-5, max(errs)
    bwd0 = sw.SwiftlyBackward(cfg, facet_cfgs, wave_axis=0)
    bwd0.add_new_subgrid_tasks(sg_cfgs, dev)
    got0 = [f.cpu().numpy() for f in bwd0.finish()]
    assert max(relrms(a, b) for a, b in zip(got, got0)) < 4e-5


def test_distributed_virtual_ranks_nonpow2_yN():
    """The multi-rank classes on the fused pipelines at yN = 3 * 256 (two virtual ranks in one process, the all-to-all
    replaced by an in-process shuffle of the flat buffers): DistributedForward(wave_axis=1) and
    DistributedBackward(wave_axis=1) against the single-process classes."""
    import torch

    import ska_sdp_exec_swiftly_amd as sw
    from ska_sdp_exec_swiftly_amd.distributed import DistributedBackward, DistributedForward
    from ska_sdp_exec_swiftly_amd.swift_configs import SWIFT_CONFIGS

    world = 2
    params = SWIFT_CONFIGS["1536[1]-n768-512"]
    cfg = sw.SwiftlyConfig(backend="hip", **params)
    facet_cfgs = sw.make_full_facet_cover(cfg)
    sg_cfgs = sw.make_full_subgrid_cover(cfg)
    yB = params["yB_size"]
    dev_facets = []
    for j, f in enumerate(facet_cfgs):
        r = numpy.random.default_rng(300 + j)
        d = (r.standard_normal((yB, yB)) + 1j * r.standard_normal((yB, yB))).astype(numpy.complex64)
        dev_facets.append(torch.from_numpy((d * f.mask0[:, None] * f.mask1[None, :]).astype(numpy.complex64)).cuda())
    ref_fwd = sw.SwiftlyForward(cfg, list(zip(facet_cfgs, dev_facets)), subgrid_configs=sg_cfgs)
    assert ref_fwd.wave_axis == 1
    fwds = [DistributedForward(cfg, facet_cfgs, dev_facets, subgrid_configs=sg_cfgs, wave_axis=1, dtype=torch.complex64,
                               rank_world=(r, world)) for r in range(world)]
    bwds = [DistributedBackward(cfg, facet_cfgs, rank_world=(r, world), wave_axis=1, subgrid_configs=sg_cfgs,
                                dtype=torch.complex64) for r in range(world)]
    ref_bwd = sw.SwiftlyBackward(cfg, facet_cfgs, subgrid_configs=sg_cfgs)

    def shuffle(sends, in_counts):
        starts = [numpy.concatenate([[0], numpy.cumsum(c)]) for c in in_counts]
        return [torch.cat([sends[s][int(starts[s][r]) : int(starts[s][r + 1])] for s in range(world)]) for r in range(world)]

    waves = {}
    for c in sg_cfgs:
        waves.setdefault(c.off1, []).append(c)
    for wave in waves.values():
        want = ref_fwd.get_wave(wave)
        packed = [f.pack_wave(wave) for f in fwds]
        recvs = shuffle([p[0] for p in packed], [p[1] for p in packed])
        got = {}
        for r, f in enumerate(fwds):
            mine, res = f.unpack_wave(wave, recvs[r])
            for k, i in enumerate(mine):
                got[i] = res[k]
        assert sorted(got) == list(range(len(wave)))
        scale = float(want.abs().max())
        for i in range(len(wave)):
            assert float((got[i] - want[i]).abs().max()) <= 2e-5 * scale
        ref_bwd.add_new_subgrid_tasks(wave, [want[i] for i in range(len(wave))])
        packed = [b.pack_wave(wave, [want[i] for i in b.sharding.subgrids_of(len(wave))]) for b in bwds]
        recvs = shuffle([p[0] for p in packed], [p[1] for p in packed])
        for r, b in enumerate(bwds):
            b.unpack_wave(wave, recvs[r])
    assert ref_bwd.wave_axis == 1
    ref = ref_bwd.finish()
    for b in bwds:
        idx, out = b.finish()
        for j, o in zip(idx, out):
            assert float((o - ref[j]).abs().pow(2).mean().sqrt()) <= 3e-5 * float(ref[j].abs().pow(2).mean().sqrt())
