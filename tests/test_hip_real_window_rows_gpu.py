"""
Real-valued (float32) facets through the whole-row K1 of the accurate order (``swiftly_hip_prepare_facet_window_rows_real``, the
``REAL`` instances of ``row_pass_whole_kernel<NSEG, WIN>``) and through ``SwiftlyForward(...,
facet_dtype=torch.float32)``.

The kernel loads a lane's two adjacent reals with one 8-byte load and runs the complex instance's operations on a zero
imaginary part, all of which are exact: the window rows must be ``torch.equal`` to what the complex entry point gives for
``x.to(complex64)``.  The bounds against ``finish_axis1_rows`` (5e-7) and against the oracle composition (2.5e-6) are those of
``test_window_rows_store_of_the_whole_row_k1_matches_the_row_pass_per_wave`` (tests/test_hip_band_pipeline_gpu.py), whose
facet offsets and waves these tests use.  Every case runs the 32768-point core of that file, the smallest the kernel exists
for.
"""
import ctypes

import numpy
import pytest

from test_band_instances_cpu import INST
from test_hip_band_pipeline_gpu import W64, N64, xM64, yN64, band_cols, core64, relrms
from test_hip_real_facets_gpu import _real_problem, _run

pytestmark = pytest.mark.gpu

M = 512
SIZE = 352
#: (facet offset, wave offsets): band start / end windows, odd and even window starts, a band that wraps
GROUPS = ((0, [0, 928, 3 * 928, -2 * 928]), (64 * 352, [-928, 5 * 928, 7 * 928 + 2, 12 * 928 + 6]),
          (-32 * 352, [30 * 928, 33 * 928, 35 * 928 + 4] + [30 * 928 + 2 * k for k in range(1, 9)]))
_shared = {}


def _rows(rows, size=SIZE, seed=117):
    """float32 rows on the device and their promoted copy (made once per shape, never written)"""
    import torch

    key = (rows, size, seed)
    if key not in _shared:
        x = numpy.random.default_rng(seed).standard_normal((rows, size)).astype(numpy.float32)
        xt = torch.from_numpy(x).cuda()
        _shared[key] = (x, xt, xt.to(torch.complex64))
    return _shared[key]


def _last_instance():
    from ska_sdp_exec_swiftly_amd import _lib

    buf = (ctypes.c_int32 * len(INST))()
    count = int(_lib.load().swiftly_hip_last_band_instance(buf, len(INST)))
    return count, dict(zip(INST, buf))


def _nan(shape):
    import torch

    return torch.full(shape, complex("nan+nanj"), dtype=torch.complex64, device="cuda")  # both parts


def _starts(core, band, wave_off1s):
    import torch

    starts = core.window_starts(band, wave_off1s)
    assert min(starts) >= 0 and max(starts) + M <= band[1]
    return starts, torch.tensor(starts, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("rows", [300, 1])
def test_16_segment_instance_and_the_persistent_loop(rows):
    """more rows than CUs: the prefetch of real rows and the stage reuse run; and a single row"""
    import torch

    core, _ = core64()
    _, xt, xc = _rows(rows)
    for foff, wave_off1s in GROUPS:
        band = core.band_for_offsets(wave_off1s)
        assert core.supports_window_rows(band, SIZE, [foff], real=True)
        starts, sd = _starts(core, band, wave_off1s)
        bands1 = core.prepare_facet_band(xc, foff, band)[None]
        for shape in ((len(starts), rows, M), (rows, len(starts) * M)):  # wave-major; the windows of a row side by side
            want = core.prepare_facet_window_rows(xc, foff, band, sd, _nan(shape))
            count0, _ = _last_instance()
            got = core.prepare_facet_window_rows(xt, foff, band, sd, _nan(shape))
            count, inst = _last_instance()
            assert count == count0 + 1  # one band row launch
            assert (inst["status"], inst["family"], inst["nseg"], inst["st"], inst["real"]) == (0, 1, 16, 3, 1), inst
            assert got.dtype == torch.complex64 and bool(torch.isfinite(torch.view_as_real(got)).all())
            assert torch.equal(got, want), (foff, shape)
            if len(shape) == 2:
                got = got.reshape(rows, len(starts), M).transpose(0, 1)
            for w, off1 in enumerate(wave_off1s):
                ref, wband = core.finish_axis1_rows(bands1, [foff], band, off1)
                assert wband[0] == (band[0] + starts[w]) % yN64
                rel = relrms(got[w].cpu().numpy(), ref[0].cpu().numpy())
                assert rel < 5e-7, (foff, w, rel)


def test_22_and_24_segment_instances():
    """full-size rows of the timed workload (a facet whose position in the padded row is not a multiple of a segment touches
    23 of them), against the promoted call and the oracle's window rows"""
    import torch

    core, ref = core64()
    x, xt, xc = _rows(3, 22528, seed=119)
    wave_off1s = [0, 928, -928 * 3, 928 * 6]
    band = core.band_for_offsets(wave_off1s)
    _, sd = _starts(core, band, wave_off1s)
    k = numpy.arange(M)
    seen = set()
    for foff in (22528, 22528 + 352, -22528 + 2):
        assert core.supports_window_rows(band, 22528, [foff], n_windows=4, real=True)
        want = core.prepare_facet_window_rows(xc, foff, band, sd, _nan((4, 3, M)), fold_other_axis_window=False)
        got = core.prepare_facet_window_rows(xt, foff, band, sd, _nan((4, 3, M)), fold_other_axis_window=False)
        _, inst = _last_instance()
        assert (inst["status"], inst["family"], inst["st"], inst["real"]) == (0, 1, 3, 1) and inst["nseg"] in (22, 24), inst
        seen.add(inst["nseg"])
        assert torch.equal(got, want), foff
        prepared = ref.prepare_facet(x.astype(complex), foff, 1)                           # [3, yN], complex128
        sp = foff * xM64 // N64
        for w, off1 in enumerate(wave_off1s):
            s1 = off1 * yN64 // N64
            placed = ref.add_to_subgrid(ref.extract_from_facet(prepared, off1, 1), foff, 1)
            Z = placed[:, (k + xM64 // 2 - M // 2 + sp) % xM64]
            want_logical = Z[:, (k + s1) % M]
            wstart = (yN64 // 2 - M // 2 + s1) % yN64
            cols = band_cols(yN64, (wstart, M))[(wstart + k) % yN64]
            rel = relrms(got[w].cpu().numpy()[:, cols], want_logical)
            print(f"real window rows, facet offset {foff}, wave {off1}: {rel:.3e} against the oracle")
            assert rel < 2.5e-6, (foff, w, rel)
    assert seen == {22, 24}


def test_descriptor_length_and_pitch():
    """rows that are a view of a wider buffer whose gap is NaN (even pitch, 8-byte-aligned rows): a descriptor that is too
    long, or an offset that is not halved, reads the NaNs"""
    import torch

    core, _ = core64()
    rows = 9
    _, xt, xc = _rows(rows)
    buf = torch.full((rows, SIZE + 6), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[:, :SIZE]
    view.copy_(xt)
    assert view.stride(0) % 2 == 0 and view.data_ptr() % 8 == 0 and not view.is_contiguous()
    for foff, wave_off1s in GROUPS[:2]:
        band = core.band_for_offsets(wave_off1s)
        starts, sd = _starts(core, band, wave_off1s)
        want = core.prepare_facet_window_rows(xc, foff, band, sd, _nan((len(starts), rows, M)))
        got = core.prepare_facet_window_rows(view, foff, band, sd, _nan((len(starts), rows, M)))
        assert bool(torch.isfinite(torch.view_as_real(got)).all()) and torch.equal(got, want), foff


def test_compacted_input_and_folded_window():
    import torch

    core, _ = core64()
    rows = 9
    _, xt, xc = _rows(rows)
    foff, wave_off1s = GROUPS[1]
    band = core.band_for_offsets(wave_off1s)
    starts, sd = _starts(core, band, wave_off1s)
    results = []
    for kw in (dict(rows_of=(SIZE, 120)), dict(rows_of=(SIZE, SIZE - rows)), dict(fold_other_axis_window=False), dict()):
        want = core.prepare_facet_window_rows(xc, foff, band, sd, _nan((len(starts), rows, M)), **kw)
        got = core.prepare_facet_window_rows(xt, foff, band, sd, _nan((len(starts), rows, M)), **kw)
        assert bool(torch.isfinite(torch.view_as_real(got)).all()) and torch.equal(got, want), kw
        results.append(got)
    # (the four forms are four different answers: the window of the other axis is folded in, and it is the block's own)
    assert all(not torch.equal(results[i], results[j]) for i in range(4) for j in range(i))


def test_refusals_not_approximations():
    import torch

    from ska_sdp_exec_swiftly_amd import SwiftlyCoreHip, _lib

    core, _ = core64()
    rows = 4
    _, xt, _ = _rows(rows)
    foff, wave_off1s = GROUPS[0]
    band = core.band_for_offsets(wave_off1s)
    starts, sd = _starts(core, band, wave_off1s)

    def refused(c, facet, band, sd, text):
        out = _nan((int(sd.numel()), rows, M))
        with pytest.raises(NotImplementedError, match=text):
            c.prepare_facet_window_rows(facet, foff, band, sd, out)
        torch.cuda.synchronize()
        assert bool(torch.isnan(torch.view_as_real(out)).all())  # nothing was written

    # an odd pitch; a base that is only 4-byte aligned: there is no 4-byte-load form
    odd = torch.zeros((rows, SIZE + 5), dtype=torch.float32, device="cuda")[:, :SIZE]
    odd.copy_(xt)
    assert odd.stride(0) % 2 == 1
    refused(core, odd, band, sd, "an even real row stride and an 8-byte-aligned input")
    shifted = torch.zeros((rows, SIZE + 6), dtype=torch.float32, device="cuda")[:, 1 : 1 + SIZE]
    shifted.copy_(xt)
    assert shifted.stride(0) % 2 == 0 and shifted.data_ptr() % 8 == 4
    refused(core, shifted, band, sd, "an even real row stride and an 8-byte-aligned input")
    _, inst = _last_instance()
    assert inst["status"] == -2
    # a band wider than the LDS stage
    wide = (0, core.WINDOW_ROWS_STAGE_COLUMNS + 64)
    assert not core.supports_window_rows(wide, SIZE, [foff], real=True)
    refused(core, xt, wide, torch.zeros(1, dtype=torch.int32, device="cuda"), "prepare_facet_window_rows")
    # a core without the feature: 16384-point rows have a real-load K1 and no window rows
    small = SwiftlyCoreHip(W64, N64 // 2, xM64, yN64 // 2)
    assert small.xM_yN_size == M and small.supports_real_facets()
    assert not small.supports_window_rows((0, 4096), SIZE, [foff], real=True)
    assert _lib.last_error().startswith("window rows:") or _lib.last_error().startswith("real window rows:")
    refused(small, xt, (0, 4096), torch.zeros(1, dtype=torch.int32, device="cuda"), "real window rows:")
    # the output of a float32 facet is complex64
    with pytest.raises(ValueError):
        core.prepare_facet_window_rows(xt, foff, band, sd, torch.zeros((len(starts), rows, M), dtype=torch.complex128, device="cuda"))


def test_forward_keeps_float32_facets_real_in_the_accurate_order():
    """the small-rows problem of tests/test_hip_real_facets_gpu.py under ``axis1_first=True`` (mode 2: the whole-row K1)"""
    torch, sw, _, facet_cfgs, reals, sg_cfgs, ordered = _real_problem(45)
    P = dict(W=W64, fov=1.0, N=N64, yB_size=SIZE, yN_size=yN64, xA_size=928, xM_size=xM64)
    cfg = sw.SwiftlyConfig(backend="hip", axis1_first=True, **P)
    promoted = [r.to(torch.complex64) for r in reals]
    base_fwd, base = _run(sw, cfg, facet_cfgs, promoted, sg_cfgs, ordered, wave_axis=1)
    assert base_fwd._axis1() == 2 and base_fwd.facet_dtype == torch.complex64  # pylint: disable=protected-access
    assert len(base) == 12 and all(float(b.abs().max()) > 0 for b in base)
    for value in (torch.float32, "float32"):
        for data in (reals, [r.cpu().numpy() for r in reals]):
            fwd, got = _run(sw, cfg, facet_cfgs, data, sg_cfgs, ordered, wave_axis=1, facet_dtype=value)
            assert fwd.facet_dtype == torch.float32 and fwd.dtype == torch.complex64
            ingested = [fwd._ingest.ready(j) for j in range(len(reals))]  # pylint: disable=protected-access
            assert all(t.dtype == torch.float32 and t.is_cuda and torch.equal(t, r) for t, r in zip(ingested, reals))
            assert fwd._axis1() == 2  # pylint: disable=protected-access
            _, inst = _last_instance()
            assert (inst["family"], inst["st"], inst["real"]) == (1, 3, 1)  # K1 was the last band row launch of this thread
            assert len(got) == 12
            for g, b in zip(got, base):
                assert g.dtype == torch.complex64 and torch.equal(g, b)
    # without the keyword: today's behaviour -- promoted, mode 2
    for data in (reals, [r.cpu().numpy() for r in reals]):
        fwd, got = _run(sw, cfg, facet_cfgs, data, sg_cfgs, ordered, wave_axis=1)
        assert fwd.facet_dtype == torch.complex64 and fwd._axis1() == 2  # pylint: disable=protected-access
        assert fwd._ingest.ready(0).dtype == torch.complex64  # pylint: disable=protected-access
        assert all(torch.equal(g, b) for g, b in zip(got, base))
    # one complex facet among them: the keyword is a promise the data do not keep
    mixed = [reals[0], promoted[1], reals[2]]
    with pytest.raises(ValueError, match="float32"):
        sw.SwiftlyForward(cfg, list(zip(facet_cfgs, mixed)), subgrid_configs=sg_cfgs, wave_axis=1, facet_dtype=torch.float32)
    # any other value
    with pytest.raises(ValueError, match="facet_dtype"):
        sw.SwiftlyForward(cfg, list(zip(facet_cfgs, reals)), subgrid_configs=sg_cfgs, wave_axis=1, facet_dtype=torch.float64)


def test_forward_facet_dtype_promotes_where_no_real_k1_exists():
    """``wave_axis=0`` has no real K1: the facets are promoted, the property says so, the values are the promoted run's"""
    torch, sw, cfg, facet_cfgs, reals, sg_cfgs, _ = _real_problem(45)
    ordered = sorted(sg_cfgs, key=lambda c: (c.off0, c.off1))
    _, base = _run(sw, cfg, facet_cfgs, [r.to(torch.complex64) for r in reals], sg_cfgs, ordered, wave_axis=0)
    fwd, got = _run(sw, cfg, facet_cfgs, reals, sg_cfgs, ordered, wave_axis=0, facet_dtype=torch.float32)
    assert fwd.facet_dtype == torch.complex64
    assert fwd._ingest.ready(0).dtype == torch.complex64  # pylint: disable=protected-access
    assert len(got) == 12 and all(torch.equal(g, b) for g, b in zip(got, base))
