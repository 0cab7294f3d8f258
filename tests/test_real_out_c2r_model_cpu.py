"""
The dataflow of the half-length backward finish (csrc/swiftly_rowc2r.h, ``swiftly_hip_finish_facet_band_c2r``) restated in
float32 numpy and compared with the complex128 oracle at yN = 32768, without a device: which four band elements every
half-length input Z[e] is made of (lane t, register r: e = t + 512 r), lane 0's own mirrors, which (register, source) pairs
the workgroup does not load at all, and where the output pair (y[2n], y[2n+1]) lands in the facet row.

With N = 32768, M = N / 2, X the band row on the padded axis in plain index (zero outside the band), W = exp(-2 pi i / N):

    2 H[k] = X[k] + conj X[(N - k) mod N]
    2 Z[e] = (2 H[e] + 2 H[e + M]) + i W^e (2 H[e] - 2 H[e + M]) ,   e < M        (the 1/2 rides on the scale)
    z      = FFT_M(Z) ;   y[2n] = Re z[n] ,  y[2n + 1] = Im z[n] ,   y = Re FFT_N(X)

Only the transform itself is numpy's (in double); loads, recombination, window and scale are float32 as in the kernel, so
the error against the oracle is the rounding of those few operations.
"""
import numpy
import pytest

from oracle import swiftly_oracle as orc

W_PARAM, N_IMAGE, XM, YN = 10.875, 65536, 1024, 32768  # the "c15" core of tests/band_instance_cases.py
M = YN // 2
T, P = 512, 32
PLAN_BAND = (10720, 11488)
FACETS = [(352, 8194), (22528, 0), (22528, 22528), (22528, -22528), (24576, 666), (32766, 667)]
BANDS = [(0, 32768), PLAN_BAND, (32001, 2049), (10737, 11471), (16383, 2)]
ROWS = 3
#: a float32 recombination and window product in front of and behind an exact transform
MODEL_BOUND = 4e-7

_REF = {}


def ref_core():
    if "core" not in _REF:
        _REF["core"] = orc.OracleCore(W_PARAM, N_IMAGE, XM, YN)
    return _REF["core"]


def store_shift(yB, off):
    """``facet_in_padded_facet(...).a`` of csrc/swiftly_geometry.h: facet column of centred column c is (c + a) mod yN"""
    return (-(off + YN // 2 - yB // 2)) % YN


def source_offsets(band_start):
    """band element index d of the four sources of every e < M, as the kernel computes them: [4, M] (X[e], X[e + M],
    X[(N - e) mod N], X[(M - e) mod N]); plain k is centred column (k + N/2) mod N, d = (column - band_start) mod N"""
    e = numpy.arange(M)
    d1 = (e + M - band_start) % YN
    d2 = (d1 + M) % YN
    d3 = (M - band_start - e) % YN
    d4 = (d3 + M) % YN
    return numpy.stack([d1, d2, d3, d4])


def pair_is_loaded(band, r, source):
    """the workgroup-uniform decision of the kernel: are the 512 consecutive band indices of (register r, source) not wholly
    outside the band?  Sources 0 / 1 ascend with the lane, 2 / 3 descend."""
    start, length = band
    base = [(T * r + M - start) % YN, (T * r - start) % YN, (M - start - T * r - (T - 1)) % YN, (-start - T * r - (T - 1)) % YN][source]
    return not (base >= length and base + (T - 1) < YN)


def loaded_pairs(band):
    return sum(pair_is_loaded(band, r, s) for r in range(P) for s in range(4))


def model(rows, band, yB, off, window, scale=1.0):
    """float32 restatement of the kernel for band rows ``rows[nrows, band_len]`` (complex64): [nrows, yB] float32"""
    start, length = band
    assert rows.dtype == numpy.complex64 and rows.shape[1] == length
    d = source_offsets(start)
    src = numpy.zeros((4, rows.shape[0], M), dtype=numpy.complex64)
    for s in range(4):
        for r in range(P):
            if not pair_is_loaded(band, r, s):
                assert (d[s, T * r : T * (r + 1)] >= length).all()  # a skipped pair holds nothing
                continue
            ds = d[s, T * r : T * (r + 1)]
            ok = ds < length  # the range check of the buffer load
            src[s][:, T * r : T * (r + 1)][:, ok] = rows[:, ds[ok]]
    a, b, c, dd = src
    fwd_sum, fwd_dif = a + b, a - b
    mir_sum, mir_dif = numpy.conj(c + dd), numpy.conj(c - dd)
    w = numpy.exp(-2j * numpy.pi * numpy.arange(M) / YN).astype(numpy.complex64)
    Z = (fwd_sum + mir_sum) + (1j * (w * (fwd_dif + mir_dif))).astype(numpy.complex64)
    z = numpy.fft.fft(Z.astype(numpy.complex128), axis=1).astype(numpy.complex64)
    out = numpy.full((rows.shape[0], yB), numpy.nan, dtype=numpy.float32)
    st_a = store_shift(yB, off)
    assert st_a % 2 == 0 and yB % 2 == 0
    n = numpy.arange(M)
    col = (2 * n + M + st_a) % YN  # facet column of y[2n]; y[2n + 1] is the next one
    keep = col < yB
    assert (col[keep] % 2 == 0).all() and (col[keep] + 1 < yB).all()
    sc = numpy.float32(0.5 * scale)
    win = window.astype(numpy.float32)
    out[:, col[keep]] = z.real[:, keep] * win[col[keep]] * sc
    out[:, col[keep] + 1] = z.imag[:, keep] * win[col[keep] + 1] * sc
    assert numpy.isfinite(out).all()  # every facet column is written exactly once
    return out


def oracle(rows, band, yB, off, mask):
    start, length = band
    full = numpy.zeros((rows.shape[0], YN), dtype=complex)
    full[:, (start + numpy.arange(length)) % YN] = rows
    return ref_core().finish_facet(full, off, yB, axis=1).real * mask[None, :]


def relrms(got, want):
    return float(numpy.sqrt(numpy.mean(numpy.abs(got - want) ** 2) / numpy.mean(numpy.abs(want) ** 2)))


def band_rows(rng, length):
    return (rng.standard_normal((ROWS, length)) + 1j * rng.standard_normal((ROWS, length))).astype(numpy.complex64)


def mask_of(rng, yB):
    mask = (rng.random(yB) > 0.15).astype(float)
    assert 0 < mask.sum() < yB
    return mask


def test_the_identity_in_double():
    """the transform of the issue, in complex128, at N = 256 and at N = 32768"""
    rng = numpy.random.default_rng(1)
    for n in (256, YN):
        m = n // 2
        X = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        H = (X + numpy.conj(X[(n - numpy.arange(n)) % n])) / 2
        e = numpy.arange(m)
        Z = (H[:m] + H[m:]) + 1j * numpy.exp(-2j * numpy.pi * e / n) * (H[:m] - H[m:])
        z = numpy.fft.fft(Z)
        y = numpy.fft.fft(X).real
        assert numpy.abs(z.real - y[0::2]).max() < 1e-9 * numpy.abs(y).max()
        assert numpy.abs(z.imag - y[1::2]).max() < 1e-9 * numpy.abs(y).max()


def test_lane_zero_reads_its_own_mirrors():
    """e = 0 is made of X[0] and X[M] alone, e = 512 v of X[512 v], X[512 v + M] and their mirrors N - 512 v, M - 512 v"""
    d = source_offsets(0)  # band (0, N): d is the centred column
    plain = (d - M) % YN
    assert list(plain[:, 0]) == [0, M, 0, M]
    for v in range(1, P):
        assert list(plain[:, T * v]) == [T * v, T * v + M, YN - T * v, M - T * v]


@pytest.mark.parametrize("yB,off", FACETS)
def test_facets_on_the_plan_band(yB, off):
    rng = numpy.random.default_rng(100 + yB + off % 1000)
    rows, mask = band_rows(rng, PLAN_BAND[1]), mask_of(rng, yB)
    win = mask * ref_core().facet_window(yB)
    got, want = model(rows, PLAN_BAND, yB, off, win), oracle(rows, PLAN_BAND, yB, off, mask)
    err = relrms(got, want)
    print(f"C2RMODEL facet {yB} off {off}: {err:.3e}")
    assert err < MODEL_BOUND
    assert not got[:, mask == 0].any()


@pytest.mark.parametrize("band", BANDS)
def test_bands(band):
    yB, off = 22528, 0
    rng = numpy.random.default_rng(200 + band[0])
    rows, mask = band_rows(rng, band[1]), mask_of(rng, yB)
    win = mask * ref_core().facet_window(yB)
    got, want = model(rows, band, yB, off, win), oracle(rows, band, yB, off, mask)
    err = relrms(got, want)
    print(f"C2RMODEL band {band}: {err:.3e}, {loaded_pairs(band)} of {4 * P} (register, source) pairs loaded")
    assert err < MODEL_BOUND


def test_pairs_loaded():
    """every pair on the full band; on the plan's band the 512-index runs that touch 11488 columns: 23 or 24 of the 64
    ascending and as many of the 64 descending ones; two columns: at most two runs per direction"""
    assert loaded_pairs((0, YN)) == 4 * P
    for band in (PLAN_BAND, (10736, 11472)):
        fwd = sum(pair_is_loaded(band, r, s) for r in range(P) for s in (0, 1))
        mir = sum(pair_is_loaded(band, r, s) for r in range(P) for s in (2, 3))
        assert 23 <= fwd <= 24 and 23 <= mir <= 24, (band, fwd, mir)
    assert loaded_pairs((16383, 2)) <= 4
