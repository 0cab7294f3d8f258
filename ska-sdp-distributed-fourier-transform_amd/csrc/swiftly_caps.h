// Capability table of libswiftly_hip.so: which kernels and pipelines exist for a configuration, as pure host functions
// of the sizes (no handle, no HIP call).  The entry points refuse through these functions and swiftly_hip_supports /
// swiftly_hip_limit / swiftly_hip_mixed_factor (include/swiftly_hip.h) answer from them, so every rule lives here once;
// the Python layer holds none.
#pragma once

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/swiftly_hip.h"

namespace swf {

static inline int ilog2_exact(int64_t n) {
    if (n <= 0 || (n & (n - 1))) return -1;
    int l = 0;
    while ((int64_t(1) << l) < n) l++;
    return l;
}

// ---------------------------------------------------------------------------------------------------------
// lengths and instance tables of the kernels
constexpr int kMinLogN = 3;        // power-of-two lengths of the row kernels (swiftly_rows.h): 8 points ...
constexpr int kMaxLogNFloat = 15;  // ... to 32768 in one complex64 launch

constexpr int kSumFinishMaxFacets = 64;  // facets summed by one sum_finish_facets call (table sizes of swiftly_sumfinish.h)
constexpr int kWholeMaxWindows = 256;    // window table of the whole-row K1 (LDS, swiftly_rowwhole.h)

bool col_pass_f64_supported(int logn);  // float64-arithmetic instances (ColPassArgs::f64; also the complex128 ones): col_pass.hip
int row_pass_whole_stage_columns();     // physical band columns (both parities) the window-rows epilogue can stage: row_whole.hip

// (m, xM) instances of the fused sum + finish row kernels (sum_finish.hip), as log2
#define SF_PAIRS(X) X(7, 8) X(7, 10) X(8, 9) X(8, 10) X(9, 10) X(9, 11) X(10, 11) X(10, 12)
// complex128 sum_finish_facets (register form, m-point transform of K3 in one column pass: m <= 512; (9, 11) would keep 32
// complex128 accumulator values per lane and spills even at 256 VGPRs)
#define SF_PAIRS_C128(X) X(7, 8) X(7, 10) X(8, 9) X(8, 10) X(9, 10)
// complex128 split_prepare_facets (backward mirror of the above; the prepared row stays in LDS, the axis-0 remainder is one
// complex128 m-point column pass: m <= 512): the same five pairs, none spills
#define SPLIT_PAIRS_C128(X) X(7, 8) X(7, 10) X(8, 9) X(8, 10) X(9, 10)

// (m, xM) instances of the column kernel that finishes the strided subgrid axis per facet off1 group (group_finish.hip):
// the benchmarked pair and the smallest pair of SF_PAIRS
#define GF_PAIRS(X) X(7, 8) X(9, 10)
constexpr int kGroupFinishMaxFacets = kSumFinishMaxFacets;  // facet table of swiftly_groupfinish.h

#define SF_HAS(M, XX) \
    if (logm == M && logx == XX) return true;
inline bool group_finish_supported(int logm, int logx) {
    GF_PAIRS(SF_HAS)
    return false;
}
inline bool sum_finish_supported(int logm, int logx) {
    SF_PAIRS(SF_HAS)
    return false;
}
inline bool sum_finish_c128_supported(int logm, int logx) {  // complex128 sum_finish_facets_kernel instances
    SF_PAIRS_C128(SF_HAS)
    return false;
}
inline bool split_prepare_c128_supported(int logm, int logx) {  // complex128 split_prepare_facets_kernel instances
    SPLIT_PAIRS_C128(SF_HAS)
    return false;
}
#undef SF_HAS
// "(128, 256), (128, 1024), ...": the sizes of SF_PAIRS_C128 / SPLIT_PAIRS_C128 for refusal texts
#define SF_NAME(M, XX) s += (s.empty() ? "(" : ", (") + std::to_string(1 << M) + ", " + std::to_string(1 << XX) + ")";
inline std::string sum_finish_c128_sizes() {
    std::string s;
    SF_PAIRS_C128(SF_NAME)
    return s;
}
inline std::string split_prepare_c128_sizes() {
    std::string s;
    SPLIT_PAIRS_C128(SF_NAME)
    return s;
}
#undef SF_NAME

// n = Q * 2^k with Q in {3, 5, 7, 9} and 2^k a length the power-of-two kernels take (one radix-Q pass in front of them,
// swiftly_mixed.h): Q and k, else false (powers of two included: they need no pass)
inline bool mixed_factor(int64_t n, int* Q, int* logM) {
    if (n <= 0) return false;
    for (int q : {3, 5, 7, 9}) {
        if (n % q) continue;
        const int l = ilog2_exact(n / q);
        if (l >= kMinLogN) {
            *Q = q;
            *logM = l;
            return true;
        }
    }
    return false;
}

// ---------------------------------------------------------------------------------------------------------
// a configuration: the sizes and their exact log2 (-1 when not a power of two); base of the handle
struct Sizes {
    int64_t N = 0, yN = 0, xM = 0, m = 0;
    int log_yN = -1, log_xM = -1, log_m = -1;
};

inline std::string reason(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return buf;
}
// parameter checks of core.py:55-74: empty when (N, yN, xM) is a configuration, else what is wrong
inline std::string check_sizes(int64_t N, int64_t yN, int64_t xM) {
    if (N <= 0 || yN <= 0 || xM <= 0) return "sizes must be positive";
    if (N % yN != 0) return reason("Image size %lld not divisible by facet size %lld!", (long long)N, (long long)yN);
    if (N % xM != 0) return reason("Image size %lld not divisible by subgrid size %lld!", (long long)N, (long long)xM);
    if ((xM * yN) % N != 0)
        return reason("Contribution size not integer with image size %lld, subgrid size %lld and facet size %lld!", (long long)N,
                      (long long)xM, (long long)yN);
    return {};
}
inline Sizes make_sizes(int64_t N, int64_t yN, int64_t xM) {
    Sizes s;
    s.N = N; s.yN = yN; s.xM = xM; s.m = xM * yN / N;
    s.log_yN = ilog2_exact(yN); s.log_xM = ilog2_exact(xM); s.log_m = ilog2_exact(s.m);
    return s;
}

// ---------------------------------------------------------------------------------------------------------
// limits of the band pipelines that no single kernel table states
constexpr int kBandMinLog = 6;  // K2 (prepare_facet_columns) takes m >= 64: the facet kernels behind it run 64 lanes per transform;
                                // the same floor for yN (and 2^k of Q * 2^k) is a policy of the streaming layer
constexpr int kBandMaxLogYN = kMaxLogNFloat + 1;  // forward K1 in complex64 (prepare_facet_band): the band row kernel, 65536 points
constexpr int kBandMaxLogYNC128 = 15;  // forward K1 in complex128: the two-kernel long-row form (swiftly_rowslong.h), 32768 points
constexpr int kBandMixedMaxLog = kMaxLogNFloat;  // yN = Q * 2^k: sub-transforms of the radix-Q tables (make_mixed)
constexpr int kFusedMaxLogM = 10;  // K3 (transform_contributions): m-point transform in ONE column pass (kColPassMaxLog)
// backward band (accumulate_facet_columns + finish_facet_band): the lengths both entry points run and the facet sweep
// (tests/test_hip_facet_sweep_gpu.py) pins on the oracle.  The column-tile passes alone would reach from 2^2
// (kColPassMinLog) to 2^20, but the handle holds no twiddle table below 2^3 (kMinLogN) and no float table above 2^16, and
// finish_facet_band has no row kernel above 65536 points; no catalogue entry lies outside 256 .. 65536.
constexpr int kBackwardBandMinLogYN = kBandMinLog;
constexpr int kBackwardBandMaxLogYN = kMaxLogNFloat + 1;
constexpr int kSplitBandMinLogYN = 14;  // yN the two-workgroup long-row K1 produces a band for (row_pass.hip)
constexpr int kSplitBandMaxLogYN = 16;
constexpr int kPlacedMaxLogXM = 11;  // sum_finish_facets, placed mode (axis-1-first pipeline): not in the wave-parallel form (xM >= 4096)
// window rows (whole-row K1 that finishes the contiguous axis, row_whole.hip): instances for 32768-point rows with the
// 512-point epilogue, in front of the placed sum_finish_facets
constexpr int kWindowRowsLogYN = 15, kWindowRowsLogM = 9;

// Band layout: parity-split where the two-workgroup long-row kernel produces the band (yN >= 16384), else PLAIN (logical
// column d of the band at physical column d; K1 is the generic contiguous-axis transform and keeps the whole padded axis).
inline bool band_is_split(const Sizes* s) { return s->log_yN >= kSplitBandMinLogYN && s->log_yN <= kSplitBandMaxLogYN; }
// complex128 band pipeline (K2, K3, sum_finish_facets): power-of-two padded facets up to 32768 points in the plain band
// layout, m-point transforms in one column pass (m <= 512) and a complex128 sum_finish_facets instance for (m, xM)
inline bool band_pipeline_c128_supported(const Sizes* s) {
    return s->log_yN >= kBandMinLog && s->log_yN <= kBandMaxLogYNC128 && col_pass_f64_supported(s->log_m) &&
           sum_finish_c128_supported(s->log_m, s->log_xM);
}

// yN of a band pipeline: a power of two 2^lo .. 2^hi, or Q * 2^k within the range of the radix-Q pass
inline bool band_yN_supported(const Sizes& s, int lo, int hi) {
    int Q = 0, k = 0;
    if (s.log_yN >= 0) return s.log_yN >= lo && s.log_yN <= hi;
    return mixed_factor(s.yN, &Q, &k) && k >= kBandMinLog && k <= kBandMixedMaxLog;
}

// ---------------------------------------------------------------------------------------------------------
// pipeline-level features (swiftly_hip_supports): empty = supported, else the reason why not.  n_facets <= 0: not given.
inline std::string too_many_facets(int64_t n_facets) {
    if (n_facets <= kSumFinishMaxFacets) return {};
    return reason("the fused subgrid side sums at most %d facets in one kernel, got %lld", kSumFinishMaxFacets, (long long)n_facets);
}
// transform_contributions + sum_finish_facets
inline std::string why_not_fused_subgrid(const Sizes& s, int dtype, int64_t n_facets) {
    if (s.log_m < 0 || s.log_xM < 0)
        return reason("fused subgrid side: m %lld and xM %lld must be powers of two", (long long)s.m, (long long)s.xM);
    if (dtype != SWIFTLY_C64) return "fused subgrid side: complex64 only (complex128: the band pipeline, when asked for explicitly)";
    if (std::string why = too_many_facets(n_facets); !why.empty()) return why;
    if (s.log_m > kFusedMaxLogM || !sum_finish_supported(s.log_m, s.log_xM))
        return reason("fused subgrid side: no sum_finish instance for m %lld, xM %lld", (long long)s.m, (long long)s.xM);
    return {};
}
// group_finish + sum_finish_facets over the rows of its output (swiftly_hip_wave_group_finish_pieces): the forward subgrid
// side with the strided axis finished first.  The row kernel takes xM / m entries per off1 group, at most one group per facet
inline std::string why_not_group_finish(const Sizes& s, int dtype, int64_t n_facets) {
    if (std::string why = why_not_fused_subgrid(s, dtype, n_facets); !why.empty()) return why;
    if (!group_finish_supported(s.log_m, s.log_xM))
        return reason("group finish: no group_finish instance for m %lld, xM %lld", (long long)s.m, (long long)s.xM);
    if (n_facets * (s.xM / s.m) > kSumFinishMaxFacets)
        return reason("group finish: %lld facets x %lld row-kernel entries per group exceed %d", (long long)n_facets,
                      (long long)(s.xM / s.m), kSumFinishMaxFacets);
    return {};
}
// split_prepare_facets + wave_split_subgrids
inline std::string why_not_split_prepare(const Sizes& s, int dtype, int64_t n_facets) {
    if (dtype != SWIFTLY_C128) return why_not_fused_subgrid(s, dtype, n_facets);  // complex64: the pairs of sum_finish_facets
    if (s.log_m < 0 || s.log_xM < 0)
        return reason("split_prepare_facets: m %lld and xM %lld must be powers of two", (long long)s.m, (long long)s.xM);
    if (std::string why = too_many_facets(n_facets); !why.empty()) return why;
    if (!split_prepare_c128_supported(s.log_m, s.log_xM) || !col_pass_f64_supported(s.log_m))
        return reason("split_prepare_facets: complex128 instances exist for (m, xM) = %s; got (%lld, %lld)",
                      split_prepare_c128_sizes().c_str(), (long long)s.m, (long long)s.xM);
    return {};
}
// contiguous-axis-first forward kernels; `explicit_`: the caller asked for this pipeline (complex128 runs only then)
inline std::string why_not_band_pipeline(const Sizes& s, int dtype, int64_t n_facets, bool explicit_) {
    if (dtype == SWIFTLY_C128) {
        if (!explicit_) return "complex128 band pipeline: runs only when asked for explicitly";
        if (s.log_yN < 0 || s.log_xM < 0 || s.log_m < 0)
            return reason("complex128 band pipeline: yN %lld, xM %lld and m %lld must be powers of two", (long long)s.yN,
                          (long long)s.xM, (long long)s.m);
        if (std::string why = too_many_facets(n_facets); !why.empty()) return why;
        if (!band_pipeline_c128_supported(&s) || s.log_m < kBandMinLog)
            return reason("complex128 band pipeline: needs yN %d .. %d and an instance for (m, xM) = %s; got yN %lld, m %lld, xM %lld",
                          1 << kBandMinLog, 1 << kBandMaxLogYNC128, sum_finish_c128_sizes().c_str(), (long long)s.yN,
                          (long long)s.m, (long long)s.xM);
        return {};
    }
    if (std::string why = why_not_fused_subgrid(s, dtype, n_facets); !why.empty()) return why;
    if (s.log_m < kBandMinLog || !band_yN_supported(s, kBandMinLog, kBandMaxLogYN))
        return reason("band pipeline: needs m >= %d and yN a power of two %d .. %d or Q * 2^k (Q = 3, 5, 7, 9; 2^k %d .. %d); "
                      "got m %lld, yN %lld", 1 << kBandMinLog, 1 << kBandMinLog, 1 << kBandMaxLogYN, 1 << kBandMinLog,
                      1 << kBandMixedMaxLog, (long long)s.m, (long long)s.yN);
    return {};
}
// accumulate_facet_columns / finish_facet_band; `explicit_`: the caller asked for the band schedule (complex128 runs only
// then: nothing picks it on its own)
inline std::string why_not_backward_band(const Sizes& s, int dtype, bool explicit_ = false) {
    if (dtype == SWIFTLY_C128 && explicit_) {
        // the gather-sum column pass with 16-byte points: single passes of 64 .. 512 points, four-steps up to 32768; there
        // is no double radix-Q gather-sum pass, so no Q * 2^k
        if (s.log_xM < 0 || s.log_m < 0 || s.log_yN < kBackwardBandMinLogYN || s.log_yN > kBandMaxLogYNC128)
            return reason("complex128 backward band: needs xM and m powers of two and yN a power of two %d .. %d (no Q * 2^k: "
                          "there is no float64 radix-Q gather-sum pass); got xM %lld, m %lld, yN %lld",
                          1 << kBackwardBandMinLogYN, 1 << kBandMaxLogYNC128, (long long)s.xM, (long long)s.m, (long long)s.yN);
        return {};
    }
    if (dtype != SWIFTLY_C64) return "backward band: complex64 only (complex128: when asked for explicitly)";
    if (s.log_xM < 0 || s.log_m < 0 || !band_yN_supported(s, kBackwardBandMinLogYN, kBackwardBandMaxLogYN))
        return reason("backward band: needs xM and m powers of two and yN a power of two %d .. %d or Q * 2^k (Q = 3, 5, 7, 9; "
                      "2^k %d .. %d); got xM %lld, m %lld, yN %lld", 1 << kBackwardBandMinLogYN, 1 << kBackwardBandMaxLogYN,
                      1 << kBandMinLog, 1 << kBandMixedMaxLog, (long long)s.xM, (long long)s.m, (long long)s.yN);
    return {};
}
inline std::string why_not_split_band(const Sizes& s) {
    if (band_is_split(&s)) return {};
    return reason("yN %lld keeps the whole padded axis in the plain band layout (split: %d .. %d)", (long long)s.yN,
                  1 << kSplitBandMinLogYN, 1 << kSplitBandMaxLogYN);
}
// real-valued (float32) facets into the forward K1 (prepare_facet_band_real / prepare_facet_band_rows_real): the complex64 band
// pipeline with a power-of-two yN -- the row kernels of both band layouts have a real-load form, the radix-Q pass in front of
// the Q * 2^k lengths has none; float64 facets into complex128 are a feature of their own (why_not_real_facets_f64)
inline std::string why_not_real_facets(const Sizes& s, int dtype) {
    if (dtype == SWIFTLY_C128) return "real facets: complex64 output only (no float64 -> complex128 load in the complex128 row kernels)";
    if (dtype != SWIFTLY_C64) return reason("real facets: unknown dtype %d", dtype);
    if (std::string why = why_not_band_pipeline(s, SWIFTLY_C64, 0, false); !why.empty()) return "real facets: " + why;
    if (s.log_yN < 0) return reason("real facets: yN %lld is Q * 2^k: the radix-Q pass has no real load", (long long)s.yN);
    return {};
}
// real-valued (float32) facets out of the backward band pass (finish_facet_band_real): the complex64 backward band with a
// power-of-two yN -- the row kernels behind finish_facet_band have a real-store form, the radix-Q pass behind Q * 2^k and
// the Bluestein kernel have none; float64 facets out of complex128 are a feature of their own (why_not_real_facets_out_f64)
inline std::string why_not_real_facets_out(const Sizes& s, int dtype) {
    if (dtype == SWIFTLY_C128)
        return "real facet output: complex64 input only (no complex128 -> float64 store in the complex128 row kernels)";
    if (dtype != SWIFTLY_C64) return reason("real facet output: unknown dtype %d", dtype);
    if (std::string why = why_not_backward_band(s, SWIFTLY_C64); !why.empty()) return "real facet output: " + why;
    if (s.log_yN < 0) return reason("real facet output: yN %lld is Q * 2^k: the radix-Q pass has no real store", (long long)s.yN);
    return {};
}
// real-valued FLOAT64 facets into the complex128 forward K1 (prepare_facet_band_real64): the sizes of the complex128 band
// pipeline -- its row kernels (swiftly_rows.h up to 8192 points, pass A of swiftly_rowslong.h above) have a float64-load form
inline std::string why_not_real_facets_f64(const Sizes& s, int dtype) {
    if (dtype == SWIFTLY_C64)
        return "real facets, float64: complex128 output only (float32 facets into complex64: features 8 / 9, "
               "SWIFTLY_FEATURE_REAL_FACETS / SWIFTLY_FEATURE_REAL_FACETS_OUT)";
    if (dtype != SWIFTLY_C128) return reason("real facets, float64: unknown dtype %d", dtype);
    if (std::string why = why_not_band_pipeline(s, SWIFTLY_C128, 0, true); !why.empty()) return "real facets, float64: " + why;
    return {};
}
// real-valued FLOAT64 facets out of the complex128 backward band (finish_facet_band_real64): the sizes of the complex128
// backward band -- the row kernels behind its finish_facet_band (swiftly_rows.h, also as pass B of the long rows) have a
// float64-store form
inline std::string why_not_real_facets_out_f64(const Sizes& s, int dtype) {
    if (dtype == SWIFTLY_C64)
        return "real facet output, float64: complex128 input only (float32 facets out of complex64: features 8 / 9, "
               "SWIFTLY_FEATURE_REAL_FACETS / SWIFTLY_FEATURE_REAL_FACETS_OUT)";
    if (dtype != SWIFTLY_C128) return reason("real facet output, float64: unknown dtype %d", dtype);
    if (std::string why = why_not_backward_band(s, SWIFTLY_C128, true); !why.empty()) return "real facet output, float64: " + why;
    return {};
}
// real-valued facets through the half-length K1 (prepare_facet_band_rfft / prepare_facet_band_rows_rfft, swiftly_rowreal.h):
// the sizes of the real-load K1 at which the one-workgroup 16384-point form exists (the per-call conditions -- even facet
// size, position and row stride, an 8-byte-aligned input -- are the entry point's)
constexpr int kRealRfftLogYN = 15;
inline std::string why_not_real_facets_rfft(const Sizes& s, int dtype) {
    if (std::string why = why_not_real_facets(s, dtype); !why.empty()) return "real facets, half-length: " + why;
    if (s.log_yN != kRealRfftLogYN)
        return reason("real facets, half-length: needs yN %d; got yN %lld", 1 << kRealRfftLogYN, (long long)s.yN);
    return {};
}
// real-valued facets out of the backward band pass through the half-length B8 (finish_facet_band_c2r, swiftly_rowc2r.h): the
// sizes of the real-store B8 at which the one-workgroup 16384-point form exists (the per-call conditions -- even facet size,
// position and output row stride, an 8-byte-aligned output -- are the entry point's)
constexpr int kRealOutC2RLogYN = 15;
inline std::string why_not_real_facets_out_c2r(const Sizes& s, int dtype) {
    if (std::string why = why_not_real_facets_out(s, dtype); !why.empty()) return "real facets out, half-length: " + why;
    if (s.log_yN != kRealOutC2RLogYN)
        return reason("real facets out, half-length: needs yN %d; got yN %lld", 1 << kRealOutC2RLogYN, (long long)s.yN);
    return {};
}
// the same two forms on 65536-point rows (one 32768-point transform, 1024 threads x 32 points: RowRealGeo64k / RowC2RGeo64k):
// features of their own, SWIFTLY_FEATURE_REAL_FACETS_RFFT_64K / _OUT_C2R_64K, so that the two above answer as they always
// did.  The entry points take a handle either feature of their pair supports and name both lengths when neither does.
constexpr int kRealRfftLogYN64k = 16;
inline std::string why_not_real_facets_rfft_64k(const Sizes& s, int dtype) {
    if (std::string why = why_not_real_facets(s, dtype); !why.empty()) return "real facets, half-length: " + why;
    if (s.log_yN != kRealRfftLogYN64k)
        return reason("real facets, half-length: needs yN %d; got yN %lld", 1 << kRealRfftLogYN64k, (long long)s.yN);
    return {};
}
constexpr int kRealOutC2RLogYN64k = 16;
inline std::string why_not_real_facets_out_c2r_64k(const Sizes& s, int dtype) {
    if (std::string why = why_not_real_facets_out(s, dtype); !why.empty()) return "real facets out, half-length: " + why;
    if (s.log_yN != kRealOutC2RLogYN64k)
        return reason("real facets out, half-length: needs yN %d; got yN %lld", 1 << kRealOutC2RLogYN64k, (long long)s.yN);
    return {};
}
// what the entry points of the half-length forms refuse through: feature 12 or 16 (13 or 17)
inline std::string why_not_half_length_k1(const Sizes& s, int dtype) {
    if (why_not_real_facets_rfft(s, dtype).empty() || why_not_real_facets_rfft_64k(s, dtype).empty()) return {};
    if (std::string why = why_not_real_facets(s, dtype); !why.empty()) return "real facets, half-length: " + why;
    return reason("real facets, half-length: needs yN %d or %d; got yN %lld", 1 << kRealRfftLogYN, 1 << kRealRfftLogYN64k, (long long)s.yN);
}
inline std::string why_not_half_length_finish(const Sizes& s, int dtype) {
    if (why_not_real_facets_out_c2r(s, dtype).empty() || why_not_real_facets_out_c2r_64k(s, dtype).empty()) return {};
    if (std::string why = why_not_real_facets_out(s, dtype); !why.empty()) return "real facets out, half-length: " + why;
    return reason("real facets out, half-length: needs yN %d or %d; got yN %lld", 1 << kRealOutC2RLogYN, 1 << kRealOutC2RLogYN64k,
                  (long long)s.yN);
}
// size part of prepare_facet_window_rows (the band, the facets and the windows are per call)
inline std::string why_not_window_rows(const Sizes& s) {
    if (s.log_yN == kWindowRowsLogYN && s.log_m == kWindowRowsLogM && s.xM <= (int64_t(1) << kPlacedMaxLogXM)) return {};
    return reason("window rows: needs yN %d, m %d and xM <= %d; got yN %lld, m %lld, xM %lld", 1 << kWindowRowsLogYN,
                  1 << kWindowRowsLogM, 1 << kPlacedMaxLogXM, (long long)s.yN, (long long)s.m, (long long)s.xM);
}
// prepare_facet_columns_axis1 (K2 with the contiguous-axis finish inside pass A' of its four-step, swiftly_colaxis1.h):
// complex64, the parity-split band layout, an instance of pass A' for (yN, m) -- n1 = 16384 / m rows of the window in LDS
// and a pass B of n2 = yN / n1 <= 1024 points -- a sum_finish pair for (m, xM), and the placed sum_finish_facets behind it
#define CA1_PAIRS(X) X(15, 9) X(14, 8)  // (log2 yN, log2 m) instances of col_axis1.hip
inline bool col_axis1_instance(int log_yN, int logm) {
#define CA1_HAS(L, M) \
    if (log_yN == L && logm == M) return true;
    CA1_PAIRS(CA1_HAS)
#undef CA1_HAS
    return false;
}
inline std::string why_not_axis1_columns(const Sizes& s, int dtype) {
    const auto got = [&] { return reason("; got yN %lld, m %lld, xM %lld", (long long)s.yN, (long long)s.m, (long long)s.xM); };
    if (dtype != SWIFTLY_C64) return "axis-1 columns: complex64 only" + got();
    if (!band_is_split(&s))
        return reason("axis-1 columns: needs the parity-split band layout (yN %d .. %d)", 1 << kSplitBandMinLogYN,
                      1 << kSplitBandMaxLogYN) + got();
    if (!col_axis1_instance(s.log_yN, s.log_m)) {
        std::string have;
#define CA1_NAME(L, M) have += (have.empty() ? "(" : ", (") + std::to_string(1 << L) + ", " + std::to_string(1 << M) + ")";
        CA1_PAIRS(CA1_NAME)
#undef CA1_NAME
        return "axis-1 columns: instances exist for (yN, m) = " + have + got();
    }
    if (s.log_xM < 0 || !sum_finish_supported(s.log_m, s.log_xM) || s.log_xM > kPlacedMaxLogXM)
        return reason("axis-1 columns: needs a sum_finish instance for (m, xM) with xM <= %d (the placed mode)", 1 << kPlacedMaxLogXM) +
               got();
    return {};
}
// size part of prepare_facet_window_rows_real (float32 rows into the whole-row K1; dtype = the output type): the sizes both
// the window rows and the real-load K1 exist for
inline std::string why_not_real_window_rows(const Sizes& s, int dtype) {
    if (std::string why = why_not_real_facets(s, dtype); !why.empty()) return "real window rows: " + why;
    if (std::string why = why_not_window_rows(s); !why.empty()) return "real window rows: " + why;
    return {};
}

}  // namespace swf
