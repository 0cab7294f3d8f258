// Internals shared by the translation units of the C ABI (swiftly_abi.hip: handles + the eight primitives and their
// batch forms; swiftly_abi_coltransform.hip: the strided-axis transform, col_transform; swiftly_abi_pipeline.hip: the
// fused / per-wave entry points of the streaming classes; swiftly_abi_util.hip: device memory, stream and diagnostic
// helpers, and the table of kernels launched with dynamic LDS (swiftly_launch.h), whose per-device attributes
// swiftly_hip_create sets from it; swiftly_abi_sources.hip: point-source truths and RMSE checks).  Two headers of pure host
// functions of the sizes stand beside it: swiftly_caps.h (which kernels and pipelines exist) and swiftly_geometry.h (how an
// offset becomes the integers of an index map); the launch sequences ask them and restate neither.  Not installed:
// include/swiftly_hip.h is the public header.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <atomic>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/swiftly_hip.h"
#include "swiftly_colpass.h"
#include "swiftly_geometry.h"
#include "swiftly_launch.h"
#include "swiftly_rowpass.h"
#include "swiftly_rowreal.h"
#include "swiftly_rowc2r.h"
#include "swiftly_sumfinish.h"
#include "swiftly_rows.h"
#include "swiftly_rowslong.h"
#include "swiftly_bluestein.h"
#include "swiftly_mixed.h"
#include <complex>

using namespace swf;

static_assert(kFusedMaxLogM == kColPassMaxLog && kBackwardBandMinLogYN >= kColPassMinLog && kBackwardBandMinLogYN >= kMinLogN &&
                  kBackwardBandMaxLogYN <= kMaxLogNFloat + 1,
              "swiftly_caps.h names the column-pass limits; the backward band stays inside the twiddle tables of make_twiddles");
// complex128 backward band: four-step twiddles from the double tables of make_twiddles (up to 2^(kMaxLogNFloat + 1)), gather-sum
// passes of at most 2^kColPassMaxLogF64 points (single pass, and both halves of the longest four-step), finish_facet_band
// through the complex128 row kernels (run_rows_long up to 2^kMaxLogNDoubleRows)
static_assert(kBandMaxLogYNC128 <= kMaxLogNFloat + 1 && kBandMaxLogYNC128 <= kMaxLogNDoubleRows &&
                  (kBandMaxLogYNC128 + 1) / 2 <= kColPassMaxLogF64 && kBackwardBandMinLogYN >= 6,
              "the complex128 backward band stays inside the double twiddle tables, the complex128 column passes and the long-row kernels");

// ---------------------------------------------------------------------------
// error state: integer status + thread-local message (swiftly_hip_last_error)
int fail(int code, const char* fmt, ...);
#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) return fail(SWIFTLY_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
// Status of a kernel launcher's return value `e` (a hipError_t, or negative: no instance): 0, or SWIFTLY_ERR_HIP and the
// message "...[ (what)]: <error>".  `negative`: the text for e < 0 ("no instance"), else hipGetErrorString takes every value.
int launch_status(int e, const char* what = nullptr, const char* negative = nullptr);
int radix_launch_status(int e, int Q, const char* pass = "pass");  // what = "radix-<Q> <pass>"

// Scratch of one call: the caller's workspace when it is big enough, else a stream-ordered allocation that release()
// frees on the same stream.  No destructor: a path that forgets release() leaks visibly instead of queueing a hidden free.
struct ScratchLease {
    void* p = nullptr; bool own = false; hipStream_t st = nullptr;
    int acquire(void* ws, size_t ws_bytes, size_t need, hipStream_t stream, const char* what) {  // error: "<what>: <hip error>"
        own = !(ws && ws_bytes >= need);
        st = stream;
        p = ws;
        if (!own) return 0;
        const hipError_t e = hipMallocAsync(&p, need, st);
        if (e == hipSuccess) return 0;
        own = false;
        return fail(SWIFTLY_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    }
    int release(int rc) {  // `rc`: the status of the work on the scratch; a failed free is reported only when that was 0
        const hipError_t e = own ? hipFreeAsync(p, st) : hipSuccess;
        own = false;
        return (!rc && e != hipSuccess) ? fail(SWIFTLY_ERR_HIP, "hipFreeAsync: %s", hipGetErrorString(e)) : rc;
    }
};

struct swiftly_hip : Sizes {  // N, yN, xM, m and log_yN, log_xM, log_m (swiftly_caps.h)
    double W;
    int device;
    int cu_count = 0;  // compute units of `device` (swiftly_hip_create): the grid of the persistent kernels
    float* invp_f = nullptr;    // 1/pswf[k] (k = 0 -> 0)
    double* invp_d = nullptr;
    float* fn_f = nullptr;  // Fn[k], k < m
    double* fn_d = nullptr;
    std::map<int, cx<float>*> tw_f;  // by log2(length)
    std::map<int, cx<double>*> tw_d;
    // compact copies of the float tables (swiftly_fft.h, "compact twiddle sections") by (log2(length), log2(points per lane))
    std::map<std::pair<int, int>, cx<float>*> twc_f;
    // Bluestein tables for transform lengths that are not a power of two (swiftly_bluestein.h), by length
    struct Blu {
        int logL = 0;
        cx<float>* chirp_f = nullptr;
        cx<float>* spec_f = nullptr;
        cx<double>* chirp_d = nullptr;
        cx<double>* spec_d = nullptr;
    };
    std::map<int64_t, Blu> blu;
    // lengths n = Q * 2^k, Q in {3, 5, 7, 9} (swiftly_mixed.h): exp(-2 pi i r / n), r < n
    struct Mixed {
        int Q = 0, logM = 0;
        cx<float>* tw_f = nullptr;
        cx<double>* tw_d = nullptr;
    };
    std::map<int64_t, Mixed> mixed;
    std::vector<void*> allocs;
    // float64 arithmetic in the column passes of the band pipelines (K2, K3 and their backward mirrors; complex64 data):
    // 0 (default: float32 arithmetic everywhere) | 1 (swiftly_hip_set_column_precision, env SWIFTLY_COL_F64)
    int col_f64 = 0;
    // which of the column-pass stages compute in float64 when col_f64 is set (SWIFTLY_COL_F64_STAGES, default 7 = all; for
    // the measured error / cost table of DESIGN.md section 2): 1 = pass A of a four-step, 2 = pass B, 4 = single-pass
    // transforms (K3 and its backward mirror)
    int col_f64_stages = 7;
    // two internal streams of the chunked four-step (col_transform): created on first use, under `chunk_mu` (the fork /
    // join events are per call: two host threads may drive one handle on different streams)
    hipStream_t chunk_st[2] = {nullptr, nullptr};
    std::mutex chunk_mu;
    // the caller's four-step workspace was last used by the UN-chunked path (on the caller's stream): the next chunked call
    // must fork its chunk streams behind that stream even when swiftly_hip_chain_chunk_streams is set (r5 advisor: a trailing
    // facet group below the chunk threshold, > 32 facets)
    std::atomic<void*> ws_plain_pending{nullptr};  // that workspace
    // re-laid-out load windows of the forward K1 (swiftly_rowpass.h), built on first use per facet offset
    Win4Cache win4;
};

// The radix-Q descriptor of a length n = Q * 2^k (swiftly_mixed.h); the caller adds `scratch` and the s_* strides of its layout.
template <typename R>
inline MixedArgs<R> mixed_args(const swiftly_hip::Mixed& mx, int64_t n) {
    MixedArgs<R> X;
    std::memset(&X, 0, sizeof X);
    X.Q = mx.Q; X.M = (int)(1ll << mx.logM); X.n = (int)n;
    for (int r = 0; r < mx.Q; r++) {
        const long double ang = -2.0L * 3.14159265358979323846264338327950288L * (long double)r / (long double)mx.Q;
        X.wq[r] = cx<R>{(R)cosl(ang), (R)sinl(ang)};
    }
    if constexpr (sizeof(R) == 4) X.tw_n = mx.tw_f; else X.tw_n = mx.tw_d;
    return X;
}
// Workspace of the band entry points at such a length: [radix-Q scratch: nf * yN * m][sub-transform scratch: nf * M * m, + 4096]
struct MixedWorkspace {
    size_t radix_bytes, sub_bytes;
    MixedWorkspace(int nf, int yN, long long M, int m)
        : radix_bytes((size_t)nf * (size_t)yN * (size_t)m * sizeof(cx<float>)),
          sub_bytes((size_t)nf * (size_t)M * (size_t)m * sizeof(cx<float>) + 4096) {}
    size_t bytes() const { return radix_bytes + sub_bytes; }
    char* sub(void* base) const { return (char*)base + radix_bytes; }
};

// swiftly_hip_chain_chunk_streams (include/swiftly_hip.h): the calling thread's chunked four-step launches skip their fork
extern thread_local int g_chain_chunk_streams;

template <typename R>
inline const cx<R>* twiddles(const swiftly_hip* h, int logn);
template <>
inline const cx<float>* twiddles<float>(const swiftly_hip* h, int logn) {
    auto it = h->tw_f.find(logn);
    return it == h->tw_f.end() ? nullptr : it->second;
}
template <>
inline const cx<double>* twiddles<double>(const swiftly_hip* h, int logn) {
    auto it = h->tw_d.find(logn);
    return it == h->tw_d.end() ? nullptr : it->second;
}
inline const cx<float>* compact_twiddles(const swiftly_hip* h, int logn, int logp) {
    auto it = h->twc_f.find({logn, logp});
    return it == h->twc_f.end() ? nullptr : it->second;
}
template <typename R>
inline const R* invp(const swiftly_hip* h);
template <>
inline const float* invp<float>(const swiftly_hip* h) { return h->invp_f; }
template <>
inline const double* invp<double>(const swiftly_hip* h) { return h->invp_d; }
template <typename R>
inline const R* fnwin(const swiftly_hip* h);
template <>
inline const float* fnwin<float>(const swiftly_hip* h) { return h->fn_f; }
template <>
inline const double* fnwin<double>(const swiftly_hip* h) { return h->fn_d; }
// RAII: make `device` current for the duration of one ABI call and restore the caller's (torch's) current
// device afterwards.  Streams handed in by the caller belong to the handle's device.
struct DeviceGuard {
    int prev = -1, rc = 0;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) rc = (int)hipSetDevice(device);
        else prev = -1;  // nothing to restore
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};
// (kTwoPassMinLog, where a strided-axis transform becomes a four-step: swiftly_rowroute.h)

// element k of a complex array of either storage type (complex128 arrays travel through the cx<float> pointers of the
// column-pass and sum_finish argument blocks)
static inline const cx<float>* cx_at(const void* p, int64_t k, bool c128) {
    return (const cx<float>*)((const char*)p + k * (int64_t)(c128 ? sizeof(cx<double>) : sizeof(cx<float>)));
}
static inline cx<float>* cx_at(void* p, int64_t k, bool c128) {
    return (cx<float>*)((char*)p + k * (int64_t)(c128 ? sizeof(cx<double>) : sizeof(cx<float>)));
}
// column-tile passes (swiftly_abi_coltransform.hip)
ColZ plain_colz();
// single-pass launch of length 2^logn: float64 arithmetic when the handle asks for it and the instance exists; complex128
// storage always takes that instance
inline int set_col_precision(const swiftly_hip* h, ColPassArgs& c, int logn, bool c128) {
    const cx<double>* t = twiddles<double>(h, logn);
    if (c128 && !t) return fail(SWIFTLY_ERR_HIP, "internal: missing twiddle table");
    c.c128 = c128 ? 1 : 0;
    c.f64 = t && (c128 || (h->col_f64 && (h->col_f64_stages & 4) && col_pass_f64_supported(logn) && !c.gs)) ? 1 : 0;
    if (c.f64) c.twd = c.twd_full = t;
    return 0;
}
// a map of swiftly_geometry.h with its windows, for the row kernels
template <typename R>
inline AxisMap<R> axis_map(const Map& g, const R* win = nullptr, const R* win2 = nullptr) {
    return AxisMap<R>{g.a, g.len, g.c, g.mod, win, win2};
}
// the argument block of a plain (un-decomposed) column pass: everything zero but the unit multipliers and the two maps
inline ColPassArgs col_pass_args(const Map& ld, const Map& st) {
    ColPassArgs c;
    std::memset(&c, 0, sizeof c);
    c.ld_mul = c.st_mul = 1;
    c.ld_a = ld.a; c.ld_len = ld.len; c.ld_c = ld.c; c.ld_mod = ld.mod;
    c.st_a = st.a; c.st_len = st.len; c.st_c = st.c; c.st_mod = st.mod;
    return c;
}
int launch_col_checked(int lg, int mode, const ColPassArgs& args, const ColZ& cz, int outer, int nb, hipStream_t st,
                       const ColPassSrc2* src2 = nullptr);
// scratch handed down by an entry point for the duration of one ABI call on this host thread (see col_transform)
extern thread_local void* t_call_ws;
extern thread_local size_t t_call_ws_bytes;
struct CallWorkspace {
    CallWorkspace(void* p, size_t bytes) { t_call_ws = p; t_call_ws_bytes = p ? bytes : 0; }
    ~CallWorkspace() { t_call_ws = nullptr; t_call_ws_bytes = 0; }
};
int col_transform(swiftly_hip* h, int logn, const ColPassArgs& c, const ColZ& cz, int W, int nb, hipStream_t st,
                  void* ws = nullptr, size_t ws_bytes = 0, int qmul = 0, int qadd = 0, int full_n = 0);
// the same transform with the contiguous-axis finish inside its first pass (swiftly_colaxis1.h; swiftly_abi_coltransform.hip)
namespace swf { struct ColAxis1Args; }
int col_transform_axis1(swiftly_hip* h, const ColPassArgs& c, const ColZ& cz, swf::ColAxis1Args x, int nb, hipStream_t st,
                        void* ws, size_t ws_bytes);

// Facet tables of the row-wise fused kernels (swiftly_sumfinish.h), grouped by off1: entries of one group are adjacent.
template <class Args>
static inline void fill_facet_groups(Args& a, const swiftly_hip* h, int64_t nfacets, const int64_t* facet_off0s,
                                     const int64_t* facet_off1s) {
    std::vector<int> order((size_t)nfacets);
    for (int f = 0; f < nfacets; f++) order[(size_t)f] = f;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return facet_off1s[x] < facet_off1s[y]; });
    a.ngroups = 0;
    for (int n = 0; n < nfacets; n++) {
        const int f = order[(size_t)n];
        if (n == 0 || facet_off1s[f] != facet_off1s[order[(size_t)n - 1]]) {
            a.gstart[a.ngroups] = n;
            a.gsp1[a.ngroups] = (int)facet_shift(*h, facet_off1s[f]);
            a.ngroups++;
        }
        a.fidx[n] = f;
        a.base0[n] = contribution_in_padded_subgrid(*h, facet_off0s[f]).c;  // first padded-subgrid row the facet contributes to
    }
    a.gstart[a.ngroups] = (int)nfacets;
}

// Rounds of the wave-parallel sum_finish_facets (SFWide): groups whose placement windows [start, start + m) on the ring
// of xM positions are mutually disjoint share a round (greedy, in group order: deterministic).
static inline void fill_group_rounds(SumFinishFacetArgs& a, const swiftly_hip* h) {
    const int xM = (int)h->xM, m = (int)h->m;
    std::vector<std::vector<int>> rounds;
    auto overlap = [&](int g1, int g2) {
        const int d = pmod(placement_start(*h, a.gsp1[g2]) - placement_start(*h, a.gsp1[g1]), xM);
        return d < m || xM - d < m;
    };
    for (int g = 0; g < a.ngroups; g++) {
        size_t r = 0;
        for (; r < rounds.size(); r++) {
            bool ok = true;
            for (int o : rounds[r]) ok = ok && !overlap(g, o);
            if (ok) break;
        }
        if (r == rounds.size()) rounds.emplace_back();
        rounds[r].push_back(g);
    }
    a.nrounds = (int)rounds.size();
    int k = 0;
    for (size_t r = 0; r < rounds.size(); r++) {
        a.rstart[r] = k;
        for (int g : rounds[r]) a.rgroup[k++] = g;
    }
    a.rstart[rounds.size()] = k;
}

// The Fn, twiddle and compact twiddle tables of an argument block of the sum_finish family (swiftly_sumfinish.h), through
// pointers to the fields the block has (null: it has none, or its instances read none).  complex128: the double Fn and
// plain double twiddle tables, behind the float pointer types; the compact copies exist in float only.  m-point
// transforms run 64 lanes each, rows 64 lanes and 256 from 4096 points on.
static inline int fill_sum_finish_tables(const swiftly_hip* h, bool c128, const float** fn, const cx<float>** tw_m,
                                         const cx<float>** tw_x, const cx<float>** twc_m, const cx<float>** twc_x) {
    *fn = c128 ? (const float*)h->fn_d : h->fn_f;
    *tw_m = c128 ? (const cx<float>*)twiddles<double>(h, h->log_m) : twiddles<float>(h, h->log_m);
    if (tw_x) *tw_x = c128 ? (const cx<float>*)twiddles<double>(h, h->log_xM) : twiddles<float>(h, h->log_xM);
    if (!*fn || !*tw_m || (tw_x && !*tw_x))
        return fail(SWIFTLY_ERR_HIP, c128 ? "internal: missing double tables" : "internal: missing twiddle tables");
    if (twc_m) *twc_m = compact_twiddles(h, h->log_m, h->log_m - 6);
    if (twc_x) *twc_x = compact_twiddles(h, h->log_xM, h->log_xM - (h->log_xM >= 12 ? 8 : 6));
    if ((twc_m && !*twc_m) || (twc_x && !*twc_x)) return fail(SWIFTLY_ERR_HIP, "internal: missing compact twiddle tables");
    return 0;
}

#define CHECK_DTYPE() \
    if (dtype != SWIFTLY_C64 && dtype != SWIFTLY_C128) return fail(SWIFTLY_ERR_PARAM, "bad dtype %d", dtype);
#define CHECK_COMMON()                                                                       \
    if (!h || !in || !out) return fail(SWIFTLY_ERR_PARAM, "null argument");                  \
    DeviceGuard device_guard_(h->device);                                                    \
    if (device_guard_.rc) return fail(SWIFTLY_ERR_HIP, "hipSetDevice(%d) failed", h->device); \
    if (rows < 0) return fail(SWIFTLY_ERR_PARAM, "negative row count");                      \
    CHECK_DTYPE()                                                                            \
    if (in_cs < 0 || out_cs < 0 || in_cs >= (int64_t(1) << 32) || out_cs >= (int64_t(1) << 32)) \
        return fail(SWIFTLY_ERR_PARAM, "column strides must be in [0, 2^32)");                 \
    if (rows > 0x7fffffff) return fail(SWIFTLY_ERR_PARAM, "too many rows");
#define CHECK_BATCH()                                                                        \
    if (nbatch < 0 || in_bs < 0 || out_bs < 0) return fail(SWIFTLY_ERR_PARAM, "bad batch description");
// The accumulating entry points read-modify-write their output non-atomically and run the batch items
// concurrently: items that share output elements would lose updates.
#define CHECK_ACCUMULATE_BATCH()                                                             \
    if (nbatch > 1 && out_bs == 0)                                                           \
        return fail(SWIFTLY_ERR_PARAM, "accumulating batch items must not share output elements (out_batch_stride = 0)");

#define DISPATCH(fn, ...) (dtype == SWIFTLY_C64 ? fn<float>(__VA_ARGS__) : fn<double>(__VA_ARGS__))
#define CHECK_FACET_SIZE()                                                                                     \
    if (facet_size <= 0 || facet_size >= h->yN)                                                                \
        return fail(SWIFTLY_ERR_PARAM, "facet size %lld must be in [1, yN_size - 1 = %lld]", (long long)facet_size, \
                    (long long)(h->yN - 1));
#define CHECK_SUBGRID_SIZE()                                                                                      \
    if (subgrid_size <= 0 || subgrid_size > h->xM)                                                                \
        return fail(SWIFTLY_ERR_PARAM, "subgrid size %lld must be in [1, xM_size = %lld]", (long long)subgrid_size, \
                    (long long)h->xM);
// (band_start, band_len) of the call is a cyclic range of the padded facet axis (band_valid, swiftly_geometry.h)
#define CHECK_BAND()                                                                                              \
    if (!band_valid(h->yN, band_start, band_len))                                                                 \
        return fail(SWIFTLY_ERR_PARAM, "band [%lld, +%lld) is not a cyclic range of [0, %lld)", (long long)band_start, \
                    (long long)band_len, (long long)h->yN);
// every element offset inside one batch item fits 32 bits (offsets_fit_32, swiftly_geometry.h)
#define CHECK_OFFSETS_32(fit) \
    if (!(fit)) return fail(SWIFTLY_ERR_PARAM, "strides too large for 32-bit offsets");

// ---------------------------------------------------------------------------------------------------------
// band buffers of the contiguous-axis-first pipeline
// half of a parity-split band buffer, in columns: a multiple of 16 (128 bytes) so that BOTH parity runs of a 64-column
// tile of the column pass start on a cache line (r2: (band_len + 1) / 2 = 5736 left every odd run 64 bytes off a line:
// 5 lines fetched per 4 lines' worth, FETCH_SIZE of K2 pass A 1.04 GB per wave against 0.83 GB)
static inline int64_t band_half_columns(int64_t band_len) { return (((band_len + 1) / 2) + 15) & ~int64_t(15); }
// (half = 0 in the plain band layout: band_is_split, swiftly_caps.h)
static inline int band_half_of(const swiftly_hip* h, int64_t band_len) {
    return band_is_split(h) ? (int)band_half_columns(band_len) : 0;
}
