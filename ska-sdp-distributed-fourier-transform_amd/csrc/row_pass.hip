// instantiations + dispatch of the lean long-row kernel (complex64)
#include <cstdlib>

#include "swiftly_launch.h"
#include "swiftly_rowinst.h"
#include "swiftly_rowpass.h"

namespace swf {

#if SWF_TRACE
__device__ unsigned long long swf_trace_buf[kTraceBlocks * kTracePoints];
extern "C" int swiftly_hip_trace_fetch(void* host, size_t bytes) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(swf_trace_buf), bytes);
}
#endif

template <int LOGN>
struct RGeoFor {
    // 1024 threads, 8 / 16 / 32 points per thread; N = 32768 needs the split re/im exchange
    using type = RGeo<LOGN, LOGN - 10, (LOGN >= 14)>;  // split from 16384: 64 KB LDS -> 2 workgroups per CU
};

template <int LOGN, int MODE, bool REAL = false, bool REAL_ST = false>
static int launch_mode(const RowPassArgs& a, hipStream_t s) {
    using G = typename RGeoFor<LOGN>::type;
    return launch_lds<row_pass_kernel<G, MODE, REAL, REAL_ST>, G::LDS_BYTES>(dim3((unsigned)a.nrows), dim3(G::NT), s, a, a.in, a.out,
                                                                             a.ld_win, a.st_win, a.st_win2, a.tw);
}
template <int LOGN>
static int launch_one(int mode, const RowPassArgs& a, hipStream_t s) {
    if (mode == 0) return launch_mode<LOGN, 0>(a, s);
    if (mode == 1) return launch_mode<LOGN, 1>(a, s);
    return launch_mode<LOGN, 2>(a, s);
}

int launch_row_pass(int logn, int mode, const RowPassArgs& a, hipStream_t s) {
    if (a.nrows <= 0) return 0;
    switch (choose_lean_form(logn, mode, a.in_real, a.out_real, a.accumulate)) {  // swiftly_rowinst.h: which forms exist
        case kLeanRealLoad: return launch_mode<13, 0, true>(a, s);
        case kLeanRealStore:
            if (logn == 13) return mode == 1 ? launch_mode<13, 1, false, true>(a, s) : launch_mode<13, 2, false, true>(a, s);
            return mode == 1 ? launch_mode<14, 1, false, true>(a, s) : launch_mode<14, 2, false, true>(a, s);
        case kLeanComplex:
            if (logn == 13) return launch_one<13>(mode, a, s);
            if (logn == 14) return launch_one<14>(mode, a, s);
            return launch_one<15>(mode, a, s);
        default: return -1;
    }
}
template <class G, int LOGS>
static int launch_split(const RowPassArgs& a, const cx<float>* tw_part, const cx<float>* tw_full, hipStream_t s) {
    const unsigned blocks = (unsigned)(((a.nrows + 7) / 8) * (8 << LOGS));
    if (a.ld_win)
        return launch_lds<row_pass_split_kernel<G, LOGS, true>, G::LDS_BYTES>(dim3(blocks), dim3(G::NT), s, a, a.in, a.out,
                                                                              a.ld_win, tw_part, tw_full);
    return launch_lds<row_pass_split_kernel<G, LOGS, false>, G::LDS_BYTES>(dim3(blocks), dim3(G::NT), s, a, a.in, a.out, a.ld_win,
                                                                           tw_part, tw_full);
}
using SplitGeo2 = RGeo<14, 4, true>;   // 2 x 16384 points, 1024 threads x 16 (one workgroup per CU)
// (4 x 8192 points in 512-thread workgroups and the interleaved-exchange forms were measured slower in r1-r2)
int launch_row_pass_split(const RowPassArgs& a, const cx<float>* tw14, const cx<float>* tw13, const cx<float>* tw_full,
                          hipStream_t s) {
    (void)tw13;
    if (a.nrows <= 0) return 0;
    return launch_split<SplitGeo2, 1>(a, tw14, tw_full, s);
}
// -- the band row kernel: 2 x 2^(logn-1) points, two workgroups per row ---------------------------------------------
// geometries (BandGeoId of swiftly_rowinst.h names them)
using BandGeo16k = RGeo<13, 4, true>;       // yN = 16384: 2 x  8192 points,  512 threads x 16, 33 KB LDS
using BandGeo4 = RGeo<14, 4, true>;         // yN = 32768: 2 x 16384 points, 1024 threads x 16, one workgroup per CU
using BandGeo5 = RGeo<14, 5, true>;         // yN = 32768: 2 x 16384 points,  512 threads x 32, 66 KB LDS: two workgroups per CU
using BandGeo5Pre = RGeoPre<14, 5, true>;   // ... with the twiddle preload (forward K1)
using BandGeo5PreC = RGeoPreC<14, 5, true>; // ... from the compact twiddle sections (forward K1 with the window table)
using BandGeo5C = RGeoC<14, 5, true>;       // ... compact sections without the preload (backward finish)
using BandGeo64k = RGeo<15, 5, true>;       // yN = 65536: 2 x 32768 points, 1024 threads x 32, 132 KB LDS, one workgroup per CU

// Every instance of row_pass_band_kernel that exists: X(geometry, WIN, ST, PAIR, NSEG, CJ, W4, REAL, REAL_ST).  Which one
// a call runs: choose_band_instance (swiftly_rowinst.h); tests/test_band_instances_cpu.py holds this list against it.
// ST: 0 plain store, 1 band store, 2 mapped store (no load window).  REAL 1: real rows; 2: through 4-byte loads (PAIR only).
#define SWF_BAND_INSTANCES(X)                                                                                          \
    /* 16384-point rows: one geometry for every form */                                                                \
    X(BandGeo16k, 0, 0, 0, 0, -1, 0, 0, 0)                                                                             \
    X(BandGeo16k, 0, 1, 0, 0, -1, 0, 0, 0)                                                                             \
    X(BandGeo16k, 0, 2, 0, 0, -1, 0, 0, 0)                                                                             \
    X(BandGeo16k, 1, 0, 0, 0, -1, 0, 0, 0)                                                                             \
    X(BandGeo16k, 1, 1, 0, 0, -1, 0, 0, 0)                                                                             \
    X(BandGeo16k, 1, 1, 0, 0, -1, 0, 1, 0)                                                                             \
    /* 32768-point rows, plain store: 1024 x 16 -- the 512-thread form spills ~49 VGPRs here */                        \
    X(BandGeo4, 0, 0, 0, 0, -1, 0, 0, 0)                                                                               \
    X(BandGeo4, 1, 0, 0, 0, -1, 0, 0, 0)                                                                               \
    /* 32768-point rows, band and mapped store: 512 x 32, two workgroups per CU (1024 x 16 for the band store: */      \
    /* 1.95 against 1.73 ms per facet, r4); without and with adjacent-point loads */                                   \
    X(BandGeo5, 0, 1, 0, 0, -1, 0, 0, 0)                                                                               \
    X(BandGeo5, 1, 1, 0, 0, -1, 0, 0, 0)                                                                               \
    X(BandGeo5, 1, 1, 0, 0, -1, 0, 1, 0)                                                                               \
    X(BandGeo5, 0, 2, 0, 0, -1, 0, 0, 0)                                                                               \
    X(BandGeo5, 0, 2, 0, 0, -1, 0, 0, 1)                                                                               \
    X(BandGeo5, 0, 1, 1, 0, -1, 0, 0, 0)                                                                               \
    X(BandGeo5, 1, 1, 1, 0, -1, 0, 0, 0)                                                                               \
    X(BandGeo5, 1, 1, 1, 0, -1, 0, 1, 0)                                                                               \
    X(BandGeo5, 1, 1, 1, 0, -1, 0, 2, 0)                                                                               \
    X(BandGeo5, 0, 2, 1, 0, -1, 0, 0, 0)                                                                               \
    X(BandGeo5, 0, 2, 1, 0, -1, 0, 0, 1)                                                                               \
    /* backward finish with its empty segments compiled out: the band is 11488 of 32768 columns, 12 segments, 13 at */ \
    /* an unaligned position; 16 for wider bands.  Plain geometry: at 128 VGPRs the preload does not gain */          \
    X(BandGeo5, 0, 2, 1, 13, 0, 0, 0, 0)                                                                               \
    X(BandGeo5, 0, 2, 1, 13, 0, 0, 0, 1)                                                                               \
    X(BandGeo5, 0, 2, 1, 16, 0, 0, 0, 0)                                                                               \
    X(BandGeo5, 0, 2, 1, 16, 0, 0, 0, 1)                                                                               \
    X(BandGeo5C, 0, 2, 1, 13, 0, 0, 0, 0)                                                                              \
    X(BandGeo5C, 0, 2, 1, 13, 0, 0, 0, 1)                                                                              \
    X(BandGeo5C, 0, 2, 1, 16, 0, 0, 0, 0)                                                                              \
    X(BandGeo5C, 0, 2, 1, 16, 0, 0, 0, 1)                                                                              \
    /* forward K1 with its empty segments compiled out: 16 (a 16384-point facet), 22 (the 22528 points of the 64k */   \
    /* workload at a segment boundary) and 24 (the same facet anywhere, and 24576 points) of 32 segments; with the */  \
    /* plain window loads, and for complex rows with the window table alone (SWIFTLY_K1_WIN4=1) */                     \
    X(BandGeo5Pre, 1, 1, 1, 16, 1, 0, 0, 0)                                                                            \
    X(BandGeo5Pre, 1, 1, 1, 16, 1, 0, 1, 0)                                                                            \
    X(BandGeo5Pre, 1, 1, 1, 16, 1, 0, 2, 0)                                                                            \
    X(BandGeo5Pre, 1, 1, 1, 16, 1, 1, 0, 0)                                                                            \
    X(BandGeo5Pre, 1, 1, 1, 22, 1, 0, 0, 0)                                                                            \
    X(BandGeo5Pre, 1, 1, 1, 22, 1, 0, 1, 0)                                                                            \
    X(BandGeo5Pre, 1, 1, 1, 22, 1, 0, 2, 0)                                                                            \
    X(BandGeo5Pre, 1, 1, 1, 22, 1, 1, 0, 0)                                                                            \
    X(BandGeo5Pre, 1, 1, 1, 24, 1, 0, 0, 0)                                                                            \
    X(BandGeo5Pre, 1, 1, 1, 24, 1, 0, 1, 0)                                                                            \
    X(BandGeo5Pre, 1, 1, 1, 24, 1, 0, 2, 0)                                                                            \
    X(BandGeo5Pre, 1, 1, 1, 24, 1, 1, 0, 0)                                                                            \
    /* ... and the tuned ones: window table, compact twiddles, load pipeline */                                        \
    X(BandGeo5PreC, 1, 1, 1, 16, 1, 1, 0, 0)                                                                           \
    X(BandGeo5PreC, 1, 1, 1, 16, 1, 1, 1, 0)                                                                           \
    X(BandGeo5PreC, 1, 1, 1, 22, 1, 1, 0, 0)                                                                           \
    X(BandGeo5PreC, 1, 1, 1, 22, 1, 1, 1, 0)                                                                           \
    X(BandGeo5PreC, 1, 1, 1, 24, 1, 1, 0, 0)                                                                           \
    X(BandGeo5PreC, 1, 1, 1, 24, 1, 1, 1, 0)                                                                           \
    /* 65536-point rows; forward K1 with 44 of 64 segments: the 45056-point facet of the 128k workloads */            \
    X(BandGeo64k, 0, 0, 0, 0, -1, 0, 0, 0)                                                                             \
    X(BandGeo64k, 0, 1, 0, 0, -1, 0, 0, 0)                                                                             \
    X(BandGeo64k, 0, 2, 0, 0, -1, 0, 0, 0)                                                                             \
    X(BandGeo64k, 0, 2, 0, 0, -1, 0, 0, 1)                                                                             \
    X(BandGeo64k, 1, 0, 0, 0, -1, 0, 0, 0)                                                                             \
    X(BandGeo64k, 1, 1, 0, 0, -1, 0, 0, 0)                                                                             \
    X(BandGeo64k, 1, 1, 0, 0, -1, 0, 1, 0)                                                                             \
    X(BandGeo64k, 1, 1, 0, 44, 1, 0, 0, 0)                                                                             \
    X(BandGeo64k, 1, 1, 0, 44, 1, 0, 1, 0)

// -- re-laid-out load windows (Win4Cache, swiftly_rowpass.h) ------------------------------------------------------
// entry (p * T + t), T = seglen / 2 lanes: the window pairs of the p-th segment pair of the K1 load loop -- segments
// (p, p + 16) for p < ns - 16, then (s, s + 1) -- at the lane's elements q = (2 t + u + c + seglen * segment) mod n
__global__ void build_win4_kernel(const float* __restrict__ win, float* __restrict__ tab, int c, int len, int ns, int n,
                                  int seglen) {
    const int T = seglen >> 1, idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (ns >> 1) * T) return;
    const int p = idx / T, t = idx - p * T, nb1 = ns - 16;
    const int s0 = p < nb1 ? p : nb1 + 2 * (p - nb1), s1 = p < nb1 ? p + 16 : s0 + 1;
    const int q0 = (2 * t + c + seglen * s0) & (n - 1), q1 = (2 * t + c + seglen * s1) & (n - 1);
    f32x4 v;
    v.x = q0 < len ? win[q0] : 0.f;
    v.y = q0 + 1 < len ? win[q0 + 1] : 0.f;
    v.z = q1 < len ? win[q1] : 0.f;
    v.w = q1 + 1 < len ? win[q1 + 1] : 0.f;
    reinterpret_cast<f32x4*>(tab)[idx] = v;
}
static int win4_enabled() {  // SWIFTLY_K1_WIN4: 0 = the plain window loads, 1 = re-laid-out window, 2 = + compact twiddle sections (A/B runs)
    static const int v = getenv("SWIFTLY_K1_WIN4") ? atoi(getenv("SWIFTLY_K1_WIN4")) : 2;
    return v;
}
const float* Win4Cache::get(const float* win, int c, int len, int ns, int n, int seglen, hipStream_t s) {
    std::lock_guard<std::mutex> lock(mu);
    for (Entry& e : items)
        if (e.win == win && e.c == c && e.len == len && e.ns == ns && e.n == n && e.seglen == seglen) {
            // (r5 advisor) a launch on another stream than the one the table was built on waits for the build -- until the
            // build has been seen complete once; after that the table is a constant like the twiddle tables
            if (!e.complete && e.built_on != s) {
                const hipError_t q = hipEventQuery(e.ready);
                if (q == hipSuccess) {
                    e.complete = true;
                } else {
                    (void)hipGetLastError();  // hipErrorNotReady must not be mistaken for a failed launch later
                    if (hipStreamWaitEvent(s, e.ready, 0) != hipSuccess) return nullptr;
                }
            }
            return e.tab;
        }
    if (items.size() >= kMaxEntries) return nullptr;
    Entry e{win, c, len, ns, n, seglen, nullptr, nullptr, s, false};
    const int count = (ns >> 1) * (seglen >> 1);
    if (hipMalloc(&e.tab, (size_t)count * 16) != hipSuccess) return nullptr;
    if (hipEventCreateWithFlags(&e.ready, hipEventDisableTiming) != hipSuccess) {
        (void)hipFree(e.tab);
        return nullptr;
    }
    hipLaunchKernelGGL(build_win4_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, win, e.tab, c, len, ns, n, seglen);
    if (hipGetLastError() != hipSuccess || hipEventRecord(e.ready, s) != hipSuccess) {
        (void)hipStreamSynchronize(s);
        (void)hipEventDestroy(e.ready);
        (void)hipFree(e.tab);
        return nullptr;
    }
    items.push_back(e);
    return e.tab;
}
void Win4Cache::clear() {
    std::lock_guard<std::mutex> lock(mu);
    for (Entry& e : items) {
        (void)hipEventDestroy(e.ready);
        (void)hipFree(e.tab);
    }
    items.clear();
}

int launch_row_pass_band(const RowPassArgs& a, const cx<float>* tw14, const cx<float>* tw_full, hipStream_t s, Win4Cache* w4) {
    return launch_row_pass_band_n(15, a, tw14, tw_full, s, w4);
}
// what choose_band_instance reads of a call; table_available: what Win4Cache::get is assumed to answer
static BandCall band_call_of(int logn, const RowPassArgs& a, const Win4Cache* w4, bool table_available) {
    BandCall c;
    c.logn = logn;
    c.ld_a = a.ld_a, c.ld_len = a.ld_len, c.ld_c = a.ld_c, c.ld_mod = a.ld_mod;
    c.ld_win = a.ld_win != nullptr;
    c.band_sign = a.band_len > 0 ? 1 : a.band_len < 0 ? -1 : 0;
    c.band_half = a.band_half;
    c.conj_ld = a.conj_ld, c.conj_st = a.conj_st, c.accumulate = a.accumulate;
    c.in_real = a.in_real, c.out_real = a.out_real;
    c.pitch_odd = a.in_pitch & 1;
    c.base_align = (int)(reinterpret_cast<uintptr_t>(a.in) & 15);
    c.win_full = a.win_full;
    c.win_logm = a.win_logm, c.nwin = a.nwin;
    c.win_d = a.win_d, c.win_fn = a.win_fn, c.win_tw_m = a.win_tw_m, c.win_twc_m = a.win_twc_m;
    c.win4_level = win4_enabled();
    c.whole_enabled = row_pass_whole_enabled();
    c.has_cache = w4 != nullptr;
    c.has_twc = w4 && w4->twc;
    c.table_available = table_available;
    c.stage_columns = row_pass_whole_stage_columns(), c.max_windows = kWholeMaxWindows;
    c.whole_real = true;  // row_whole.hip has the real window-rows instances
    return c;
}
// per thread: the instance the last call with rows settled on, and the number of such calls (last_band_instance)
static thread_local BandInst t_last_band;
static thread_local long long t_band_calls = 0;
long long last_band_instance(BandInst* out) {
    if (out) *out = t_last_band;
    return t_band_calls;
}
// logn = log2 of the full row length (14, 15 or 16); tw_half = table of length 2^(logn-1), tw_full of length 2^logn.
// Returns -1 when no instance takes the call and -2 when the window-rows form (RowPassArgs::win_full) does not apply.
int launch_row_pass_band_n(int logn, const RowPassArgs& a0, const cx<float>* tw_half, const cx<float>* tw_full, hipStream_t s,
                           Win4Cache* w4) {
    if (a0.nrows <= 0) return 0;
    RowPassArgs a = a0;
    // the choice is pure: made with the window table assumed available, and again without it when the cache has none
    BandInst inst = choose_band_instance(band_call_of(logn, a, w4, true));
    const float* table = nullptr;
    if (inst.key_ns) {
        table = w4->get(a.ld_win, inst.key_c, a.ld_len, inst.key_ns, inst.key_n, inst.key_seglen, s);
        if (!table) inst = choose_band_instance(band_call_of(logn, a, w4, false));
    }
    t_last_band = inst, t_band_calls++;  // (what last_band_instance answers: the choice after the fallback, refusals too)
    if (inst.status != kBandChosen) return inst.status;
    a.seg_rot = inst.seg_rot;
    a.ld_win4 = inst.ld_win4 ? table : nullptr;
    a.twc = inst.twc ? w4->twc : nullptr;
    if (inst.family == kBandWholeRow) return launch_row_pass_whole(a, inst.nseg, inst.real, tw_half, tw_full, s);
    const unsigned blocks = (unsigned)(((a.nrows + 7) / 8) * 16);
#define SWF_BAND_LAUNCH(G, WIN, ST, PAIR, NSEG, CJ, W4, REAL, REAL_ST)                                                       \
    if (inst.geo == k##G && inst.win == WIN && inst.st == ST && inst.pair == PAIR && inst.nseg == NSEG && inst.cj == CJ &&   \
        inst.w4 == W4 && inst.real == REAL && inst.real_st == REAL_ST)                                                       \
        return launch_lds<row_pass_band_kernel<G, WIN, ST, PAIR, NSEG, CJ, W4, REAL, REAL_ST>, G::LDS_BYTES>(                \
            dim3(blocks), dim3(G::NT), s, a, a.in, a.out, a.ld_win, tw_half, tw_full);
    SWF_BAND_INSTANCES(SWF_BAND_LAUNCH)
#undef SWF_BAND_LAUNCH
    return -1;  // the choice names an instance the list lacks: a bug (tests/test_band_instances_cpu.py)
}
int row_pass_band_occupancy() {
    int n = -1;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, row_pass_band_kernel<BandGeo5, true, 1>, BandGeo5::NT,
                                                       BandGeo5::LDS_BYTES);
    return n;
}
// occupancy query (blocks per CU) for tuning / DESIGN.md
int row_pass_half_occupancy(int lds_bytes) {
    int n = -1;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, row_pass_split_kernel<SplitGeo2, 1, false>, SplitGeo2::NT,
                                                       lds_bytes < 0 ? SplitGeo2::LDS_BYTES : (size_t)lds_bytes);
    return n;
}

}  // namespace swf
