// C ABI of libswiftly_hip.so, part 3: device memory / stream helpers for callers without their own allocator,
// CU-partitioned streams and diagnostics (include/swiftly_hip.h, last section).
#include "swiftly_abi_internal.h"
#include "swiftly_rowinst.h"
#include "build/build_id.h"

// where does this workgroup run?  xcc_id << 16 | se_id << 8 | cu_id  (HW_REG_XCC_ID, HW_REG_HW_ID of gfx9);
// the workgroup lingers for a few microseconds so that a census grid spreads over all CUs its stream may use
__global__ void cu_census_kernel(int* __restrict__ out) {
    unsigned xcc, hw;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    const long long t0 = __builtin_readcyclecounter();
    while (__builtin_readcyclecounter() - t0 < 20000) {
    }
    if (threadIdx.x == 0) out[blockIdx.x] = (int)(((xcc & 0xf) << 16) | (((hw >> 13) & 0x7) << 8) | ((hw >> 8) & 0xf));
}


thread_local int g_chain_chunk_streams = 0;

// the kernels launched with dynamic LDS (swiftly_launch.h): filled while the library is loaded, read afterwards
namespace swf {
struct KernelLdsEntry {
    const void* host_fn;
    int lds_bytes;
};
static std::vector<KernelLdsEntry>& kernel_lds_table() {
    static std::vector<KernelLdsEntry> table;
    return table;
}
bool register_kernel_lds(const void* host_fn, int lds_bytes) {
    kernel_lds_table().push_back({host_fn, lds_bytes});
    return true;
}
int set_registered_kernel_attributes(int* failed_lds_bytes) {
    for (const KernelLdsEntry& e : kernel_lds_table())
        if (const hipError_t rc = hipFuncSetAttribute(e.host_fn, hipFuncAttributeMaxDynamicSharedMemorySize, e.lds_bytes)) {
            *failed_lds_bytes = e.lds_bytes;
            return (int)rc;
        }
    return 0;
}
}  // namespace swf

extern "C" {

const char* swiftly_hip_build_id(void) { return SWF_SRC_HASH; }

void swiftly_hip_chain_chunk_streams(int chain) { g_chain_chunk_streams = chain ? 1 : 0; }

int swiftly_hip_set_column_precision(swiftly_hip_t* h, int bits) {
    if (!h) return fail(SWIFTLY_ERR_PARAM, "null argument");
    if (bits != 32 && bits != 64) return fail(SWIFTLY_ERR_PARAM, "column precision must be 32 or 64");
    h->col_f64 = bits == 64;
    return 0;
}
int swiftly_hip_get_column_precision(const swiftly_hip_t* h) { return h ? (h->col_f64 ? 64 : 32) : -1; }

// the capability table (swiftly_caps.h) for callers: sizes in, no handle, no device
int swiftly_hip_supports(int feature, int dtype, int64_t N, int64_t yN_size, int64_t xM_size, int64_t n_facets) {
    std::string why = check_sizes(N, yN_size, xM_size);
    if (why.empty()) {
        const Sizes s = make_sizes(N, yN_size, xM_size);
        switch (feature) {
            case SWIFTLY_FEATURE_FUSED_SUBGRID: why = why_not_fused_subgrid(s, dtype, n_facets); break;
            case SWIFTLY_FEATURE_BAND_PIPELINE: why = why_not_band_pipeline(s, dtype, n_facets, false); break;
            case SWIFTLY_FEATURE_BAND_PIPELINE_EXPLICIT: why = why_not_band_pipeline(s, dtype, n_facets, true); break;
            case SWIFTLY_FEATURE_BACKWARD_BAND: why = why_not_backward_band(s, dtype); break;
            case SWIFTLY_FEATURE_SPLIT_BAND: why = why_not_split_band(s); break;
            case SWIFTLY_FEATURE_WINDOW_ROWS: why = why_not_window_rows(s); break;
            case SWIFTLY_FEATURE_BACKWARD_BAND_EXPLICIT: why = why_not_backward_band(s, dtype, true); break;
            case SWIFTLY_FEATURE_SPLIT_PREPARE: why = why_not_split_prepare(s, dtype, n_facets); break;
            case SWIFTLY_FEATURE_REAL_FACETS: why = why_not_real_facets(s, dtype); break;
            case SWIFTLY_FEATURE_REAL_FACETS_OUT: why = why_not_real_facets_out(s, dtype); break;
            case SWIFTLY_FEATURE_GROUP_FINISH: why = why_not_group_finish(s, dtype, n_facets); break;
            case SWIFTLY_FEATURE_REAL_WINDOW_ROWS: why = why_not_real_window_rows(s, dtype); break;
            case SWIFTLY_FEATURE_REAL_FACETS_RFFT: why = why_not_real_facets_rfft(s, dtype); break;
            case SWIFTLY_FEATURE_REAL_FACETS_OUT_C2R: why = why_not_real_facets_out_c2r(s, dtype); break;
            case SWIFTLY_FEATURE_REAL_FACETS_F64: why = why_not_real_facets_f64(s, dtype); break;
            case SWIFTLY_FEATURE_REAL_FACETS_OUT_F64: why = why_not_real_facets_out_f64(s, dtype); break;
            case SWIFTLY_FEATURE_REAL_FACETS_RFFT_64K: why = why_not_real_facets_rfft_64k(s, dtype); break;
            case SWIFTLY_FEATURE_REAL_FACETS_OUT_C2R_64K: why = why_not_real_facets_out_c2r_64k(s, dtype); break;
            case SWIFTLY_FEATURE_AXIS1_COLUMNS: why = why_not_axis1_columns(s, dtype); break;
            default: why = reason("unknown feature %d", feature);
        }
    }
    if (why.empty()) return 1;
    fail(SWIFTLY_ERR_UNSUPPORTED, "%s", why.c_str());
    return 0;
}
int64_t swiftly_hip_limit(int which) {
    switch (which) {
        case SWIFTLY_LIMIT_FUSED_FACETS: return kSumFinishMaxFacets;
        case SWIFTLY_LIMIT_WINDOW_ROWS_STAGE_COLUMNS: return row_pass_whole_stage_columns();
        case SWIFTLY_LIMIT_WINDOW_ROWS_WINDOWS: return kWholeMaxWindows;
        default: return -1;
    }
}
int swiftly_hip_mixed_factor(int64_t n, int* Q, int* log2_rest) {
    int q = 0, l = 0;
    if (!mixed_factor(n, &q, &l)) return 0;
    if (Q) *Q = q;
    if (log2_rest) *log2_rest = l;
    return 1;
}

int swiftly_hip_debug_row_band_occupancy(void) { return swf::row_pass_band_occupancy(); }

int swiftly_hip_debug_occupancy(int lds_bytes) { return swf::row_pass_half_occupancy(lds_bytes); }

int swiftly_hip_malloc(void** ptr, size_t bytes) {
    if (!ptr) return fail(SWIFTLY_ERR_PARAM, "null argument");
    HIP_TRY(hipMalloc(ptr, bytes));
    return 0;
}
int swiftly_hip_free(void* ptr) {
    HIP_TRY(hipFree(ptr));
    return 0;
}
int swiftly_hip_memset_async(void* ptr, int value, size_t bytes, void* stream) {
    HIP_TRY(hipMemsetAsync(ptr, value, bytes, (hipStream_t)stream));
    return 0;
}
int swiftly_hip_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream) {
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return 0;
}
int swiftly_hip_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream) {
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return 0;
}
int swiftly_hip_stream_synchronize(void* stream) {
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

int swiftly_hip_stream_create_cu_mask(void** stream, const uint32_t* cu_mask, int nwords) {
    if (!stream || !cu_mask || nwords <= 0) return fail(SWIFTLY_ERR_PARAM, "null argument");
    hipStream_t st = nullptr;
    HIP_TRY(hipExtStreamCreateWithCUMask(&st, (uint32_t)nwords, cu_mask));
    *stream = (void*)st;
    return 0;
}
int swiftly_hip_stream_destroy(void* stream) {
    HIP_TRY(hipStreamDestroy((hipStream_t)stream));
    return 0;
}
int swiftly_hip_cu_census(int32_t* out, int nblocks, void* stream) {
    if (!out || nblocks <= 0) return fail(SWIFTLY_ERR_PARAM, "null argument");
    hipLaunchKernelGGL(cu_census_kernel, dim3((unsigned)nblocks), dim3(64), 0, (hipStream_t)stream, out);
    HIP_TRY(hipGetLastError());
    return 0;
}
int swiftly_hip_kernel_table(int64_t* count, int64_t* max_lds_bytes) {
    if (!count || !max_lds_bytes) return fail(SWIFTLY_ERR_PARAM, "null argument");
    *count = 0;
    *max_lds_bytes = 0;
    for (const KernelLdsEntry& e : kernel_lds_table()) {
        ++*count;
        *max_lds_bytes = std::max<int64_t>(*max_lds_bytes, e.lds_bytes);
    }
    return 0;
}
int64_t swiftly_hip_last_band_instance(int32_t* out, int n) {
    BandInst b;
    const int64_t calls = last_band_instance(&b);
    const int32_t fields[18] = {b.status, b.family, b.geo, b.win, b.st, b.pair, b.nseg, b.cj, b.w4, b.real, b.real_st,
                                b.seg_rot, b.ld_win4, b.twc, b.key_c, b.key_ns, b.key_n, b.key_seglen};
    for (int i = 0; out && i < n && i < 18; i++) out[i] = fields[i];
    return calls;
}

}  // extern "C"
