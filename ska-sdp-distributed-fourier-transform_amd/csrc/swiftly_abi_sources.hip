// C ABI of libswiftly_hip.so, part 4: point-source truths and RMSE checks on the device (include/swiftly_hip.h,
// "point-source truths"; kernels: swiftly_sources.h).  Handle-free: the sizes come with the call, the work runs on the
// caller's current device and stream.
#include "swiftly_abi_internal.h"
#include "swiftly_sources.h"

namespace {

const int64_t kSrcMaxImage = int64_t(1) << 31;

int check_sources_common(int dtype, const void* sources, int64_t n_sources, int64_t image_size, int64_t size) {
    CHECK_DTYPE();
    if (image_size <= 0 || image_size > kSrcMaxImage)
        return fail(SWIFTLY_ERR_PARAM, "image size %lld must be in [1, 2^31]", (long long)image_size);
    if (size <= 0 || size > image_size)
        return fail(SWIFTLY_ERR_PARAM, "size %lld must be in [1, image size = %lld]", (long long)size, (long long)image_size);
    if (n_sources < 0 || n_sources > 0x7fffffff) return fail(SWIFTLY_ERR_PARAM, "bad source count %lld", (long long)n_sources);
    if (n_sources > 0 && !sources) return fail(SWIFTLY_ERR_PARAM, "null source table");
    return 0;
}

// distinct values of offs[0 .. n) in order of first appearance (as first pixels, (off - size // 2) mod N) and the index
// of every item's value among them
void distinct_offsets(const int64_t* offs, int64_t n, int64_t size, int64_t N, std::vector<long long>& first,
                      std::vector<int32_t>& idx) {
    std::map<long long, int32_t> seen;
    idx.resize((size_t)n);
    for (int64_t b = 0; b < n; b++) {
        const long long f = src_pmod(offs[b] - size / 2, N);
        auto it = seen.find(f);
        if (it == seen.end()) {
            it = seen.emplace(f, (int32_t)first.size()).first;
            first.push_back(f);
        }
        idx[(size_t)b] = it->second;
    }
}

size_t round16(size_t x) { return (x + 15) & ~size_t(15); }

// Both subgrid entry points: phase tables per axis and distinct offset into one stream-ordered allocation, then ONE
// launch of the rank-S kernel over (tile, subgrid); check: + the fixed-order sum of the per-tile partial sums.
int subgrids_from_sources(int dtype, const void* sources, int64_t n_sources, int64_t image_size, int64_t size,
                          const int64_t* off0s, const int64_t* off1s, int64_t n_subgrids, const double* mask0s,
                          const double* mask1s, void* data, int64_t sub_stride, int64_t row_stride, double* result,
                          hipStream_t st) {
    if (int rc = check_sources_common(dtype, sources, n_sources, image_size, size)) return rc;
    if (n_subgrids < 0 || n_subgrids > 65535) return fail(SWIFTLY_ERR_PARAM, "subgrid count %lld must be in [0, 65535]", (long long)n_subgrids);
    if (n_subgrids == 0) return 0;
    if (!off0s || !off1s || !data) return fail(SWIFTLY_ERR_PARAM, "null argument");
    if (row_stride < size || sub_stride < 0) return fail(SWIFTLY_ERR_PARAM, "bad strides");
    const bool check = result != nullptr;
    const int S = (int)n_sources, tiles = (int)((size + kSrcTile - 1) / kSrcTile);
    if ((int64_t)tiles * tiles > 0x7fffffff || ((size + 255) / 256) * std::max<int64_t>(S, 1) > 0x7fffffff)
        return fail(SWIFTLY_ERR_PARAM, "size %lld x %d sources exceeds the launch grid", (long long)size, S);

    std::vector<long long> first[2];
    std::vector<int32_t> idx[2];
    distinct_offsets(off0s, n_subgrids, size, image_size, first[0], idx[0]);
    distinct_offsets(off1s, n_subgrids, size, image_size, first[1], idx[1]);

    // scratch: [P0][P1][first pixels 0][first pixels 1][idx0][idx1][partials]
    const size_t table = (size_t)S * (size_t)size * sizeof(cx<double>);
    size_t at = 0, o_p[2], o_first[2], o_idx[2];
    for (int ax = 0; ax < 2; ax++) { o_p[ax] = at; at += round16(first[ax].size() * table); }
    const size_t o_host = at;
    for (int ax = 0; ax < 2; ax++) { o_first[ax] = at; at += round16(first[ax].size() * sizeof(long long)); }
    for (int ax = 0; ax < 2; ax++) { o_idx[ax] = at; at += round16((size_t)n_subgrids * sizeof(int32_t)); }
    const size_t host_bytes = at - o_host, o_part = at;
    const size_t ntile = (size_t)tiles * tiles;
    if (check) at += (size_t)n_subgrids * ntile * 2 * sizeof(double);

    ScratchLease lease;
    if (int rc = lease.acquire(nullptr, 0, at, st, "source phase tables")) return rc;
    char* base = (char*)lease.p;
    std::vector<char> host(host_bytes, 0);
    for (int ax = 0; ax < 2; ax++) {
        std::memcpy(host.data() + (o_first[ax] - o_host), first[ax].data(), first[ax].size() * sizeof(long long));
        std::memcpy(host.data() + (o_idx[ax] - o_host), idx[ax].data(), idx[ax].size() * sizeof(int32_t));
    }
    // (pageable source: the runtime has taken its copy of `host` when this returns)
    hipError_t e = hipMemcpyAsync(base + o_host, host.data(), host_bytes, hipMemcpyHostToDevice, st);
    int rc = e == hipSuccess ? 0 : fail(SWIFTLY_ERR_HIP, "source offsets upload: %s", hipGetErrorString(e));

    for (int ax = 0; ax < 2 && !rc && S > 0; ax++) {
        SrcPhaseArgs p;
        p.src = (const SourceRec*)sources;
        p.offs = (const long long*)(base + o_first[ax]);
        p.out = (cx<double>*)(base + o_p[ax]);
        p.N = image_size; p.S = S; p.size = (int)size;
        rc = launch_status(launch_src_phase(p, ax, (int)first[ax].size(), st), "source phase tables");
    }
    if (!rc) {
        SrcSubgridArgs a;
        a.src = (const SourceRec*)sources;
        a.p0 = (const cx<double>*)(base + o_p[0]); a.p1 = (const cx<double>*)(base + o_p[1]);
        a.idx0 = (const int32_t*)(base + o_idx[0]); a.idx1 = (const int32_t*)(base + o_idx[1]);
        a.mask0 = mask0s; a.mask1 = mask1s;
        a.data = data; a.sub_stride = sub_stride; a.row_stride = row_stride;
        a.partials = check ? (double*)(base + o_part) : nullptr;
        a.inv_n2 = 1.0 / ((double)image_size * (double)image_size);
        a.S = S; a.size = (int)size; a.tiles = tiles;
        rc = launch_status(launch_src_subgrids(a, (int)n_subgrids, dtype == SWIFTLY_C128, check, st), "subgrids from sources");
        if (!rc && check)
            rc = launch_status(launch_src_sum_partials(a.partials, (long long)ntile, (int)n_subgrids, result, st), "sum of partials");
    }
    return lease.release(rc);
}

int facet_args(SrcFacetArgs& a, int dtype, const void* sources, int64_t n_sources, int64_t image_size, int64_t size,
               int64_t off0, int64_t off1, const double* mask0, const double* mask1, const void* data, int64_t row_stride) {
    if (int rc = check_sources_common(dtype, sources, n_sources, image_size, size)) return rc;
    if (!data) return fail(SWIFTLY_ERR_PARAM, "null argument");
    if (row_stride < size) return fail(SWIFTLY_ERR_PARAM, "bad row stride");
    if (((size + 255) / 256) * size > 0x7fffffff) return fail(SWIFTLY_ERR_PARAM, "facet size %lld exceeds the launch grid", (long long)size);
    std::memset(&a, 0, sizeof a);
    a.src = (const SourceRec*)sources;
    a.mask0 = mask0; a.mask1 = mask1;
    a.data = const_cast<void*>(data); a.row_stride = row_stride;
    a.N = image_size;
    a.org0 = src_pmod(off0 - size / 2, image_size); a.org1 = src_pmod(off1 - size / 2, image_size);
    a.S = (int)n_sources; a.size = (int)size;
    return 0;
}

// Both facet scatters (real: `out` holds float / double, row_stride counts reals) ...
int facet_from_sources(bool real, int dtype, const void* sources, int64_t n_sources, int64_t image_size, int64_t size,
                       int64_t off0, int64_t off1, const double* mask0, const double* mask1, void* out, int64_t row_stride,
                       hipStream_t st) {
    SrcFacetArgs a;
    if (int rc = facet_args(a, dtype, sources, n_sources, image_size, size, off0, off1, mask0, mask1, out, row_stride)) return rc;
    return launch_status(launch_src_facet_store(a, dtype == SWIFTLY_C128, real, st), "facet from sources");
}

// ... and both facet checks: one workgroup per row into per-row partial sums, then their fixed-order sum
int check_facet_from_sources(bool real, int dtype, const void* sources, int64_t n_sources, int64_t image_size, int64_t size,
                             int64_t off0, int64_t off1, const double* mask0, const double* mask1, const void* approx,
                             int64_t row_stride, const int32_t* row_start, const int32_t* row_sources, double* result,
                             hipStream_t st) {
    SrcFacetArgs a;
    if (int rc = facet_args(a, dtype, sources, n_sources, image_size, size, off0, off1, mask0, mask1, approx, row_stride)) return rc;
    if (!row_start || !result || (n_sources > 0 && !row_sources)) return fail(SWIFTLY_ERR_PARAM, "null argument");
    ScratchLease lease;
    if (int rc = lease.acquire(nullptr, 0, (size_t)size * 2 * sizeof(double), st, "facet check partial sums")) return rc;
    a.row_start = row_start; a.row_srcs = row_sources; a.partials = (double*)lease.p;
    int rc = launch_status(launch_src_facet_check(a, dtype == SWIFTLY_C128, real, st), "facet check");
    if (!rc) rc = launch_status(launch_src_sum_partials(a.partials, (long long)size, 1, result, st), "sum of partials");
    return lease.release(rc);
}

}  // namespace

extern "C" {

int swiftly_hip_subgrids_from_sources(int dtype, const void* sources, int64_t n_sources, int64_t image_size,
                                      int64_t size, const int64_t* off0s, const int64_t* off1s, int64_t n_subgrids,
                                      const double* mask0s, const double* mask1s, void* out, int64_t out_sub_stride,
                                      int64_t out_row_stride, void* stream) {
    return subgrids_from_sources(dtype, sources, n_sources, image_size, size, off0s, off1s, n_subgrids, mask0s, mask1s, out,
                                 out_sub_stride, out_row_stride, nullptr, (hipStream_t)stream);
}

int swiftly_hip_check_subgrids_from_sources(int dtype, const void* sources, int64_t n_sources, int64_t image_size,
                                            int64_t size, const int64_t* off0s, const int64_t* off1s,
                                            int64_t n_subgrids, const double* mask0s, const double* mask1s,
                                            const void* approx, int64_t approx_sub_stride, int64_t approx_row_stride,
                                            double* result, void* stream) {
    if (!result) return fail(SWIFTLY_ERR_PARAM, "null argument");
    return subgrids_from_sources(dtype, sources, n_sources, image_size, size, off0s, off1s, n_subgrids, mask0s, mask1s,
                                 const_cast<void*>(approx), approx_sub_stride, approx_row_stride, result, (hipStream_t)stream);
}

int swiftly_hip_facet_from_sources(int dtype, const void* sources, int64_t n_sources, int64_t image_size, int64_t size,
                                   int64_t off0, int64_t off1, const double* mask0, const double* mask1, void* out,
                                   int64_t out_row_stride, void* stream) {
    return facet_from_sources(false, dtype, sources, n_sources, image_size, size, off0, off1, mask0, mask1, out, out_row_stride,
                              (hipStream_t)stream);
}

int swiftly_hip_facet_from_sources_real(int dtype, const void* sources, int64_t n_sources, int64_t image_size,
                                        int64_t size, int64_t off0, int64_t off1, const double* mask0,
                                        const double* mask1, void* out, int64_t out_row_stride, void* stream) {
    return facet_from_sources(true, dtype, sources, n_sources, image_size, size, off0, off1, mask0, mask1, out, out_row_stride,
                              (hipStream_t)stream);
}

int swiftly_hip_check_facet_from_sources(int dtype, const void* sources, int64_t n_sources, int64_t image_size,
                                         int64_t size, int64_t off0, int64_t off1, const double* mask0,
                                         const double* mask1, const void* approx, int64_t approx_row_stride,
                                         const int32_t* row_start, const int32_t* row_sources, double* result,
                                         void* stream) {
    return check_facet_from_sources(false, dtype, sources, n_sources, image_size, size, off0, off1, mask0, mask1, approx,
                                    approx_row_stride, row_start, row_sources, result, (hipStream_t)stream);
}

int swiftly_hip_check_facet_from_sources_real(int dtype, const void* sources, int64_t n_sources, int64_t image_size,
                                              int64_t size, int64_t off0, int64_t off1, const double* mask0,
                                              const double* mask1, const void* approx, int64_t approx_row_stride,
                                              const int32_t* row_start, const int32_t* row_sources, double* result,
                                              void* stream) {
    return check_facet_from_sources(true, dtype, sources, n_sources, image_size, size, off0, off1, mask0, mask1, approx,
                                    approx_row_stride, row_start, row_sources, result, (hipStream_t)stream);
}

}  // extern "C"
