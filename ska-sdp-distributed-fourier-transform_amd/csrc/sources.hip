// instantiations of the point-source truth kernels (swiftly_sources.h): phase tables, the rank-S subgrid update with its
// store / check epilogues for both storage types, the fixed-order partial sums and the facet scatter / row check
// (complex and real element types)
#include "swiftly_sources.h"

namespace swf {

int launch_src_phase(const SrcPhaseArgs& a, int axis, int ndistinct, hipStream_t st) {
    const dim3 grid((unsigned)((a.size + 255) / 256) * (unsigned)a.S, (unsigned)ndistinct);
    if (axis) hipLaunchKernelGGL(src_phase_kernel<1>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(src_phase_kernel<0>, grid, dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

template <typename OUT, bool CHECK>
static int launch_subgrids_one(const SrcSubgridArgs& a, int nsub, hipStream_t st) {
    hipLaunchKernelGGL((src_subgrid_kernel<OUT, CHECK>), dim3((unsigned)(a.tiles * a.tiles), (unsigned)nsub), dim3(kSrcThreads),
                       0, st, a);
    return (int)hipGetLastError();
}
int launch_src_subgrids(const SrcSubgridArgs& a, int nsub, bool c128, bool check, hipStream_t st) {
    if (c128) return check ? launch_subgrids_one<cx<double>, true>(a, nsub, st) : launch_subgrids_one<cx<double>, false>(a, nsub, st);
    return check ? launch_subgrids_one<cx<float>, true>(a, nsub, st) : launch_subgrids_one<cx<float>, false>(a, nsub, st);
}

int launch_src_sum_partials(const double* partials, long long n, int nitems, double* out, hipStream_t st) {
    hipLaunchKernelGGL(src_sum_partials_kernel<64>, dim3((unsigned)nitems), dim3(64), 0, st, partials, n, out);
    return (int)hipGetLastError();
}

template <typename OUT>
static int facet_store_one(const SrcFacetArgs& a, hipStream_t st) {
    const unsigned per_row = (unsigned)((a.size + 255) / 256);
    hipLaunchKernelGGL(src_facet_zero_kernel<OUT>, dim3(per_row * (unsigned)a.size), dim3(256), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || a.S == 0) return (int)e;
    hipLaunchKernelGGL(src_facet_store_kernel<OUT>, dim3((unsigned)((a.S + 255) / 256)), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}
int launch_src_facet_store(const SrcFacetArgs& a, bool c128, bool real, hipStream_t st) {
    if (real) return c128 ? facet_store_one<double>(a, st) : facet_store_one<float>(a, st);
    return c128 ? facet_store_one<cx<double>>(a, st) : facet_store_one<cx<float>>(a, st);
}

template <typename OUT>
static int facet_check_one(const SrcFacetArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(src_facet_check_kernel<OUT>, dim3((unsigned)a.size), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}
int launch_src_facet_check(const SrcFacetArgs& a, bool c128, bool real, hipStream_t st) {
    if (real) return c128 ? facet_check_one<double>(a, st) : facet_check_one<float>(a, st);
    return c128 ? facet_check_one<cx<double>>(a, st) : facet_check_one<cx<float>>(a, st);
}

}  // namespace swf
