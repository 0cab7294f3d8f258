// instantiations of the fused sum + finish row kernel for the (m, xM) pairs of the catalogue families
#include "swiftly_launch.h"
#include "swiftly_sumfinish.h"

namespace swf {

template <int LOGM, int LOGX>
static int launch_one(const SumFinishArgs& a, int nbatch, hipStream_t s) {
    using S = SFGeo<LOGM, LOGX>;
    dim3 grid((unsigned)((a.nrows + S::RB - 1) / S::RB), (unsigned)nbatch);
    return launch_lds<sum_finish_rows_kernel<LOGM, LOGX>, S::LDS_BYTES>(grid, dim3(S::NT), s, a);
}

template <int LOGM, int LOGX, typename R = float>
static int launch_one_f(const SumFinishFacetArgs& a, int nbatch, hipStream_t s) {
    using S = SFGeo<LOGM, LOGX, R>;
    dim3 grid((unsigned)((a.nrows + S::RB - 1) / S::RB), (unsigned)nbatch);
    constexpr size_t lds = sum_finish_facets_kernel_lds<LOGM, LOGX, R>();
    return launch_lds<sum_finish_facets_kernel<LOGM, LOGX, R>, lds>(grid, dim3(S::NT), s, a);
}
// (complex128: exchange buffer of the m-point transforms + the prepared row, in doubles; never the wave-parallel geometry)
template <int LOGM, int LOGX, typename R>
constexpr size_t split_prepare_lds() {
    if constexpr (std::is_same_v<R, float>) return sum_finish_facets_lds<LOGM, LOGX>();  // (the same wave-parallel geometry)
    else return SFGeo<LOGM, LOGX, R>::LDS_BYTES;
}
template <int LOGM, int LOGX, typename R = float>
static int launch_one_s(const SplitFacetArgs& a, int nbatch, hipStream_t s) {
    using S = SFGeo<LOGM, LOGX, R>;
    dim3 grid((unsigned)((a.nrows + S::RB - 1) / S::RB), (unsigned)nbatch);
    constexpr size_t lds = split_prepare_lds<LOGM, LOGX, R>();
    return launch_lds<split_prepare_facets_kernel<LOGM, LOGX, R>, lds>(grid, dim3(S::NT), s, a);
}

template <int LOGM>
static int launch_axis1(const Axis1RowsArgs& a, int nfacets, hipStream_t s) {
    using GM = typename Axis1Geo<LOGM>::GM;
    dim3 grid((unsigned)((a.nrows + GM::RB - 1) / GM::RB), (unsigned)nfacets);
    return launch_lds<axis1_rows_kernel<LOGM>, Axis1Geo<LOGM>::LDS_BYTES>(grid, dim3(kAxis1Threads), s, a);
}
int launch_axis1_rows(int logm, const Axis1RowsArgs& a, int nfacets, hipStream_t s) {
    switch (logm) {
        case 7: return launch_axis1<7>(a, nfacets, s);
        case 8: return launch_axis1<8>(a, nfacets, s);
        case 9: return launch_axis1<9>(a, nfacets, s);
        case 10: return launch_axis1<10>(a, nfacets, s);
        default: return -1;
    }
}

// one instance per pair of SF_PAIRS / SF_PAIRS_C128 (swiftly_caps.h, where the gates read the same tables)

int launch_sum_finish_rows(int logm, int logx, const SumFinishArgs& a, int nbatch, hipStream_t s) {
#define SF_CASE(M, XX) \
    if (logm == M && logx == XX) return launch_one<M, XX>(a, nbatch, s);
    SF_PAIRS(SF_CASE)
#undef SF_CASE
    return -1;
}
int launch_sum_finish_facets(int logm, int logx, const SumFinishFacetArgs& a, int nbatch, hipStream_t s) {
#define SF_CASE_F(M, XX) \
    if (logm == M && logx == XX) return launch_one_f<M, XX>(a, nbatch, s);
    SF_PAIRS(SF_CASE_F)
#undef SF_CASE_F
    return -1;
}
int launch_sum_finish_facets_c128(int logm, int logx, const SumFinishFacetArgs& a, int nbatch, hipStream_t s) {
#define SF_CASE_D(M, XX) \
    if (logm == M && logx == XX) return launch_one_f<M, XX, double>(a, nbatch, s);
    SF_PAIRS_C128(SF_CASE_D)
#undef SF_CASE_D
    return -1;
}
int launch_split_prepare_facets(int logm, int logx, const SplitFacetArgs& a, int nbatch, hipStream_t s) {
#define SF_CASE_S(M, XX) \
    if (logm == M && logx == XX) return launch_one_s<M, XX>(a, nbatch, s);
    SF_PAIRS(SF_CASE_S)
#undef SF_CASE_S
    return -1;
}
int launch_split_prepare_facets_c128(int logm, int logx, const SplitFacetArgs& a, int nbatch, hipStream_t s) {
#define SF_CASE_SD(M, XX) \
    if (logm == M && logx == XX) return launch_one_s<M, XX, double>(a, nbatch, s);
    SPLIT_PAIRS_C128(SF_CASE_SD)
#undef SF_CASE_SD
    return -1;
}

}  // namespace swf
