// instantiations of pass A' of K2's four-step with the contiguous-axis finish inside (swiftly_colaxis1.h): one instance
// per pair of CA1_PAIRS (swiftly_caps.h, where the gate reads the same table)
#include "swiftly_colaxis1.h"
#include "swiftly_launch.h"

namespace swf {

template <int LOGYN, int LOGM>
static int launch_one(const ColAxis1Args& a, int nfacets, hipStream_t s) {
    using G = ColAxis1Geo<LOGM>;
    static_assert(LOGYN - G::LOGN1 <= kColPassMaxLog, "pass B is one column pass");
    dim3 grid((unsigned)(a.yN >> G::LOGN1), (unsigned)nfacets);  // (y2, facet)
    return launch_lds<col_axis1_kernel<LOGM>, G::LDS_BYTES>(grid, dim3(kColAxis1Threads), s, a);
}

int launch_col_axis1(int log_yN, int logm, const ColAxis1Args& a, int nfacets, hipStream_t s) {
#define CA1_CASE(L, M) \
    if (log_yN == L && logm == M) return launch_one<L, M>(a, nfacets, s);
    CA1_PAIRS(CA1_CASE)
#undef CA1_CASE
    return -1;
}

}  // namespace swf
