// instantiations + dispatch of the fused "sum over an off1 group + finish along the strided axis" column kernel: one
// instance per pair of GF_PAIRS (swiftly_caps.h, where the gate reads the same table)
#include "swiftly_groupfinish.h"
#include "swiftly_launch.h"

namespace swf {

template <int LOGM, int LOGX>
static int launch_one_g(const GroupFinishArgs& a, int nbatch, int ngroups, hipStream_t s) {
    using S = GFGeo<LOGM, LOGX>;
    dim3 grid((unsigned)((a.ncols + 15) / 16), (unsigned)nbatch, (unsigned)ngroups);
    return launch_lds<group_finish_kernel<LOGM, LOGX>, S::LDS_BYTES>(grid, dim3(S::NT), s, a);
}

int launch_group_finish(int logm, int logx, const GroupFinishArgs& a, int nbatch, int ngroups, hipStream_t s) {
#define GF_CASE(M, XX) \
    if (logm == M && logx == XX) return launch_one_g<M, XX>(a, nbatch, ngroups, s);
    GF_PAIRS(GF_CASE)
#undef GF_CASE
    return -1;
}

}  // namespace swf
