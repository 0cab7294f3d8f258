// instantiations + dispatch of the fused "sum over an off1 group + finish along the strided axis" column kernel: one
// instance per pair of GF_PAIRS (swiftly_caps.h, where the gate reads the same table), in two forms: one workgroup per
// tile, and persistent workgroups that walk the tiles (grid_cap > 0)
#include "swiftly_groupfinish.h"
#include "swiftly_launch.h"

namespace swf {

template <int LOGM, int LOGX>
static int launch_one_g(const GroupFinishArgs& a, int nbatch, int ngroups, int grid_cap, hipStream_t s) {
    using S = GFGeo<LOGM, LOGX>;
    const unsigned ntx = (unsigned)((a.ncols + 15) / 16);
    if (grid_cap <= 0)
        return launch_lds<group_finish_kernel<LOGM, LOGX>, S::LDS_BYTES>(dim3(ntx, (unsigned)nbatch, (unsigned)ngroups), dim3(S::NT), s,
                                                                        a);
    const long long ntiles = (long long)ntx * nbatch * ngroups;
    if (ntiles <= 0 || ntiles > 0x7fffffff) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)std::min<long long>(ntiles, grid_cap));
    return launch_lds<group_finish_kernel_persistent<LOGM, LOGX>, GFPersistentLds<LOGM, LOGX>::BYTES>(grid, dim3(S::NT), s, a, nbatch, (int)ntiles);
}

int launch_group_finish(int logm, int logx, const GroupFinishArgs& a, int nbatch, int ngroups, int grid_cap, hipStream_t s) {
#define GF_CASE(M, XX) \
    if (logm == M && logx == XX) return launch_one_g<M, XX>(a, nbatch, ngroups, grid_cap, s);
    GF_PAIRS(GF_CASE)
#undef GF_CASE
    return -1;
}

}  // namespace swf
