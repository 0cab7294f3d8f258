// instantiation + launcher of the half-length real K1 (swiftly_rowreal.h)
#include "swiftly_launch.h"
#include "swiftly_rowreal.h"

namespace swf {

int launch_row_real_band(const RowPassArgs& a, const cx<float>* tw14, const cx<float>* tw_full, hipStream_t s) {
    if (a.nrows <= 0) return 0;
    if (!a.in_real || a.out_real || a.band_len <= 0 || !a.ld_win || !a.twc || a.accumulate || a.ld_c != 0 || a.ld_mod != a.ld_len ||
        ((a.ld_a | a.ld_len | a.in_pitch) & 1) || (reinterpret_cast<uintptr_t>(a.in) & 7))
        return -1;  // not this kernel's call: the entry point refuses before it gets here
    return launch_lds<row_real_band_kernel<RowRealGeo>, RowRealGeo::LDS_BYTES>(dim3((unsigned)a.nrows), dim3(RowRealGeo::NT), s, a,
                                                                              reinterpret_cast<const float*>(a.in), a.out,
                                                                              a.ld_win, tw14, tw_full);
}
int row_real_band_occupancy() {
    int n = -1;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, row_real_band_kernel<RowRealGeo>, RowRealGeo::NT, RowRealGeo::LDS_BYTES);
    return n;
}

}  // namespace swf
