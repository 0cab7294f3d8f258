// instantiation + launcher of the half-length real-output B8 (swiftly_rowc2r.h)
#include "swiftly_launch.h"
#include "swiftly_rowc2r.h"

namespace swf {

int launch_row_c2r_band(const RowPassArgs& a, const cx<float>* tw14, const cx<float>* tw_full, hipStream_t s) {
    constexpr int N = 2 * RowC2RGeo::N;
    if (a.nrows <= 0) return 0;
    if (a.in_real || !a.out_real || !a.st_win || a.st_win2 || a.ld_win || !a.twc || a.accumulate || a.conj_ld || a.conj_st ||
        a.rm_mod > 0 || a.row_win || a.ld_c != 0 || a.ld_mod != a.ld_len || a.st_c != 0 || a.st_mod != a.st_len ||
        a.ld_a < 0 || a.ld_a >= N || a.ld_len <= 0 || a.ld_len > N || a.st_a < 0 || a.st_a >= N || a.st_len <= 0 || a.st_len >= N ||
        ((a.st_a | a.st_len) & 1) || (a.out_pitch & 1) || a.out_pitch < a.st_len || (reinterpret_cast<uintptr_t>(a.out) & 7))
        return -1;  // not this kernel's call: the entry point refuses before it gets here
    return launch_lds<row_c2r_band_kernel<RowC2RGeo>, RowC2RGeo::LDS_BYTES>(dim3((unsigned)a.nrows), dim3(RowC2RGeo::NT), s, a, a.in,
                                                                           reinterpret_cast<float*>(a.out), a.st_win, tw14, tw_full);
}
int row_c2r_band_occupancy() {
    int n = -1;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, row_c2r_band_kernel<RowC2RGeo>, RowC2RGeo::NT, RowC2RGeo::LDS_BYTES);
    return n;
}

}  // namespace swf
