// instantiation + launcher of the half-length real-output B8 (swiftly_rowc2r.h)
#include "swiftly_launch.h"
#include "swiftly_rowc2r.h"

namespace swf {

template <class G>
static int launch_row_c2r_band_geo(const RowPassArgs& a, const cx<float>* tw_half, const cx<float>* tw_full, hipStream_t s) {
    return launch_lds<row_c2r_band_kernel<G>, G::LDS_BYTES>(dim3((unsigned)a.nrows), dim3(G::NT), s, a, a.in,
                                                            reinterpret_cast<float*>(a.out), a.st_win, tw_half, tw_full);
}

int launch_row_c2r_band(int log_yN, const RowPassArgs& a, const cx<float>* tw_half, const cx<float>* tw_full, hipStream_t s) {
    if (log_yN != RowC2RGeo::LOGN + 1 && log_yN != RowC2RGeo64k::LOGN + 1) return -1;
    const int N = 1 << log_yN;
    if (a.nrows <= 0) return 0;
    if (a.in_real || !a.out_real || !a.st_win || a.st_win2 || a.ld_win || !a.twc || a.accumulate || a.conj_ld || a.conj_st ||
        a.rm_mod > 0 || a.row_win || a.ld_c != 0 || a.ld_mod != a.ld_len || a.st_c != 0 || a.st_mod != a.st_len ||
        a.ld_a < 0 || a.ld_a >= N || a.ld_len <= 0 || a.ld_len > N || a.st_a < 0 || a.st_a >= N || a.st_len <= 0 || a.st_len >= N ||
        ((a.st_a | a.st_len) & 1) || (a.out_pitch & 1) || a.out_pitch < a.st_len || (reinterpret_cast<uintptr_t>(a.out) & 7))
        return -1;  // not this kernel's call: the entry point refuses before it gets here
    if (log_yN == RowC2RGeo64k::LOGN + 1) return launch_row_c2r_band_geo<RowC2RGeo64k>(a, tw_half, tw_full, s);
    return launch_row_c2r_band_geo<RowC2RGeo>(a, tw_half, tw_full, s);
}
int row_c2r_band_occupancy(int log_yN) {
    int n = -1;
    if (log_yN == RowC2RGeo64k::LOGN + 1)
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, row_c2r_band_kernel<RowC2RGeo64k>, RowC2RGeo64k::NT, RowC2RGeo64k::LDS_BYTES);
    else
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, row_c2r_band_kernel<RowC2RGeo>, RowC2RGeo::NT, RowC2RGeo::LDS_BYTES);
    return n;
}

}  // namespace swf
