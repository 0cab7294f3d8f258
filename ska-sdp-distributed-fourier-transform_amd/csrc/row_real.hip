// instantiation + launcher of the half-length real K1 (swiftly_rowreal.h)
#include "swiftly_launch.h"
#include "swiftly_rowreal.h"

namespace swf {

template <class G>
static int launch_row_real_band_geo(const RowPassArgs& a, const cx<float>* tw_half, const cx<float>* tw_full, hipStream_t s) {
    return launch_lds<row_real_band_kernel<G>, G::LDS_BYTES>(dim3((unsigned)a.nrows), dim3(G::NT), s, a,
                                                             reinterpret_cast<const float*>(a.in), a.out, a.ld_win, tw_half, tw_full);
}

int launch_row_real_band(int log_yN, const RowPassArgs& a, const cx<float>* tw_half, const cx<float>* tw_full, hipStream_t s) {
    if (log_yN != RowRealGeo::LOGN + 1 && log_yN != RowRealGeo64k::LOGN + 1) return -1;
    if (a.nrows <= 0) return 0;
    if (!a.in_real || a.out_real || a.band_len <= 0 || !a.ld_win || !a.twc || a.accumulate || a.ld_c != 0 || a.ld_mod != a.ld_len ||
        ((a.ld_a | a.ld_len | a.in_pitch) & 1) || (reinterpret_cast<uintptr_t>(a.in) & 7))
        return -1;  // not this kernel's call: the entry point refuses before it gets here
    // (the load map and the band of the padded row: the kernel masks with N - 1, the descriptors range-check with ld_len)
    const int N = 1 << log_yN;
    if (a.ld_a < 0 || a.ld_a >= N || a.ld_len <= 0 || a.ld_len > N || a.band_start < 0 || a.band_start >= N || a.band_len > N)
        return -1;
    if (log_yN == RowRealGeo64k::LOGN + 1) return launch_row_real_band_geo<RowRealGeo64k>(a, tw_half, tw_full, s);
    return launch_row_real_band_geo<RowRealGeo>(a, tw_half, tw_full, s);
}
int row_real_band_occupancy(int log_yN) {
    int n = -1;
    if (log_yN == RowRealGeo64k::LOGN + 1)
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, row_real_band_kernel<RowRealGeo64k>, RowRealGeo64k::NT, RowRealGeo64k::LDS_BYTES);
    else
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, row_real_band_kernel<RowRealGeo>, RowRealGeo::NT, RowRealGeo::LDS_BYTES);
    return n;
}

}  // namespace swf
