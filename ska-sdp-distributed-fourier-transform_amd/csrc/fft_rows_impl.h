// Instantiates fft_rows_kernel for one scalar type over every supported
// transform length and provides the runtime dispatch.  Included by
// fft_rows_f32.hip and fft_rows_f64.hip (separate TUs so they build in
// parallel).
#pragma once
#include "swiftly_launch.h"
#include "swiftly_rows.h"

namespace swf {

template <typename R, int LOGN>
static int launch_one(const RowsArgs<R>& a, const OffTab& tab, hipStream_t s) {
    using G = typename GeoFor<R, LOGN>::type;
    const long long total = (long long)a.nrows * a.outer;
    if (total <= 0) return 0;
    unsigned grid = (unsigned)((total + G::RB - 1) / G::RB);
    if (a.outer_group) {  // row blocks padded to a multiple of 8 (one per XCD), `outer` workgroups each
        const long long rowblocks = ((long long)a.nrows + G::RB - 1) / G::RB;
        grid = (unsigned)(((rowblocks + 7) / 8) * 8 * a.outer);
    }
    if (a.real_in) {
        // real input: complex64 prepare_facet of the plain band layout (swiftly_caps.h, why_not_real_facets), 64 .. 4096 points
        // (8192: the lean row kernel, row_pass.hip)
        // complex128 prepare_facet (why_not_real_facets_f64): float64 rows, 64 .. 8192 points in one workgroup (16384 / 32768:
        // pass A of swiftly_rowslong.h)
        if constexpr ((sizeof(R) == 4 && LOGN >= kBandMinLog && LOGN < 13) ||
                      (sizeof(R) == 8 && LOGN >= kBandMinLog && LOGN <= kMaxLogNDouble))
            return launch_lds<fft_rows_kernel<G, R, true>, G::LDS_BYTES>(dim3(grid, a.nbatch > 0 ? a.nbatch : 1), dim3(G::NT), s, a, tab);
        else
            return -1;
    }
    if (a.real_out) {
        // real output: complex64 finish_facet of the plain band layout (swiftly_caps.h, why_not_real_facets_out), 64 .. 4096
        // points (8192 and longer: the lean row kernels, row_pass.hip); the mapped store only
        // complex128 finish_facet (why_not_real_facets_out_f64): float64 rows, 64 .. 8192 points, and pass B of the long rows
        // (128 / 256 points behind n1 = 128, swiftly_rowslong.h)
        if constexpr ((sizeof(R) == 4 && LOGN >= kBackwardBandMinLogYN && LOGN < 13) ||
                      (sizeof(R) == 8 && LOGN >= kBackwardBandMinLogYN && LOGN <= kMaxLogNDouble)) {
            if (a.raw_st || a.st_rowmap || a.accumulate) return -1;
            return launch_lds<fft_rows_kernel<G, R, false, true>, G::LDS_BYTES>(dim3(grid, a.nbatch > 0 ? a.nbatch : 1), dim3(G::NT), s, a, tab);
        } else {
            return -1;
        }
    }
    return launch_lds<fft_rows_kernel<G, R>, G::LDS_BYTES>(dim3(grid, a.nbatch > 0 ? a.nbatch : 1), dim3(G::NT), s, a, tab);
}

template <typename R, int LO, int HI>
struct Dispatch {
    static int launch(int logn, const RowsArgs<R>& a, const OffTab& tab, hipStream_t s) {
        if (logn == LO) return launch_one<R, LO>(a, tab, s);
        if constexpr (LO < HI) return Dispatch<R, LO + 1, HI>::launch(logn, a, tab, s);
        return -1;
    }
};

}  // namespace swf
