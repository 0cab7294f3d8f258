// complex128 pass A of the contiguous-axis four-step for 16384 / 32768 points (swiftly_rowslong.h)
#include "swiftly_launch.h"
#include "swiftly_rowslong.h"
namespace swf {
int launch_fft_long_a(const RowsArgs<double>& a, const OffTab& tab, const LongArgs<double>& L, hipStream_t s) {
    using G = LongAGeo;
    const int tiles = (1 << L.log_n2) / G::RB;
    if (L.nrows <= 0) return 0;
    const dim3 grid((unsigned)((long long)L.nrows * tiles), a.nbatch > 0 ? a.nbatch : 1);
    if (a.real_in) return launch_lds<fft_long_a_kernel<G, double, true>, kLongALds>(grid, dim3(G::NT), s, a, tab, L);
    return launch_lds<fft_long_a_kernel<G, double>, kLongALds>(grid, dim3(G::NT), s, a, tab, L);
}
}  // namespace swf
