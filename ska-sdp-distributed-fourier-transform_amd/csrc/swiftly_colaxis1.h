// SwiFTly on MI355X: pass A' of K2's strided-axis four-step with the contiguous-axis finish folded in (the third form of
// the axis-1-first order, SwiftlyConfig(axis1_first="k2"); swiftly_hip_prepare_facet_columns_axis1).
//
// The strided-axis transform of K2 has length yN = n1 * n2 (input index y = y1*n2 + y2, output index k = k1 + n1*k2,
// col_transform).  Its first pass reads, per workgroup, the n1 band-buffer rows {y1*n2 + y2} restricted to the wave's
// m-column window -- exactly the data the contiguous-axis half of add_to_subgrid (core.py:255-285) works on.  A workgroup
// here owns that tile across the WHOLE window (n1 * m = 16384 points in LDS) and runs, in this order:
//   1. per PRESENT row (rows outside the facet are the zero padding of prepare_facet along axis 0: neither loaded nor
//      transformed), what axis1_rows_kernel (swiftly_sumfinish.h) does -- gather in window order, m-point transform, Fn,
//      rotation by the facet's s'1 -- one wave per row; the finished row Z stays in LDS, in the row's own exchange buffer;
//   2. the n1-point step of the strided-axis transform over the tile's rows for every window column, the four-step
//      twiddle W_yN^(y2 k1), and the store to the four-step scratch (row y2*n1 + k1, as pass A of col_transform).
// The order matters: the strided-axis arithmetic sees rows that carry ONE facet window (tests/accuracy_model.py,
// forward_chain_reordered).  Pass B is the unchanged column pass of n2 points.  The finished rows never reach HBM: the
// "rows" form writes and re-reads them (finish_axis1_rows -> K2), 2 * rows * m * 8 bytes per facet and wave.
#pragma once
#include "swiftly_colpass.h"
#include "swiftly_sumfinish.h"

namespace swf {

struct ColAxis1Args {
    const cx<float>* in;   // bands[f][row][band columns], parity-split
    cx<float>* out;        // four-step scratch [f][y2 * n1 + k1][m]
    long long in_fs, in_rs;  // elements: facet, row
    long long out_fs;        // yN * m
    int rows;              // facet rows held by a band buffer (the other yN - rows are zero padding)
    int yN;
    int band_start, band_len, band_half;
    int c0;                // logical column of window element 0: (yN/2 - m/2 + s) mod yN
    int s;                 // s mod m
    int scratch_nt;        // stream the scratch stores (a large intermediate), as ColPassArgs::scratch_nt
    int sp[kSumFinishMaxFacets];    // s'1 = floor(facet_off1 * xM / N) mod m per facet
    int ld_a[kSumFinishMaxFacets];  // facet_in_padded_facet(rows, facet_off0).a per facet: the load map of K2
    const float* fn;
    const cx<float>* tw_m;
    const cx<float>* twc_m;
    const cx<float>* tw_full;  // exp(-2 pi i k / yN)
};

constexpr int kColAxis1Threads = 512;  // eight waves: a wave finishes n1 / 8 rows, a thread then transforms 32 points of a column
constexpr int kColAxis1LogTile = 14;   // n1 * m points per workgroup

// The m-point transform of one row on one wave, as Axis1Geo, with the row's exchange buffer as the row of the tile: one pad
// element per 16 (128 bytes) at every radix, so that both instances keep 16384 * 17 / 16 elements = 136 KiB.  (A phase's
// scatter offsets stay compile-time constants: the radix digit only fills bits that are zero in the base index, so
// (e0 | d) >> 4 == (e0 >> 4) + (d >> 4) whatever the radix.)
template <int LOGM>
struct ColAxis1RowGeo : Geo<float, LOGM, LOGM - 6, 64, false> {
    static constexpr int LOGPAD = 4;
    static constexpr int PITCH = (1 << LOGM) + ((1 << LOGM) >> LOGPAD);
    static constexpr size_t LDS_BYTES = (size_t)PITCH * sizeof(cx<float>);
};
template <int LOGM>
struct ColAxis1Geo {
    static constexpr int LOGN1 = kColAxis1LogTile - LOGM;
    static_assert(LOGN1 == 5 || LOGN1 == 6, "column step: 32 points per thread, one or two threads per column");
    using GM = ColAxis1RowGeo<LOGM>;
    static constexpr size_t LDS_BYTES = (size_t)(1 << LOGN1) * GM::LDS_BYTES;
};

template <int LOGM>
__global__ __launch_bounds__(kColAxis1Threads) void col_axis1_kernel(const ColAxis1Args A) {
    using GM = typename ColAxis1Geo<LOGM>::GM;
    constexpr int LOGN1 = ColAxis1Geo<LOGM>::LOGN1;
    constexpr int M = 1 << LOGM, N1 = 1 << LOGN1, PM = GM::P, NW = kColAxis1Threads / 64, RW = N1 / NW;
    static_assert(GM::T == 64 && RW * NW == N1, "one wave per row");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    cx<float>* tile = reinterpret_cast<cx<float>*>(smem);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int o = blockIdx.x, f = blockIdx.y;  // y2, facet
    const int yN = A.yN, n2 = yN >> LOGN1;
    const cx<float>* __restrict__ in = A.in + (long long)f * A.in_fs;
    const int sp = A.sp[f], lda = A.ld_a[f];
    auto wrapn = [yN](int v) { return v >= yN ? v - yN : v; };
    auto pos = [](int e) { return e + (e >> GM::LOGPAD); };

    // ---- 1. the contiguous-axis finish of the wave's rows y1 = wave + j * NW
    // physical band column of the lane's window elements (axis1_rows_kernel), the same for every row; -1: outside the band
    int src[PM];
    static_for<0, PM>([&](auto vI) {
        constexpr int v = decltype(vI)::value;
        const int ci = (lane + v * 64) ^ (M >> 1);   // centred element of x (plain index lane + 64 v)
        const int i = (ci - A.s) & (M - 1);          // window element that lands there
        int col = A.c0 + i;
        if (col >= yN) col -= yN;
        int d = col - A.band_start;
        if (d < 0) d += yN;
        src[v] = d < A.band_len ? (d & 1) * A.band_half + (d >> 1) : -1;  // (a window always lies inside the band: host-checked)
    });
    // every row of the wave is requested before the first transform starts
    cx<float> x[RW][PM];
    int present = 0;  // bit j: row j of the wave lies inside the facet (uniform)
    static_for<0, RW>([&](auto jI) {
        constexpr int j = decltype(jI)::value;
        const int pi = (wave + j * NW) * n2 + o;  // the load map of K2's pass A: centred shift, facet offset, zero padding
        const int q = wrapn(wrapn(pi + (yN >> 1)) + lda);
        if (q < A.rows) {  // uniform
            present |= 1 << j;
            const cx<float>* __restrict__ row = in + (long long)q * A.in_rs;
            static_for<0, PM>([&](auto vI) {
                constexpr int v = decltype(vI)::value;
                x[j][v] = row[src[v] >= 0 ? src[v] : 0];
                if (src[v] < 0) x[j][v] = cx<float>{0.f, 0.f};
            });
        }
    });
    static_for<0, RW>([&](auto jI) {
        constexpr int j = decltype(jI)::value;
        cx<float>* zrow = tile + (wave + j * NW) * GM::PITCH;
        if (present & (1 << j)) {  // uniform
            fft_phases<SFCompact<GM>, float, 0>(x[j], lane, 0, false, zrow, A.tw_m, [&](int e, cx<float> v) {
                const int ck = e ^ (M >> 1);
                const int kk = (ck - sp) & (M - 1);
                const float w = A.fn[kk];
                // Z[kk] is what K2 gathers as window element kk; conjugated here as K2 conjugates on load (inverse transform)
                zrow[pos(kk)] = cx<float>{v.x * w, -v.y * w};
            }, nullptr, A.twc_m);
        } else {
            static_for<0, PM>([&](auto vI) { zrow[pos(lane + decltype(vI)::value * 64)] = cx<float>{0.f, 0.f}; });
        }
    });
    __syncthreads();

    // ---- 2. the n1-point step over the rows of the tile, four-step twiddle, store at scratch row y2 * n1 + k1
    cx<float>* __restrict__ out = A.out + (long long)f * A.out_fs + (long long)o * N1 * M;
    const unsigned mask = (unsigned)yN - 1u;
    auto store = [&](int k1, int c, cx<float> v) {
        const cx<float> w = A.tw_full[((unsigned)k1 * (unsigned)o) & mask];  // uniform
        v = cmul(v, w);
        cx<float>* p = out + k1 * M + c;
        if (A.scratch_nt) cp_store<true>(p, v);
        else cp_store<false>(p, v);
    };
    cx<float> y[32];
    if constexpr (N1 == 32) {  // one thread per column
        const int c = threadIdx.x;
        static_for<0, 32>([&](auto vI) { y[decltype(vI)::value] = tile[decltype(vI)::value * GM::PITCH + pos(c)]; });
        fft_reg<float, 5, 1, 0, 32>(y);
        static_for<0, 32>([&](auto kI) {
            constexpr int k = decltype(kI)::value;
            store(k, c, y[bitrev(k, 5)]);
        });
    } else {  // 64 = 2 x 32: thread (c, h) transforms the rows of parity h, then combines 16 of the 32 pairs
        const int c = threadIdx.x & (M - 1);
        const int h = __builtin_amdgcn_readfirstlane(threadIdx.x >> LOGM);
        cx<float>* col = tile + pos(c);
        static_for<0, 32>([&](auto vI) { y[decltype(vI)::value] = col[(h + 2 * decltype(vI)::value) * GM::PITCH]; });
        fft_reg<float, 5, 1, 0, 32>(y);
        // A_h[ka] * W_64^(h ka) back to row h + 2 ka (a thread only rewrites the rows it has read)
        static_for<0, 32>([&](auto kI) {
            constexpr int ka = decltype(kI)::value;
            cx<float> v = y[bitrev(ka, 5)];
            if (h) v = mul_w64<float, ka>(v);  // uniform
            col[(h + 2 * ka) * GM::PITCH] = v;
        });
        __syncthreads();
        static_for<0, 16>([&](auto iI) {
            const int ka = 16 * h + decltype(iI)::value;
            const cx<float> a = col[(2 * ka) * GM::PITCH], b = col[(2 * ka + 1) * GM::PITCH];
            store(ka, c, a + b);
            store(ka + 32, c, a - b);
        });
    }
}

// is there an instance for (log2 yN, log2 m)?  (col_axis1_instance, swiftly_caps.h, states the same pairs for the gates)
int launch_col_axis1(int log_yN, int logm, const ColAxis1Args& a, int nfacets, hipStream_t s);

}  // namespace swf
