// SwiFTly on MI355X: complex128 transforms of 16384 and 32768 points along the CONTIGUOUS axis ("complex128
// at yN = 16384 / 32768").
//
// One double row of 2^14 / 2^15 points is 256 / 512 KiB: it fits no workgroup's LDS, so the transform is a four-step
// n = n1 * n2 (n1 = 128, n2 = n / 128), y = y1*n2 + y2, k = k1 + n1*k2, through a stream-ordered scratch:
//
//   pass A (this kernel): one workgroup per (row, tile of RB consecutive y2).  Lanes run along y2, so every load and
//     every store is a contiguous run of RB elements of the row.  Loads go through the primitive's full load map (the
//     same centred shift / window / zero-pad / modular row gather / per-item offsets as fft_rows_kernel), the n1-point
//     transform over y1 runs through LDS (fft_phases, rowfast layout), the product with W_n^(y2 k1) is applied on
//     store:  scratch[row][k1][y2].
//   pass B: fft_rows_kernel<double> at log2(n2), raw load from the scratch (outer index k1), the primitive's store map
//     with plain output index k1 + n1*k2 (swiftly_abi.hip, run_rows_long).
#pragma once
#include "swiftly_rows.h"

namespace swf {

// (kLongLogN1, n1 = 128 points per column of pass A: swiftly_rowroute.h)
constexpr int kLongTileY2 = 32;  // RB: consecutive y2 per workgroup = 512-byte runs per load / store

// Pass A geometry: radix 8 (double register budget, as fft_rows_kernel), T = n1 / 8 = 16 lanes per column
using LongAGeo = Geo<double, kLongLogN1, 3, (1 << (kLongLogN1 - 3)) * kLongTileY2, false>;
static_assert(LongAGeo::RB == kLongTileY2, "pass A: one column per y2 of the tile");
// rowfast exchange layout (lds_pos = e*RB + rb): no padding
constexpr size_t kLongALds = (size_t)LongAGeo::N * LongAGeo::RB * sizeof(cx<double>);

template <typename R>
struct LongArgs {
    cx<R>* scratch;          // [nbatch][nrows][n1][n2]
    long long s_bs;          // batch stride of the scratch (nrows * n)
    int row0;                // first row of the primitive this chunk covers
    int nrows;               // rows of this chunk
    int log_n2;
    const cx<R>* tw_full;    // exp(-2 pi i k / n), k < n
};

// REAL_IN (RowsArgs::real_in, float64 facet rows into the complex128 K1): `A.in` points to R, in_rs / in_cs / in_bs count
// reals; the imaginary part is zero in registers as in load_in of fft_rows_kernel, so everything after the load sees the
// values of the promoted row.
template <class G, typename R, bool REAL_IN = false>
__global__ __launch_bounds__(G::NT) void fft_long_a_kernel(const RowsArgs<R> A, const OffTab tab, const LongArgs<R> L) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int P = G::P, T = G::T, RB = G::RB;
    const int tid = threadIdx.x;
    const int rb = tid % RB, t = tid / RB;
    const int n2 = 1 << L.log_n2;
    const int tiles = n2 / RB;
    const int r = (int)(blockIdx.x / (unsigned)tiles);  // grid.x = nrows * tiles exactly: every workgroup is live
    const int y2 = (int)(blockIdx.x % (unsigned)tiles) * RB + rb;
    const int row = L.row0 + r;
    const int FN = 1 << A.full_logn;
    auto wrapn = [FN](int v) { return v >= FN ? v - FN : v; };
    long long in_row = row;
    if (A.rm_mod > 0) {
        int r1 = row + A.rm_inner;
        if (r1 >= A.rm_mod) r1 -= A.rm_mod;
        r1 += A.rm_outer;
        if (r1 >= A.rm_full) r1 -= A.rm_full;
        in_row = r1;
    }
    if (A.in_rowmap) in_row = A.in_rowmap[in_row];
    const bool absent = in_row < 0;  // row absent from a compacted input: reads as zeros
    if (absent) in_row = 0;
    const int b = blockIdx.y;
    const long long in_base = in_row * A.in_rs + (long long)b * A.in_bs;
    const cx<R>* __restrict__ in = A.in + (REAL_IN ? 0ll : in_base);
    const R* __restrict__ rin = reinterpret_cast<const R*>(A.in) + (REAL_IN ? in_base : 0ll);
    auto load_in = [&](size_t e) -> cx<R> {
        if constexpr (REAL_IN)
            return cx<R>{rin[e], (R)0};
        else
            return in[e];
    };
    const int ld_a = (tab.use & 1) ? tab.ld_a[b] : A.ld.a;
    const int ld_c = (tab.use & 2) ? tab.ld_c[b] : A.ld.c;
    const R csign_ld = A.conj_ld ? (R)-1 : (R)1;
    const R* __restrict__ win1 = A.ld.win ? A.ld.win : &kOneTable<R>::value;
    const R* __restrict__ win2 = A.ld.win2 ? A.ld.win2 : &kOneTable<R>::value;
    const int w1s = A.ld.win ? 1 : 0, w2s = A.ld.win2 ? 1 : 0;
    const R live_f = absent ? (R)0 : (R)1;

    // branch-free mapped loads (as fft_rows_kernel): plain index y1*n2 + y2, out-of-map elements zeroed via the window
    cx<R> x[P];
    static_for<0, P>([&](auto vI) {
        constexpr int v = decltype(vI)::value;
        const int pi = (t + v * T) * n2 + y2;
        const int ci = wrapn(pi + (FN >> 1));
        const int q = wrapn(ci + ld_a);
        const bool ok = q < A.ld.len;
        const int qs = ok ? q : 0;
        int idx = qs + ld_c;
        if (idx >= A.ld.mod) idx -= A.ld.mod;
        cx<R> val = load_in((size_t)((unsigned)idx * A.in_cs));
        R w = win1[qs * w1s] * win2[qs * w2s];
        w = ok ? w * live_f : (R)0;
        val.x *= w;
        val.y *= w * csign_ld;
        x[v] = val;
    });

    cx<R>* __restrict__ out = L.scratch + (long long)b * L.s_bs + (long long)r * FN + y2;
    fft_phases<G, R, 0>(x, t, rb, true, smem, A.tw, [&](int k1, cx<R> v) {
        v = cmul(v, L.tw_full[((unsigned)k1 * (unsigned)y2) & (unsigned)(FN - 1)]);
        out[k1 * n2] = v;
    });
}

// implemented in rows_long_f64.hip
int launch_fft_long_a(const RowsArgs<double>& a, const OffTab& tab, const LongArgs<double>& L, hipStream_t s);

}  // namespace swf
