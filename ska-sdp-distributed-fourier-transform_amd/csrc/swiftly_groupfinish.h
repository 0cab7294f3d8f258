// SwiFTly on MI355X: "sum over the facets of one off1 GROUP + finish" along the STRIDED axis of a subgrid (complex64).
//
// The subgrid side of the forward pass (api_helper.sum_and_finish_subgrid, api_helper.py:73-112) is separable, so the
// axis-0 half can be finished completely before the axis-1 half starts:
//
//     T_g[a, j] = mask0[a] * cifft_xM( sum_{f in g} place0_f( Fn * cfft_m( C_f[:, j] ) ) )[(xM/2 - xA//2 + a + off0) mod xM]
//     S[a, c]   = mask1[c] * cifft_xM( sum_g place1_g( Fn * cfft_m( T_g[a, :] ) ) )[(xM/2 - xA//2 + c + off1) mod xM]
//
// with g = the facets that share an off1 (a column of the facet grid), C_f the [m, m] contribution of facet f
// (extract_from_facet along both axes, core.py:243-253), place0_f / place1_g the placement of add_to_subgrid
// (core.py:274-285) and the crop of finish_subgrid (core.py:316-323).  This kernel is the first line: per 16-column tile
// it gathers the window rows of every facet of the group straight from the wave's K2 buffers Q_f (one or two column
// pieces, as col_pass2_kernel reads them), transforms them (m points, strided axis), weights with Fn, places and sums
// them over the facets IN REGISTERS, runs the xM-point inverse transform, crops to xA rows and applies mask0.  The second
// line is sum_finish_facets_kernel (swiftly_sumfinish.h) over the rows of T, one full-coverage entry list per group.
//
// Against K3 -> G[F][S][m][m] -> sum_finish_facets -> tmp[S][xM][xA] -> finish_subgrid(axis 0) the intermediate shrinks
// from F*m*m + xM*xA to n_groups*xA*m complex values per subgrid (26.5 -> 11.4 MB on the 3x3 cover of the N = 65536
// workload) and is written once and read once: 78.8 -> 48.6 MB of HBM traffic per subgrid.
//
// Geometry: 16-column tiles (128-byte row segments), 64 thread-rows, 1024 threads: thread (tr, c) owns the points
// tr + 64 v of column c in BOTH transforms (m/64 and xM/64 points per lane).  The accumulator of a lane is the register
// image of its xM-point input: output e of the m-point transform lands, placed, at a plain inverse-transform index that
// is congruent to e modulo m (see sum_finish_facets_kernel, "ACCUMULATOR IN REGISTERS"), i.e. in one of the SAME lane's
// inputs, so the placement is xM/m weighted adds per output and neither an accumulator nor a hand-over plane sits in LDS
// (the r3 form of this kernel, tools/experiments/swiftly_groupfinish.h, went through a [m][16] plane and two more
// barriers per facet).  One exchange buffer [xM][16] serves both transforms.
#pragma once
#include "swiftly_caps.h"  // GF_PAIRS, kGroupFinishMaxFacets
#include "swiftly_colpass.h"

namespace swf {

constexpr int kGroupFinishMaxBatch = 64;

struct GroupFinishArgs {
    // the wave's K2 buffers Q[f][kept rows][m], in up to two column pieces: tile columns below `split` (a multiple of 16,
    // so a tile never straddles it; 0 = one piece) come from piece B, the others from piece A; both keep window position c
    // at column c of their rows (ColPassSrc2)
    const cx<float>* in_a;
    const cx<float>* in_b;
    long long in_fs_a, in_fs_b;  // facet strides (elements)
    const int* rowmap_a;         // optional: physical row of logical row idx of the padded axis (negative = absent: zero)
    const int* rowmap_b;
    unsigned in_pitch;           // row pitch of both pieces (elements)
    int split;
    cx<float>* out;              // T[g][b][a][m]
    long long out_gs, out_bs;    // group / subgrid strides of T (elements); row stride = ncols
    int yN, xA;
    int ncols;                   // m
    int gstart[kGroupFinishMaxFacets + 1];  // facets of group g = blockIdx.z: entries gstart[g] .. gstart[g+1]
    int fidx[kGroupFinishMaxFacets];        // facet index into Q
    int sp0[kGroupFinishMaxFacets];         // s'0 = floor(facet_off0 * xM / N) of that facet
    int lda[kGroupFinishMaxBatch], ldc[kGroupFinishMaxBatch];  // row window of subgrid b: rot, base (window_of)
    int st_a[kGroupFinishMaxBatch];                            // (-(xM/2 - xA//2 + off0_b)) mod xM
    const float* fn;       // Fn[m]
    const float* mask;     // optional mask0 [nbatch][xA]
    long long mask_bs;
    const cx<float>* tw_m;
    const cx<float>* tw_x;
};

template <int LOGM, int LOGX>
struct GFGeo {
    static_assert(LOGM >= 7 && LOGM < LOGX && LOGX <= 10, "m = 128 .. , m < xM <= 1024 (128 KiB of exchange buffer)");
    static constexpr int LOGT = 6, T = 64;  // thread-rows
    template <int LOGN_>
    struct G16 {
        static constexpr int LOGN = LOGN_, LOGP = LOGN_ - LOGT;
        // interleaved (re, im) exchange: half the LDS passes and workgroup barriers of the split form.  The workgroup is
        // alone on its CU either way (1024 threads at up to 128 VGPRs fill the register file)
        static constexpr bool SPLIT = false;
        static constexpr int N = 1 << LOGN, P = 1 << LOGP, T = N / P;
        static constexpr bool WAVE_ROWS = false;
        static constexpr int COLS = 16, RB = 16, NT = COLS * T, ELEM = 8, PITCH = 0, LOGPAD = 4;
        static constexpr bool LEAN_TW = true;  // the accumulator stays live next to the m-point transform
        static constexpr size_t LDS_BYTES = (size_t)N * RB * ELEM;
    };
    using GM = G16<LOGM>;
    using GX = G16<LOGX>;
    static constexpr int NT = 16 * T;
    static constexpr size_t LDS_BYTES = GX::LDS_BYTES;
};

template <int LOGM, int LOGX>
__global__ __launch_bounds__((GFGeo<LOGM, LOGX>::NT)) void group_finish_kernel(const GroupFinishArgs A) {
    using S = GFGeo<LOGM, LOGX>;
    using GM = typename S::GM;
    using GX = typename S::GX;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int M = 1 << LOGM, X = 1 << LOGX, T = S::T, PM = GM::P, PX = GX::P, RATIO = X / M;
    static_assert(PX == PM * RATIO, "accumulator slots");
    const int tr = threadIdx.x >> 4, c16 = threadIdx.x & 15;
    const int col = blockIdx.x * 16 + c16;
    const bool live = col < A.ncols;
    const int b = blockIdx.y;  // subgrid of the wave
    const int g = blockIdx.z;  // off1 group
    // the tile's piece (workgroup-uniform)
    const bool from_b = (int)blockIdx.x * 16 < A.split;
    const cx<float>* __restrict__ src = (from_b ? A.in_b : A.in_a) + col;
    const long long in_fs = from_b ? A.in_fs_b : A.in_fs_a;
    const int* __restrict__ rowmap = from_b ? A.rowmap_b : A.rowmap_a;

    // input rows of the m-point transform (the same for every facet: the window only depends on the subgrid)
    int in_row[PM];
    static_for<0, PM>([&](auto vI) {
        constexpr int v = decltype(vI)::value;
        const int ci = (tr + v * T) ^ (M >> 1);
        const int q = (ci + A.lda[b]) & (M - 1);
        int idx = q + A.ldc[b];
        if (idx >= A.yN) idx -= A.yN;
        in_row[v] = rowmap ? rowmap[idx] : idx;
    });

    cx<float> y[PX];  // the lane's part of the padded column, y[v] = column[tr + v * T] at its plain inverse-transform index
    static_for<0, PX>([&](auto vI) { y[decltype(vI)::value] = cx<float>{0.f, 0.f}; });

    // the rows of facet n+1 are requested before facet n is transformed (the workgroup is alone on its CU: nothing else
    // hides the HBM latency)
    auto load_rows = [&](cx<float> (&dst)[PM], int n) {
        const cx<float>* __restrict__ in = src + (long long)A.fidx[n] * in_fs;
        static_for<0, PM>([&](auto vI) {
            constexpr int v = decltype(vI)::value;
            cx<float> val = {0.f, 0.f};
            if (in_row[v] >= 0 && live) val = cp_load<true>(in + (unsigned)in_row[v] * A.in_pitch);
            dst[v] = val;
        });
    };
    const int n_end = A.gstart[g + 1];
    cx<float> x[PM], xn[PM];
    if (A.gstart[g] < n_end) load_rows(x, A.gstart[g]);
    for (int n = A.gstart[g]; n < n_end; n++) {  // workgroup-uniform
        const int sp = A.sp0[n];
        if (n + 1 < n_end) load_rows(xn, n + 1);
        fft_phases<GM, float, 0>(x, tr, c16, true, smem, A.tw_m, [&](int e, cx<float> v, auto sI) {
            // slot = u * RAD + r of the last phase (radix RAD = 2^LR, NBL = PM / RAD blocks): e = tr + T * (u + NBL * r)
            constexpr int LR = GM::LOGN % GM::LOGP == 0 ? GM::LOGP : GM::LOGN % GM::LOGP, RAD = 1 << LR, NBL = PM / RAD;
            constexpr int slot = (decltype(sI)::value / RAD) + NBL * (decltype(sI)::value % RAD);
            const int ck = e ^ (M >> 1);
            const int kk = (ck - sp) & (M - 1);              // row of G = Fn[kk] * F[(kk + s') mod m]
            const int p = (kk - (M >> 1) + sp) & (X - 1);    // plain inverse-transform index of the placed element
            const int c = p >> LOGM;
            const float w = A.fn[kk];
            static_for<0, RATIO>([&](auto cI) {
                constexpr int cc = decltype(cI)::value;
                const float wc = c == cc ? w : 0.f;
                y[slot + PM * cc].x += v.x * wc;
                y[slot + PM * cc].y += v.y * wc;
            });
        });
        // (every exchange ends with a barrier behind its gather and the last phase touches no LDS: the next transform may
        // scatter at once)
        static_for<0, PM>([&](auto vI) { x[decltype(vI)::value] = xn[decltype(vI)::value]; });
    }

    // ---- xM-point inverse transform (conj . FFT . conj), crop, mask0, store
    static_for<0, PX>([&](auto vI) { y[decltype(vI)::value].y = -y[decltype(vI)::value].y; });
    cx<float>* __restrict__ out = A.out + (long long)g * A.out_gs + (long long)b * A.out_bs + col;
    const float* __restrict__ mask = A.mask ? A.mask + (long long)b * A.mask_bs : nullptr;
    const int st_a = A.st_a[b];
    const float scale = 1.f / (float)X;
    fft_phases<GX, float, 0>(y, tr, c16, true, smem, A.tw_x, [&](int e, cx<float> v) {
        const int ck = e ^ (X >> 1);
        const int d = (ck + st_a) & (X - 1);
        if (d < A.xA && live) {
            float w = scale;
            if (mask) w *= mask[d];
            cp_store<true>(out + (unsigned)d * (unsigned)A.ncols, cx<float>{v.x * w, -v.y * w});
        }
    });
}

int launch_group_finish(int logm, int logx, const GroupFinishArgs& a, int nbatch, int ngroups, hipStream_t s);

}  // namespace swf
