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
// is congruent to e modulo m (swiftly_place.h, shared with sum_finish_facets_kernel), i.e. in one of the SAME lane's
// inputs, so the placement is xM/m weighted adds per output and neither an accumulator nor a hand-over plane sits in LDS
// (the r3 form of this kernel, tools/experiments/swiftly_groupfinish.h, went through a [m][16] plane and two more
// barriers per facet).  One exchange buffer [xM][16] serves both transforms.
#pragma once
#include "swiftly_caps.h"  // GF_PAIRS, kGroupFinishMaxFacets
#include "swiftly_colpass.h"
#include "swiftly_place.h"

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

// ---- The pieces of one tile (column tile tx, subgrid b, group g) that both kernels below are made of.  What differs
// between the kernels -- where the tables and the window rows live, what is requested when -- stays in the kernels.

// the piece of column tile tx (workgroup-uniform): its row map, column col of its facet 0, its facet stride
__device__ __forceinline__ bool gf_from_b(const GroupFinishArgs& A, int tx) { return tx * 16 < A.split; }
__device__ __forceinline__ const int* gf_rowmap(const GroupFinishArgs& A, int tx) { return gf_from_b(A, tx) ? A.rowmap_b : A.rowmap_a; }
__device__ __forceinline__ const cx<float>* gf_piece_column(const GroupFinishArgs& A, int tx, int col) {
    return (gf_from_b(A, tx) ? A.in_b : A.in_a) + col;
}
__device__ __forceinline__ long long gf_facet_stride(const GroupFinishArgs& A, int tx) { return gf_from_b(A, tx) ? A.in_fs_b : A.in_fs_a; }
// physical row of input point i of the m-point transform (the same for every facet: the window only depends on the
// subgrid); negative = absent
template <int M>
__device__ __forceinline__ int gf_window_row(const GroupFinishArgs& A, const int* rowmap, int b, int i) {
    const int ci = i ^ (M >> 1);
    const int q = (ci + A.lda[b]) & (M - 1);
    int idx = q + A.ldc[b];
    if (idx >= A.yN) idx -= A.yN;
    return rowmap ? rowmap[idx] : idx;
}
// the rows of one facet: dst[v] = point tr + v * T of column col, whose physical row is row_of(v); src = the piece's
// column col, facet = the facet's index in the piece, fs = the piece's facet stride
template <int PM, class RowOf>
__device__ __forceinline__ void gf_load_rows(const GroupFinishArgs& A, cx<float> (&dst)[PM], const cx<float>* src, int facet, long long fs,
                                             int col, RowOf&& row_of) {
    const bool live = col < A.ncols;
    const cx<float>* __restrict__ in = src + (long long)facet * fs;
    static_for<0, PM>([&](auto vI) {
        const int row = row_of(vI);
        cx<float> val = {0.f, 0.f};
        if (row >= 0 && live) val = cp_load<true>(in + (unsigned)row * A.in_pitch);
        dst[decltype(vI)::value] = val;
    });
}
// where the tile's column goes (element d of the cropped axis at + d * ncols), and the mask row of its subgrid, if any
__device__ __forceinline__ cx<float>* gf_out_column(const GroupFinishArgs& A, int col, int b, int g) {
    return A.out + (long long)g * A.out_gs + (long long)b * A.out_bs + col;
}
__device__ __forceinline__ const float* gf_mask_row(const GroupFinishArgs& A, int b) {
    return A.mask ? A.mask + (long long)b * A.mask_bs : nullptr;
}

// One workgroup per tile: window rows in registers, tables read from global memory, mask loaded inside the store callback.
template <int LOGM, int LOGX>
__global__ __launch_bounds__((GFGeo<LOGM, LOGX>::NT)) void group_finish_kernel(const GroupFinishArgs A) {
    using S = GFGeo<LOGM, LOGX>;
    using GM = typename S::GM;
    using GX = typename S::GX;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int M = 1 << LOGM, X = 1 << LOGX, T = S::T, PM = GM::P, PX = GX::P;
    const int tr = threadIdx.x >> 4, c16 = threadIdx.x & 15;
    const int col = blockIdx.x * 16 + c16;
    const bool live = col < A.ncols;
    const int b = blockIdx.y;  // subgrid of the wave
    const int g = blockIdx.z;  // off1 group
    const cx<float>* __restrict__ src = gf_piece_column(A, blockIdx.x, col);
    const long long in_fs = gf_facet_stride(A, blockIdx.x);
    const int* __restrict__ rowmap = gf_rowmap(A, blockIdx.x);

    int in_row[PM];
    static_for<0, PM>([&](auto vI) { in_row[decltype(vI)::value] = gf_window_row<M>(A, rowmap, b, tr + decltype(vI)::value * T); });

    cx<float> y[PX];  // the lane's part of the padded column, y[v] = column[tr + v * T] at its plain inverse-transform index
    static_for<0, PX>([&](auto vI) { y[decltype(vI)::value] = cx<float>{0.f, 0.f}; });

    // the rows of facet n+1 are requested before facet n is transformed (the workgroup is alone on its CU: nothing else
    // hides the HBM latency)
    auto load_rows = [&](cx<float> (&dst)[PM], int n) {
        gf_load_rows(A, dst, src, A.fidx[n], in_fs, col, [&](auto vI) { return in_row[decltype(vI)::value]; });
    };
    const int n_end = A.gstart[g + 1];
    cx<float> x[PM], xn[PM];
    if (A.gstart[g] < n_end) load_rows(x, A.gstart[g]);
    for (int n = A.gstart[g]; n < n_end; n++) {  // workgroup-uniform
        const int sp = A.sp0[n];
        if (n + 1 < n_end) load_rows(xn, n + 1);
        fft_phases<GM, float, 0>(x, tr, c16, true, smem, A.tw_m, [&](int e, cx<float> v, auto sI) {
            place_output<GM, LOGX, decltype(sI)::value>(y, e, sp, v, A.fn);
        });
        // (every exchange ends with a barrier behind its gather and the last phase touches no LDS: the next transform may
        // scatter at once)
        static_for<0, PM>([&](auto vI) { x[decltype(vI)::value] = xn[decltype(vI)::value]; });
    }

    // ---- xM-point inverse transform (conj . FFT . conj), crop, mask0, store
    conj_regs(y);
    cx<float>* __restrict__ out = gf_out_column(A, col, b, g);
    const float* __restrict__ mask = gf_mask_row(A, b);
    const int st_a = A.st_a[b];
    const float scale = 1.f / (float)X;
    fft_phases<GX, float, 0>(y, tr, c16, true, smem, A.tw_x, [&](int e, cx<float> v) {
        const int d = crop_index<X>(e, st_a);
        if (d < A.xA && live) {
            float w = scale;
            if (mask) w *= mask[d];
            cp_store<true>(out + (unsigned)d * (unsigned)A.ncols, cx<float>{v.x * w, -v.y * w});
        }
    });
}

// The same tiles on a PERSISTENT grid: workgroup w walks the tiles t = w, w + gridDim.x, ... of the index space
// (column tile, subgrid, group), column tile fastest -- a static walk: no counter in memory, no workgroup waits for
// another.  A tile's arithmetic is group_finish_kernel's: the same tile pieces (above), fft_phases, place_output and
// products, so every output bit is the same.  What changes is what is in flight when.
//
// gfx950 counts a wave's loads AND stores in one in-order counter (vmcnt): waiting for any of them waits for everything
// requested before it.  In group_finish_kernel every transform phase fetches its twiddles, every placement its Fn value
// and every store its mask value from global memory, so the rows of facet n + 1, requested "ahead", are waited for at the
// first table value of facet n's transform, each store is waited for at the next mask value, and from the last m-point
// transform to the exit nothing is in flight at all.  Here
//   - the tables (both twiddle tables, Fn) are copied once per workgroup into the LDS the exchange buffer leaves free, and
//     the tile's window rows (a function of the thread-row only: M values, not M x 16) are looked up once per tile into
//     LDS as well: the transforms make no global request, and what is in flight stays in flight under them;
//   - x is waited for (touch) BEFORE the next rows are requested, never after;
//   - the first facet of tile t + gridDim.x is requested before the inverse transform of tile t and waited for behind it,
//     ahead of the tile's stores; the mask values are requested together, ahead of the first store; the stores then drain
//     under the next tile's facet loop.
// tr and c16 are made opaque once per tile: every per-lane LDS address of every phase derives from them, and hoisted out
// of the tile loop they would all stay live across it (152 - 176 bytes of scratch per lane).
template <int LOGM, int LOGX>
struct GFPersistentLds {
    static constexpr int M = 1 << LOGM, X = 1 << LOGX;
    // behind the exchange buffer: tw_x[X], tw_m[M] (complex), Fn[M] (float), window rows[M] (int)
    static constexpr size_t TW_X = GFGeo<LOGM, LOGX>::LDS_BYTES, TW_M = TW_X + X * sizeof(cx<float>),
                            FN = TW_M + M * sizeof(cx<float>), ROWS = FN + M * sizeof(float), BYTES = ROWS + M * sizeof(int);
};

template <int LOGM, int LOGX>
__global__ __launch_bounds__((GFGeo<LOGM, LOGX>::NT)) void group_finish_kernel_persistent(const GroupFinishArgs A, const int nbatch,
                                                                                          const int ntiles) {
    using S = GFGeo<LOGM, LOGX>;
    using GM = typename S::GM;
    using GX = typename S::GX;
    using L = GFPersistentLds<LOGM, LOGX>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int M = 1 << LOGM, X = 1 << LOGX, T = S::T, PM = GM::P, PX = GX::P, NT = S::NT;
    static_assert(M <= NT, "one thread per window row");
    cx<float>* const tw_x = reinterpret_cast<cx<float>*>(smem + L::TW_X);
    cx<float>* const tw_m = reinterpret_cast<cx<float>*>(smem + L::TW_M);
    float* const fn = reinterpret_cast<float*>(smem + L::FN);
    int* const rows = reinterpret_cast<int*>(smem + L::ROWS);
    int tr = threadIdx.x >> 4, c16 = threadIdx.x & 15;
    const int ntx = (A.ncols + 15) >> 4;

    // (column tile, subgrid, group) of tile t: workgroup-uniform, kept in scalar registers
    auto decode = [&](int t, int& tx, int& b, int& g) {
        const int q = t / ntx;
        tx = __builtin_amdgcn_readfirstlane(t - q * ntx);
        g = __builtin_amdgcn_readfirstlane(q / nbatch);
        b = __builtin_amdgcn_readfirstlane(q - g * nbatch);
    };
    // window row ci (threads below M: ci = threadIdx.x) of a tile (tx, b): group_finish_kernel's in_row, once per thread-row
    auto window_row = [&](int tx, int b) { return gf_window_row<M>(A, gf_rowmap(A, tx), b, (int)threadIdx.x); };
    // the rows of facet entry n for tile (tx, b), whose window rows are in `rows`
    auto load_rows = [&](cx<float> (&dst)[PM], int n, int tx) {
        const int col = tx * 16 + c16;
        gf_load_rows(A, dst, gf_piece_column(A, tx, col), A.fidx[n], gf_facet_stride(A, tx), col,
                     [&](auto vI) { return rows[tr + decltype(vI)::value * T]; });
    };
    // every request for x has been answered from here on (the compiler's own wait would stand at x's first use: behind
    // the requests made in between, which the one counter then waits for too)
    auto touch = [](cx<float> (&v)[PM]) {
        static_for<0, PM>([&](auto vI) {
            const float re = v[decltype(vI)::value].x, im = v[decltype(vI)::value].y;
            asm volatile("" ::"v"(re), "v"(im) : "memory");
        });
    };

    int t = blockIdx.x, tx, b, g;
    if (t >= ntiles) return;
    decode(t, tx, b, g);
    for (int i = threadIdx.x; i < X; i += NT) tw_x[i] = A.tw_x[i];
    for (int i = threadIdx.x; i < M; i += NT) {
        tw_m[i] = A.tw_m[i];
        fn[i] = A.fn[i];
    }
    if (threadIdx.x < M) rows[threadIdx.x] = window_row(tx, b);
    __syncthreads();
    cx<float> x[PM], xn[PM];
    if (A.gstart[g] < A.gstart[g + 1]) load_rows(x, A.gstart[g], tx);
    touch(x);
    for (;;) {  // workgroup-uniform
        asm volatile("" : "+v"(tr), "+v"(c16));
        // the next tile's window rows: requested here, parked in LDS behind the facet loop
        const int t_next = t + gridDim.x;
        const bool more = t_next < ntiles;
        int tx_next = 0, b_next = 0, g_next = 0, row_next = 0;
        if (more) {
            decode(t_next, tx_next, b_next, g_next);
            if (threadIdx.x < M) row_next = window_row(tx_next, b_next);
        }
        cx<float> y[PX];
        static_for<0, PX>([&](auto vI) { y[decltype(vI)::value] = cx<float>{0.f, 0.f}; });
        const int n_end = A.gstart[g + 1];
        for (int n = A.gstart[g]; n < n_end; n++) {
            const int sp = A.sp0[n];
            if (n + 1 < n_end) load_rows(xn, n + 1, tx);
            fft_phases<GM, float, 0>(x, tr, c16, true, smem, tw_m, [&](int e, cx<float> v, auto sI) {
                place_output<GM, LOGX, decltype(sI)::value>(y, e, sp, v, fn);
            });
            static_for<0, PM>([&](auto vI) { x[decltype(vI)::value] = xn[decltype(vI)::value]; });
            touch(x);
        }

        // what the finishing tile's stores need
        const int col = tx * 16 + c16;
        const bool live = col < A.ncols;
        cx<float>* __restrict__ out = gf_out_column(A, col, b, g);
        const float* __restrict__ mask = gf_mask_row(A, b);
        const int st_a = A.st_a[b];
        // the next tile's first facet: in flight under the inverse transform.  (Every lane is behind the last barrier of
        // the facet loop, so behind every read of `rows`; every exchange ends with a barrier behind its gather and the last
        // phase touches no LDS, so nothing of x is in the exchange buffer)
        t = t_next; tx = tx_next; b = b_next; g = g_next;
        asm volatile("" ::"v"(row_next) : "memory");  // (its wait, for every lane: not left to the branch below)
        if (more) {
            if (threadIdx.x < M) rows[threadIdx.x] = row_next;
            __syncthreads();
            if (A.gstart[g] < A.gstart[g + 1]) load_rows(x, A.gstart[g], tx);
        }

        // ---- xM-point inverse transform (conj . FFT . conj), crop, mask0, store
        conj_regs(y);
        const float scale = 1.f / (float)X;
        cx<float> z[PX];
        int d[PX];
        fft_phases<GX, float, 0>(y, tr, c16, true, smem, tw_x, [&](int e, cx<float> v, auto sI) {
            z[decltype(sI)::value] = v;
            d[decltype(sI)::value] = crop_index<X>(e, st_a);
        });
        touch(x);
        float w[PX];
        static_for<0, PX>([&](auto sI) { w[decltype(sI)::value] = scale; });
        if (mask)  // (the rows the crop drops read the last entry of the mask row: in bounds, not used)
            static_for<0, PX>([&](auto sI) {
                constexpr int s = decltype(sI)::value;
                w[s] *= mask[d[s] < A.xA ? d[s] : A.xA - 1];
            });
        static_for<0, PX>([&](auto sI) {
            constexpr int s = decltype(sI)::value;
            if (d[s] < A.xA && live) cp_store<true>(out + (unsigned)d[s] * (unsigned)A.ncols, cx<float>{z[s].x * w[s], -z[s].y * w[s]});
        });
        if (!more) break;
    }
}

// grid_cap = 0: one workgroup per tile (group_finish_kernel); > 0: the persistent kernel on min(tiles, grid_cap) workgroups
int launch_group_finish(int logm, int logx, const GroupFinishArgs& a, int nbatch, int ngroups, int grid_cap, hipStream_t s);

}  // namespace swf
