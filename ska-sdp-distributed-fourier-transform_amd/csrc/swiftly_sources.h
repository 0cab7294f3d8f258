// SwiFTly on MI355X: point-source truths on the device (reference fourier_algorithm.py:218-315, api_helper.py:39-70).
//
// Subgrid side: the direct Fourier sum of S point sources on a batch of subgrids of one size,
//     T[b][u0, u1] = mask0_b[u0] * mask1_b[u1] * N^-2 sum_s I_s * P0[s][u0] * P1[s][u1],
//     P[s][u] = exp(2 pi i * ((c_s * (off - size//2 + u)) mod N) / N)                        (make_subgrid_from_sources)
// as a tiled complex float64 product [size x S] . [S x size], either stored or compared with the caller's subgrid
// without ever being stored (check_subgrid).  The phase is reduced EXACTLY: product and modulus in 64-bit integers
// (|c| <= N/2, 0 <= u < N <= 2^31, so |c * u| < 2^61), then one sincospi of 2 r / N with |r| <= N/2 -- the reference's
// exp(2 pi i c u / N) in double carries a phase error of ~ eps * pi * c * u / N, 1e5 ulp of the result at N = 131072.
// No recurrences: every table entry is evaluated from its own reduced integer.
//
// Facet side: the sources scattered onto a facet (make_facet_from_sources) and the streaming sum of |truth - approx|^2
// over a whole facet (check_facet), the sources of a row found through per-row lists built by the caller.
//
// All arithmetic is float64 whatever the dtype of the output / the approximation; complex64 is rounded once on store
// and widened exactly on load.  Every reduction runs in a fixed order (no floating-point atomics): results are
// bit-reproducible from run to run.
//
// Real-valued images: the three facet kernels also take float / double elements.  The store writes Re(I) * mask0 * mask1,
// the check takes the truth's imaginary part as zero and adds the squares in the order of the complex kernel, whose
// sums for a facet with zero imaginary parts it reproduces bit for bit.
#pragma once
#include <stdint.h>

#include <type_traits>

#include "swiftly_fft.h"  // cx<R>

namespace swf {

// One record of the device source table (24 bytes, 8-byte aligned).  The caller normalises the table: coordinates are
// reduced into [-N/2, N/2), no two records share a pixel.
struct SourceRec {
    double re, im;   // complex intensity
    int32_t c0, c1;  // image coordinates relative to the image centre, axis 0 / axis 1
};
static_assert(sizeof(SourceRec) == 24, "the Python layer builds the table with this layout");

constexpr int kSrcTile = 64;      // output tile: kSrcTile x kSrcTile pixels per workgroup
constexpr int kSrcThreads = 256;  // 16 x 16 threads, 4 x 4 pixels each (stride 16: stores coalesce along u1)
constexpr int kSrcChunk = 16;     // sources staged per LDS round: 2 * 16 * 64 complex doubles = 32 KB
constexpr int kSrcPix = kSrcTile / 16;

// (a mod n) in [0, n)
__host__ __device__ __forceinline__ long long src_pmod(long long a, long long n) {
    const long long r = a % n;
    return r < 0 ? r + n : r;
}

// exp(2 pi i * ((c * u) mod N) / N) for 0 <= u < N, |c| <= N / 2
__device__ __forceinline__ cx<double> src_phase(long long c, long long u, long long N) {
    long long r = src_pmod(c * u, N);
    if (2 * r > N) r -= N;  // |angle| <= pi: 2 r / N is one correctly rounded quotient in [-1, 1]
    double s, co;
    sincospi(2.0 * (double)r / (double)N, &s, &co);
    return {co, s};
}

struct SrcPhaseArgs {
    const SourceRec* src;
    const long long* offs;  // [ndistinct] first pixel of the axis, (off - size // 2) mod N
    cx<double>* out;        // [ndistinct][S][size]
    long long N;
    int S, size;
};
// grid (ceil(size / 256) * S, ndistinct).  AXIS: which coordinate of the records
template <int AXIS>
__global__ void __launch_bounds__(256) src_phase_kernel(SrcPhaseArgs a) {
    const int per_row = (a.size + 255) / 256;
    const int u = (int)(blockIdx.x % per_row) * 256 + (int)threadIdx.x, s = (int)(blockIdx.x / per_row), d = (int)blockIdx.y;
    if (u >= a.size) return;
    const long long c = AXIS ? a.src[s].c1 : a.src[s].c0;
    const long long uu = src_pmod(a.offs[d] + u, a.N);
    a.out[((size_t)d * a.S + s) * (size_t)a.size + u] = src_phase(c, uu, a.N);
}

struct SrcSubgridArgs {
    const SourceRec* src;
    const cx<double>* p0;  // [nd0][S][size]
    const cx<double>* p1;  // [nd1][S][size]
    const int32_t* idx0;   // [nsub] which table of p0 / p1 a subgrid uses
    const int32_t* idx1;
    const double* mask0;   // optional [nsub][size]
    const double* mask1;
    void* data;            // store: out; check: the caller's approximation (read only)
    long long sub_stride, row_stride;  // of `data`, in complex elements
    double* partials;      // check: [nsub][tiles][2] = sum |T - approx|^2, sum |T|^2 of a tile
    double inv_n2;         // N^-2
    int S, size, tiles;    // tiles per axis
};

// block-wide sum of two values in a fixed order: butterfly inside each wave, then the waves one after the other
__device__ __forceinline__ void src_block_sum2(double& a, double& b, double* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    const int w = (int)threadIdx.x >> 6, nw = (int)blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        lds[2 * w] = a;
        lds[2 * w + 1] = b;
    }
    __syncthreads();
    a = lds[0];
    b = lds[1];
    for (int k = 1; k < nw; k++) {
        a += lds[2 * k];
        b += lds[2 * k + 1];
    }
}

// grid (tiles * tiles, nsub).  OUT: cx<float> | cx<double>, the element type of `data`.
template <typename OUT, bool CHECK>
__global__ void __launch_bounds__(kSrcThreads) src_subgrid_kernel(SrcSubgridArgs a) {
    __shared__ cx<double> sa[kSrcChunk][kSrcTile];  // I_s / N^2 * P0[s][u0]
    __shared__ cx<double> sb[kSrcChunk][kSrcTile];  // P1[s][u1]
    __shared__ double red[2 * (kSrcThreads / 64)];
    const int t = (int)threadIdx.x, tx = t & 15, ty = t >> 4;
    const int b = (int)blockIdx.y;
    const int u0_0 = ((int)blockIdx.x / a.tiles) * kSrcTile, u1_0 = ((int)blockIdx.x % a.tiles) * kSrcTile;
    const cx<double>* p0 = a.p0 + (size_t)a.idx0[b] * a.S * (size_t)a.size;
    const cx<double>* p1 = a.p1 + (size_t)a.idx1[b] * a.S * (size_t)a.size;

    cx<double> acc[kSrcPix][kSrcPix];
#pragma unroll
    for (int i = 0; i < kSrcPix; i++)
#pragma unroll
        for (int j = 0; j < kSrcPix; j++) acc[i][j] = {0.0, 0.0};

    for (int s0 = 0; s0 < a.S; s0 += kSrcChunk) {
        const int kn = min(kSrcChunk, a.S - s0);  // ragged last chunk
        __syncthreads();
        for (int e = t; e < kn * kSrcTile; e += kSrcThreads) {
            const int k = e / kSrcTile, u = e % kSrcTile;
            const SourceRec r = a.src[s0 + k];
            const cx<double> w = {r.re * a.inv_n2, r.im * a.inv_n2};
            const cx<double> zero = {0.0, 0.0};  // ragged last tile: zeros, the stores are guarded too
            sa[k][u] = u0_0 + u < a.size ? cmul(w, p0[(size_t)(s0 + k) * a.size + u0_0 + u]) : zero;
            sb[k][u] = u1_0 + u < a.size ? p1[(size_t)(s0 + k) * a.size + u1_0 + u] : zero;
        }
        __syncthreads();
        for (int k = 0; k < kn; k++) {
            cx<double> va[kSrcPix], vb[kSrcPix];
#pragma unroll
            for (int i = 0; i < kSrcPix; i++) {
                va[i] = sa[k][ty + 16 * i];
                vb[i] = sb[k][tx + 16 * i];
            }
#pragma unroll
            for (int i = 0; i < kSrcPix; i++)
#pragma unroll
                for (int j = 0; j < kSrcPix; j++) {
                    acc[i][j].x += va[i].x * vb[j].x - va[i].y * vb[j].y;
                    acc[i][j].y += va[i].x * vb[j].y + va[i].y * vb[j].x;
                }
        }
    }

    double res = 0.0, tru = 0.0;
    OUT* data = (OUT*)a.data + (size_t)b * a.sub_stride;
#pragma unroll
    for (int i = 0; i < kSrcPix; i++) {
        const int u0 = u0_0 + ty + 16 * i;
        if (u0 >= a.size) continue;
        const double m0 = a.mask0 ? a.mask0[(size_t)b * a.size + u0] : 1.0;
#pragma unroll
        for (int j = 0; j < kSrcPix; j++) {
            const int u1 = u1_0 + tx + 16 * j;
            if (u1 >= a.size) continue;
            const double m = m0 * (a.mask1 ? a.mask1[(size_t)b * a.size + u1] : 1.0);
            const double tr = acc[i][j].x * m, ti = acc[i][j].y * m;
            OUT* p = data + (size_t)u0 * a.row_stride + u1;
            if constexpr (CHECK) {
                const OUT v = *p;
                const double dr = tr - (double)v.x, di = ti - (double)v.y;
                res += dr * dr + di * di;
                tru += tr * tr + ti * ti;
            } else {
                *p = OUT{(decltype(p->x))tr, (decltype(p->x))ti};
            }
        }
    }
    if constexpr (CHECK) {
        src_block_sum2(res, tru, red);
        if (t == 0) {
            double* o = a.partials + ((size_t)b * gridDim.x + blockIdx.x) * 2;
            o[0] = res;
            o[1] = tru;
        }
    }
}

// out[item][0 .. 1] = the sums of partials[item][0 .. n)[0 .. 1], always in the same order.  grid (nitems), one wave.
template <int NT = 64>
__global__ void __launch_bounds__(NT) src_sum_partials_kernel(const double* partials, long long n, double* out) {
    const double* p = partials + (size_t)blockIdx.x * (size_t)n * 2;
    double a = 0.0, b = 0.0;
    for (long long k = threadIdx.x; k < n; k += NT) {
        a += p[2 * k];
        b += p[2 * k + 1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    if (threadIdx.x == 0) {
        out[2 * (size_t)blockIdx.x] = a;
        out[2 * (size_t)blockIdx.x + 1] = b;
    }
}

struct SrcFacetArgs {
    const SourceRec* src;
    const double* mask0;  // optional [size]
    const double* mask1;
    void* data;           // store: out; check: the caller's approximation (read only)
    long long row_stride;
    long long N, org0, org1;  // first pixel of the facet per axis: (off - size // 2) mod N
    int S, size;
    // check: the sources of row r are row_srcs[row_start[r] .. row_start[r + 1]), ascending in their column
    const int32_t* row_start;
    const int32_t* row_srcs;
    double* partials;  // [size][2]
};

// element types of a facet: cx<float> / cx<double>, or float / double for a real-valued image
template <typename OUT>
constexpr bool kSrcReal = std::is_floating_point<OUT>::value;
// (re, im) rounded once to OUT; a real element keeps re
template <typename OUT>
__device__ __forceinline__ OUT src_elem(double re, double im) {
    if constexpr (kSrcReal<OUT>) return (OUT)re;
    else return OUT{(decltype(OUT::x))re, (decltype(OUT::x))im};
}

// facet pixel of a source along one axis (reference fourier_algorithm.py:253-256): inside the facet when < size
__device__ __forceinline__ long long src_pixel(long long c, long long org, long long N) { return src_pmod(c - org, N); }

// grid (ceil(size / 256) * size): zero fill of a strided facet
template <typename OUT>
__global__ void __launch_bounds__(256) src_facet_zero_kernel(SrcFacetArgs a) {
    const int per_row = (a.size + 255) / 256;
    const int c = (int)(blockIdx.x % per_row) * 256 + (int)threadIdx.x, row = (int)(blockIdx.x / per_row);
    if (c < a.size) ((OUT*)a.data)[(size_t)row * a.row_stride + c] = src_elem<OUT>(0.0, 0.0);
}
// grid (ceil(S / 256)): one source per thread; sources sit on distinct pixels, so plain stores suffice
template <typename OUT>
__global__ void __launch_bounds__(256) src_facet_store_kernel(SrcFacetArgs a) {
    const int s = (int)(blockIdx.x * 256 + threadIdx.x);
    if (s >= a.S) return;
    const SourceRec r = a.src[s];
    const long long q0 = src_pixel(r.c0, a.org0, a.N), q1 = src_pixel(r.c1, a.org1, a.N);
    if (q0 >= a.size || q1 >= a.size) return;
    const double m0 = a.mask0 ? a.mask0[q0] : 1.0, m1 = a.mask1 ? a.mask1[q1] : 1.0;
    // (I * mask0) * mask1 per component, the order the reference multiplies in
    ((OUT*)a.data)[(size_t)q0 * a.row_stride + q1] = src_elem<OUT>(r.re * m0 * m1, r.im * m0 * m1);
}
// grid (size): one workgroup streams one row and sums |truth - approx|^2 pixel by pixel -- never sum |approx|^2 with
// corrections at the source pixels, which cancels completely for an approximation that is right to 1e-10
template <typename OUT>
__global__ void __launch_bounds__(256) src_facet_check_kernel(SrcFacetArgs a) {
    __shared__ double red[2 * 4];
    const int row = (int)blockIdx.x;
    const int lo0 = a.row_start[row], hi0 = a.row_start[row + 1];
    const OUT* p = (const OUT*)a.data + (size_t)row * a.row_stride;
    const double m0 = a.mask0 ? a.mask0[row] : 1.0;
    double res = 0.0, tru = 0.0;
    for (int c = (int)threadIdx.x; c < a.size; c += 256) {
        double tr = 0.0, ti = 0.0;
        int lo = lo0, hi = hi0;  // first list entry whose column is >= c
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (src_pixel(a.src[a.row_srcs[mid]].c1, a.org1, a.N) < c) lo = mid + 1;
            else hi = mid;
        }
        if (lo < hi0) {
            const SourceRec r = a.src[a.row_srcs[lo]];
            if (src_pixel(r.c1, a.org1, a.N) == c && src_pixel(r.c0, a.org0, a.N) == row) {
                const double m1 = a.mask1 ? a.mask1[c] : 1.0;
                tr = r.re * m0 * m1;
                ti = r.im * m0 * m1;
            }
        }
        if constexpr (kSrcReal<OUT>) {
            // the complex kernel on zero imaginary parts adds round(dr * dr) [+ 0]: the product is rounded on its own
            // here too, never contracted into the running sum
#pragma clang fp contract(off)
            const double dr = tr - (double)p[c];
            const double d2 = dr * dr, t2 = tr * tr;
            res += d2;
            tru += t2;
        } else {
            const OUT v = p[c];
            const double dr = tr - (double)v.x, di = ti - (double)v.y;
            res += dr * dr + di * di;
            tru += tr * tr + ti * ti;
        }
    }
    src_block_sum2(res, tru, red);
    if (threadIdx.x == 0) {
        a.partials[2 * (size_t)row] = res;
        a.partials[2 * (size_t)row + 1] = tru;
    }
}

// launchers (sources.hip); return a hipError_t as int
int launch_src_phase(const SrcPhaseArgs& a, int axis, int ndistinct, hipStream_t st);
int launch_src_subgrids(const SrcSubgridArgs& a, int nsub, bool c128, bool check, hipStream_t st);
int launch_src_sum_partials(const double* partials, long long n, int nitems, double* out, hipStream_t st);
// (real: the elements of a.data are float / double instead of cx<float> / cx<double>)
int launch_src_facet_store(const SrcFacetArgs& a, bool c128, bool real, hipStream_t st);
int launch_src_facet_check(const SrcFacetArgs& a, bool c128, bool real, hipStream_t st);

}  // namespace swf
