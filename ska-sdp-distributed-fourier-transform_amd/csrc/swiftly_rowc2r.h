// SwiFTly on MI355X: B8 (finish_facet along the contiguous axis of a band accumulator) for a REAL-valued facet as a
// HALF-LENGTH transform (swiftly_hip_finish_facet_band_c2r): the backward counterpart of swiftly_rowreal.h.
//
// Only y = Re FFT_N(X) of the band row X (N = 32768, plain index, zero outside the band) is wanted, and that is the transform
// of the Hermitian part of X.  With M = N / 2 and
//     2 H[k] = X[k] + conj X[(N - k) mod N]
//     2 Z[e] = (2 H[e] + 2 H[e + M]) + i W_N^e (2 H[e] - 2 H[e + M]) ,  e < M ,        z = FFT_M(Z)
// the output is y[2n] = Re z[n], y[2n + 1] = Im z[n] (the halves ride on the scale).  ONE workgroup per row (the band row
// kernel of swiftly_rowpass.h runs two, each loading the whole band row): 512 threads x 32 points, phases 32 . 32 . 16 of the
// engine in swiftly_fft.h, the split re/im exchange buffer (66 KB, two workgroups = two ROWS per CU at <= 128 VGPRs),
// preloaded twiddles from the compact sections.
// N = 65536 (RowC2RGeo64k): the same kernel on T = 1024 threads x 32 points, phases 32 . 32 . 32, a 132 KB exchange buffer
// (one workgroup per CU).  Everything below holds with T for 512 (runs of T consecutive indices are workgroup-uniform
// questions, a wave stores 512 contiguous bytes): the kernel needs 32 points per lane and N / T = 64, nothing else of the
// geometry.
//
// Load: the band row is [ld_len] complex64 in plain column order -- element d is centred column (band_start + d) mod N, i.e.
// plain k sits at d = (k + N/2 + ld_a) mod N with ld_a = -band_start mod N (band_as_load_map) -- read through buffer loads
// over a descriptor of exactly ld_len * 8 bytes (an absent row: an empty descriptor), so the range check supplies the zeros
// outside the band.  Lane t, register r holds e = t + 512 r and needs FOUR band elements:
//     X[e], X[e + M]  at  d1 = (e + N/2 + ld_a) mod N  and  d1 + M          (ascending with the lane)
//     X[(N - e) mod N], X[(M - e) mod N]  at  d3 = (N/2 - e + ld_a) mod N  and  d3 + M   (descending; e = 0: X[0] and X[M] again)
// straight from global memory: the band (92 KB on the 64k plan) does not fit beside the exchange buffer at two workgroups
// per CU.  The 512 indices of a (register, source) pair are consecutive, so whether the pair lies wholly outside the band is
// a WORKGROUP-uniform question: such a pair is not requested at all (a scalar branch; the load phase of these kernels is
// bound by the number of vector-memory instructions, swiftly_rowpass.h) -- on the plan's band 24 + 24 of the 4 x 32 pairs
// remain.  The registers go in chunks of CH: all kept loads of a chunk are requested, then recombined
//     2 Z[e] = (a + b) + conj(c + d) + i W_N^e ((a - b) + conj(c - d)) ,   W_N^e = W_N^t W_64^r
// (one table value per lane, mul_w64), eight VGPRs of sources shrinking to two.
//
// Store: that of finish_facet_band -- plain p is centred column (p + N/2) mod N, facet column (that + st_a) mod N, kept below
// st_len, times the ONE combined window (mask / pswf) and the scale -- as float32.  N/2, st_a and st_len are even (host-
// checked), so a lane's (y[2n], y[2n + 1]) is one aligned pair of facet columns: one 8-byte window pair and one 8-byte store,
// adjacent lanes adjacent pairs (512 contiguous bytes per wave).  The window pairs of CH outputs are requested together before
// their stores; both go through descriptors of exactly st_len * 4 bytes, whose range check is the crop to the facet: a pair
// at or beyond st_len reads no window and writes nothing.  No accumulate form.
#pragma once
#include "swiftly_rowpass.h"

namespace swf {

using RowC2RGeo = RGeoPreC<14, 5, true>;
using RowC2RGeo64k = RGeoPreC<15, 5, true>;  // 65536-point rows

template <class G>
__global__ __launch_bounds__(G::NT, 4) void row_c2r_band_kernel(const RowPassArgs A, const cx<float>* __restrict__ gin,
                                                                float* __restrict__ gout,
                                                                const float* __restrict__ st_win,
                                                                const cx<float>* __restrict__ tw,
                                                                const cx<float>* __restrict__ tw_full) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int P = G::P, T = G::T, M = G::N, N = 2 * G::N;
    static_assert(P == 32 && G::SPLIT, "32 points per lane, split exchange");
    static_assert(N / T == 64, "W_N^(T r) = W_64^r (mul_w64)");
    const int t = threadIdx.x;
    const int row = blockIdx.x;  // uniform; row r on XCD r mod 8
    int in_row = row;
    if (A.in_rowmap) in_row = A.in_rowmap[in_row];
    const bool dead = in_row < 0;  // row not present in a compacted input: treated as zeros
    if (dead) in_row = 0;
    in_row = __builtin_amdgcn_readfirstlane(in_row);
    const char* __restrict__ inb = reinterpret_cast<const char*>(gin + (long long)in_row * A.in_pitch);
    char* __restrict__ outb = reinterpret_cast<char*>(gout + (long long)__builtin_amdgcn_readfirstlane(row) * A.out_pitch);  // out_pitch counts reals

    // -- load + recombination: x[r] = 2 Z[t + T r] -----------------------------------------------------------------------
    cx<float> x[P];
    {
        const int len = dead ? 0 : A.ld_len;  // uniform
        const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(inb), (short)0, len << 3, 0x00020000);
        const int fb = (A.ld_a + (N >> 1)) & (N - 1);  // d of plain k = 0
        // (uniform) d of lane 0 of the ascending sources of register 0, of lane T - 1 of the descending ones
        const int up0 = fb, dn0 = (fb - (T - 1)) & (N - 1);
        const unsigned up8 = (unsigned)((fb + t) & (N - 1)) << 3, dn8 = (unsigned)((fb - t) & (N - 1)) << 3;
        const cx<float> wt = tw_full[t];  // W_N^t
        // a run of T consecutive d from `lo` on holds nothing of the band: it starts behind it and does not wrap into it
        auto outside = [&](int lo) { return lo >= len && lo + (T - 1) < N; };
        constexpr int CH = 8;
        constexpr unsigned MASK8 = (unsigned)((N << 3) - 1);
        static_for<0, P / CH>([&](auto cI) {
            constexpr int c0 = decltype(cI)::value * CH;
            f32x2 g[CH][4];
            static_for<0, CH>([&](auto iI) {
                constexpr int i = decltype(iI)::value, r = c0 + i;
                static_for<0, 4>([&](auto sI) {
                    constexpr int s = decltype(sI)::value;
                    constexpr int step = (s < 2 ? T * r : N - T * r) + (s & 1) * M;  // sources 1 and 3: M further on
                    const int lo = ((s < 2 ? up0 : dn0) + step) & (N - 1);
                    g[i][s] = f32x2{0.f, 0.f};
                    if (!outside(lo)) {
                        const unsigned off = ((s < 2 ? up8 : dn8) + ((unsigned)step << 3)) & MASK8;
                        g[i][s] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_in, (int)off, 0, 0));
                    }
                });
            });
            __builtin_amdgcn_sched_barrier(0);
            static_for<0, CH>([&](auto iI) {
                constexpr int i = decltype(iI)::value, r = c0 + i;
                const f32x2 cj = {1.f, -1.f};
                const f32x2 sum = (g[i][0] + g[i][1]) + (g[i][2] + g[i][3]) * cj;  // 2 (H[e] + H[e + M])
                const f32x2 dif = (g[i][0] - g[i][1]) + (g[i][2] - g[i][3]) * cj;  // 2 (H[e] - H[e + M])
                const cx<float> wd = mul_w64<float, r>(cmul(pkc(dif), wt));       // W_N^(t + T r) = W_N^t W_64^r
                // sum + i wd as (wd - i sum) * i, so that the chunk ends in one of the packed-arithmetic statements of
                // swiftly_fft.h: an expression the compiler may move is sunk into the block of its use -- the first butterflies
                // -- and takes the eight source registers of ALL chunks along (728 bytes of scratch)
                x[r] = pk_sub_pi(wd, cx<float>{-sum.y, sum.x});
            });
            __builtin_amdgcn_sched_barrier(0);
        });
    }

    // -- z = FFT_M(2 Z): z[t + T v] in register z[v] ---------------------------------------------------------------------
    cx<float> z[P];
    fft_phases<G, float, 0>(x, t, 0, false, smem, tw, [&](int, cx<float> v, auto sI) {
        z[last_phase_slot<G>(decltype(sI)::value)] = v;
    }, nullptr, A.twc);

    // -- store: (y[2n], y[2n + 1]) = (Re, Im) z[n], n = t + T v, at facet columns (2n + N/2 + st_a) mod N and the next ---------
    {
        const int flen = A.st_len;  // uniform, even
        const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(st_win), (short)0, flen << 2, 0x00020000);
        const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(outb, (short)0, flen << 2, 0x00020000);
        const float scale = 0.5f * A.scale;  // the halves of H
        const f32x2 sc = {scale, scale};
        const unsigned col4 = (unsigned)((2 * t + (N >> 1) + A.st_a) & (N - 1)) << 2;  // byte offset of the pair of v = 0
        constexpr unsigned MASK4 = (unsigned)((N << 2) - 1);
        constexpr int CH = 8;
        static_for<0, P / CH>([&](auto cI) {
            constexpr int c0 = decltype(cI)::value * CH;
            f32x2 w[CH];
            static_for<0, CH>([&](auto iI) {
                constexpr int i = decltype(iI)::value, v = c0 + i;
                const unsigned off = (col4 + (unsigned)((2 * T * v) << 2)) & MASK4;
                w[i] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_w, (int)off, 0, 0));
            });
            static_for<0, CH>([&](auto iI) {
                constexpr int i = decltype(iI)::value, v = c0 + i;
                const unsigned off = (col4 + (unsigned)((2 * T * v) << 2)) & MASK4;
                const f32x2 val = pkv(z[v]) * (w[i] * sc);
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, val), rs_out, (int)off, 0, 0);
            });
        });
    }
}

// B8 of `a.nrows` band rows of 2^log_yN = 32768 or 65536 points ([a.ld_len] complex64 at a.in, a.in_pitch in elements,
// a.ld_a = -band_start mod 2^log_yN) into float32 facet rows (a.out float32, a.out_pitch in reals, a.out_real set): a.st_a /
// a.st_len / a.out_pitch even and a.out 8-byte aligned (caller-checked), a.st_win the ONE combined window of st_len entries,
// tw_half / tw_full = the tables of length 2^(log_yN - 1) / 2^log_yN, a.twc = the compact twiddle sections of the half-length
// table for 32 points per lane.  Returns the launch status; -1: not this kernel's call (another row length included).
int launch_row_c2r_band(int log_yN, const RowPassArgs& a, const cx<float>* tw_half, const cx<float>* tw_full, hipStream_t s);
int row_c2r_band_occupancy(int log_yN = 15);  // workgroups per CU

}  // namespace swf
