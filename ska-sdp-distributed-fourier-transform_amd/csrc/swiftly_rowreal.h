// SwiFTly on MI355X: K1 of a REAL-valued facet row as a HALF-LENGTH transform (swiftly_hip_prepare_facet_band_rfft).
//
// A real row x of N = 32768 points needs one complex transform of M = N / 2 points: with z[n] = x[2n] + i x[2n+1] and
// Z = FFT_M(z),
//     E[e] = (Z[e] + conj Z[M - e]) / 2      (transform of the even samples)
//     O[e] = (Z[e] - conj Z[M - e]) / (2 i)  (transform of the odd samples)
//     S[e] = E[e] + W_N^e O[e] ,  S[e + M] = E[e] - W_N^e O[e] ,  e < M .
// ONE workgroup per row (the band row kernel of swiftly_rowpass.h runs two, each loading and windowing the whole row):
// 512 threads x 32 points, phases 32 . 32 . 16 of the engine in swiftly_fft.h, the split re/im exchange buffer (66 KB,
// two workgroups per CU at <= 128 VGPRs), preloaded twiddles from the compact sections.
// N = 65536 (RowRealGeo64k): the same kernel on T = 1024 threads x 32 points, phases 32 . 32 . 32, a 132 KB exchange buffer
// (one workgroup per CU).  Everything below holds with T for 512: the kernel needs 32 points per lane, N / T = 64 and
// padded exchange positions that are affine in the register, nothing else of the geometry.
//
// Load: the map of a prepare_* primitive as the PAIR / REAL = 1 instances read it -- plain index p is element
// q = ((p + N/2) mod N + ld_a) mod N of the row, window ld_win[q], zero for q >= ld_len -- through buffer loads whose
// descriptors cover exactly ld_len * 4 bytes (an absent row: an empty descriptor).  Lane t, register r holds
// z[t + 512 r] from ONE 8-byte data load and one 8-byte window pair; ld_a, ld_len and the row pitch even and the base
// 8-byte aligned (host-checked).  Empty segments are skipped by the descriptors alone (no rotation, no output phase):
// their loads touch no memory, and the arithmetic on their zeros is 10 of 32 first-stage inputs of a 22528-point facet.
//
// Mirror exchange: lane t holds the outputs e = t + 512 v and needs Z[(M - e) mod M] -- lane 512 - t, register 31 - v
// for t > 0; lane 0, register (32 - v) mod 32 for t = 0.  The exchange buffer is free after the last gather and holds
// one component at a time: the real parts go round first and become a + c and a - c in registers (a = Re Z[e],
// c = Re Z[M - e]), then the imaginary parts b, whose mirrors d are read in chunks of eight that are recombined and
// stored at once -- 96 live values plus a chunk, never Z and its whole mirror:
//     2 E = (a + c, b - d) ,  2 O = (b + d, -(a - c)) .
// W_N^e = W_N^t (one table value per lane) times the compile-time constant W_64^v.
//
// Store: what swiftly_hip_prepare_facet_band_rows_real defines -- the inverse-transform convention of prepare_facet (for
// a real row: the conjugate of the forward transform), scale, the folded window of the other axis -- in the parity-split
// band layout: output k has centred index c = (k + N/2) mod N, d = (c - band_start) mod N, kept when d < band_len at
// column (d & 1) * band_half + (d >> 1).  A wave's 64 outputs of one register are 64 consecutive d, so for all but at
// most two registers per half the whole wave is inside or outside the band: that decision is scalar.
#pragma once
#include "swiftly_rowpass.h"

namespace swf {

using RowRealGeo = RGeoPreC<14, 5, true>;
using RowRealGeo64k = RGeoPreC<15, 5, true>;  // 65536-point rows

template <class G>
__global__ __launch_bounds__(G::NT, 4) void row_real_band_kernel(const RowPassArgs A, const float* __restrict__ gin,
                                                                 cx<float>* __restrict__ gout,
                                                                 const float* __restrict__ ld_win,
                                                                 const cx<float>* __restrict__ tw,
                                                                 const cx<float>* __restrict__ tw_full) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int P = G::P, T = G::T, M = G::N, N = 2 * G::N;
    static_assert(P == 32 && G::SPLIT, "32 points per lane (registers v and 31 - v mirror each other), split exchange");
    static_assert(N / T == 64, "W_N^(T v) = W_64^v (mul_w64)");
    constexpr int VSTEP = T + (T >> G::LOGPAD);  // exchange-buffer distance of e and e + T
    static_assert((T & ((1 << G::LOGPAD) - 1)) == 0 && (size_t)G::PITCH * 4 == G::LDS_BYTES, "padded positions are affine in the register");
    const int t = threadIdx.x;
    const int row = blockIdx.x;  // uniform; row r on XCD r mod 8 like the two halves of the band row kernel
    int in_row = row;
    if (A.rm_mod > 0) {
        int r1 = row + A.rm_inner;
        if (r1 >= A.rm_mod) r1 -= A.rm_mod;
        r1 += A.rm_outer;
        if (r1 >= A.rm_full) r1 -= A.rm_full;
        in_row = r1;
    }
    if (A.in_rowmap) in_row = A.in_rowmap[in_row];
    const bool dead = in_row < 0;  // row not present in a compacted input: treated as zeros
    if (dead) in_row = 0;
    in_row = __builtin_amdgcn_readfirstlane(in_row);
    const char* __restrict__ inb = reinterpret_cast<const char*>(gin + (long long)in_row * A.in_pitch);  // in_pitch counts reals
    char* __restrict__ outb = reinterpret_cast<char*>(gout + (long long)__builtin_amdgcn_readfirstlane(row) * A.out_pitch);

    // -- load + window: z[t + T r] = (x[q] w[q], x[q+1] w[q+1]), q = (2 (t + T r) + N/2 + ld_a) mod N ------------------
    cx<float> x[P];
    {
        const unsigned valid = dead ? 0u : (unsigned)A.ld_len;
        const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(inb), (short)0, (int)(valid << 2), 0x00020000);
        const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ld_win), (short)0, (int)(valid << 2), 0x00020000);
        const unsigned base4 = (unsigned)((2 * t + A.ld_a + (N >> 1)) & (N - 1)) << 2;
        // explicit load pipeline (as the W4 instances of the band row kernel): PIPE groups of one data and one window pair
        // are requested at once, every group consumed (4 VGPRs shrink to 2) makes room for the next request
        constexpr int PIPE = 12;
        f32x2 gd[P], gw[P];
        auto issue = [&](auto rI) {
            constexpr int r = decltype(rI)::value;
            const unsigned off = (base4 + (unsigned)((2 * T * r) << 2)) & (unsigned)((N << 2) - 1);
            gd[r] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_in, (int)off, 0, 0));
            gw[r] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_w, (int)off, 0, 0));
        };
        static_for<0, PIPE>(issue);
        __builtin_amdgcn_sched_barrier(0);
        static_for<0, P>([&](auto rI) {
            constexpr int r = decltype(rI)::value;
            x[r] = pkc(gd[r] * gw[r]);
            if constexpr (r + PIPE < P) issue(std::integral_constant<int, r + PIPE>{});
            __builtin_amdgcn_sched_barrier(0);
        });
    }

    // -- Z = FFT_M(z): Z[t + T v] in register z[v] -----------------------------------------------------------------------
    cx<float> z[P];
    fft_phases<G, float, 0>(x, t, 0, false, smem, tw, [&](int, cx<float> v, auto sI) {
        z[last_phase_slot<G>(decltype(sI)::value)] = v;
    }, nullptr, A.twc);

    // -- mirror exchange, real parts: a -> (a + c, a - c) --------------------------------------------------------------
    float* buf = reinterpret_cast<float*>(smem);
    const int pw = t + (t >> G::LOGPAD);               // position of e = t (+ VSTEP v)
    const int mb = T - t;                              // mirror of e = t + T v: mb + T (31 - v); t = 0: T (32 - v), 0 for v = 0
    const int pm = mb + (mb >> G::LOGPAD);
    // An LDS instruction carries a 16-bit byte offset.  Positions further than that from the lane's base -- none in the
    // 66 KB buffer of T = 512, registers 16 .. 31 in the 132 KB buffer of T = 1024 -- are addressed from a SECOND base,
    // VFAR registers on, which an empty asm statement keeps in one register: left alone the compiler holds an address
    // register per far position through the exchange (T = 1024: 40 bytes of scratch).
    constexpr int VFAR = (size_t)VSTEP * (P - 1) * 4 > 0xffff ? P / 2 : P;
    static_assert(VSTEP * (VFAR - 1) * 4 <= 0xffff && VSTEP * (P - 1 - VFAR) * 4 <= 0xffff, "LDS offsets");
    int pw_far = 0, pm_far = 0;
    if constexpr (VFAR < P) {
        pw_far = pw + VSTEP * VFAR;
        pm_far = pm + VSTEP * VFAR;
        asm("" : "+v"(pw_far), "+v"(pm_far));
    }
    auto own = [&](auto vI) {  // position of e = t + T v
        constexpr int v = decltype(vI)::value;
        if constexpr (v < VFAR)
            return pw + VSTEP * v;
        else
            return pw_far + VSTEP * (v - VFAR);
    };
    auto mirror = [&](auto vI) {  // position of M - e for t > 0 (and of T (32 - v) for t = 0, v > 0)
        constexpr int k = P - 1 - decltype(vI)::value;
        if constexpr (k < VFAR)
            return pm + VSTEP * k;
        else
            return pm_far + VSTEP * (k - VFAR);
    };
    const int pm0 = t == 0 ? 0 : mirror(std::integral_constant<int, 0>{});  // v = 0
    // (the last gather of fft_phases ends with a barrier: the buffer is free)
    static_for<0, P>([&](auto vI) {
        constexpr int v = decltype(vI)::value;
        buf[own(vI)] = z[v].x;
    });
    __syncthreads();
    float dm[P];  // a - c
    static_for<0, P>([&](auto vI) {
        constexpr int v = decltype(vI)::value;
        float c;
        if constexpr (v == 0)
            c = buf[pm0];
        else
            c = buf[mirror(vI)];
        dm[v] = z[v].x - c;
        z[v].x += c;
    });
    __syncthreads();
    static_for<0, P>([&](auto vI) {
        constexpr int v = decltype(vI)::value;
        buf[own(vI)] = z[v].y;
    });
    __syncthreads();

    // -- recombination and band store, in chunks of CH registers ----------------------------------------------------------
    float scale = 0.5f * A.scale;  // the halves of E and O
    if (A.row_win) scale *= A.row_win[row];
    const f32x2 sc = {scale, -scale};  // conjugate: the inverse-transform convention on a real row
    const cx<float> wt = tw_full[t];   // W_N^t
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int lane = t & 63;
    const int dw = ((wave << 6) + (N >> 1) - A.band_start) & (N - 1);  // d of lane 0, register 0, first half
    const unsigned half8 = (unsigned)A.band_half << 3;
    auto outside = [&](int base) { return base >= A.band_len && base + 63 < N; };  // base: wave-uniform d of lane 0
    auto store = [&](int base, cx<float> s) {
        if (outside(base)) return;
        const int d = (base + lane) & (N - 1);
        const f32x2 val = pkv(s) * sc;
        if (d < A.band_len) *reinterpret_cast<f32x2*>(outb + ((d & 1) ? half8 : 0u) + ((unsigned)(d >> 1) << 3)) = val;
    };
    // (a wave-uniform skip of the whole recombination of a pair (e, e + M) neither of whose halves the wave keeps -- 30 % of
    // the pairs on the 64k plan's band -- was measured SLOWER: 0.93 instead of 0.88 of the real two-workgroup form, each in
    // its own process, profiles/r19_k1_rfft_timing_pair_skip_variant.json; the branches fence the chunk's LDS reads.  Not kept.)
    constexpr int CH = 8;
    static_for<0, P / CH>([&](auto cI) {
        constexpr int c0 = decltype(cI)::value * CH;
        float dmir[CH];
        static_for<0, CH>([&](auto iI) {
            constexpr int v = c0 + decltype(iI)::value;
            if constexpr (v == 0)
                dmir[0] = buf[pm0];
            else
                dmir[v - c0] = buf[mirror(std::integral_constant<int, v>{})];
        });
        static_for<0, CH>([&](auto iI) {
            constexpr int v = c0 + decltype(iI)::value;
            const int base = (dw + T * v) & (N - 1), base_m = (base + M) & (N - 1);
            const float b = z[v].y, d = dmir[v - c0];
            const cx<float> e2 = {z[v].x, b - d};   // 2 E
            const cx<float> o2 = {b + d, -dm[v]};   // 2 O
            const cx<float> wo = mul_w64<float, v>(cmul(o2, wt));  // W_N^(t + T v) = W_N^t W_64^v
            store(base, e2 + wo);    // k = e
            store(base_m, e2 - wo);  // k = e + M
        });
    });
}

// K1 of `a.nrows` real rows of 2^log_yN = 32768 or 65536 points into the parity-split band (a.band_len > 0): a.in float32,
// a.in_pitch in reals, a.ld_a / a.ld_len / a.in_pitch even and a.in 8-byte aligned (caller-checked), tw_half / tw_full = the
// tables of length 2^(log_yN - 1) / 2^log_yN, a.twc = the compact twiddle sections of the half-length table for 32 points
// per lane.  Returns the launch status; -1: not this kernel's call (another row length included).
int launch_row_real_band(int log_yN, const RowPassArgs& a, const cx<float>* tw_half, const cx<float>* tw_full, hipStream_t s);
int row_real_band_occupancy(int log_yN = 15);  // workgroups per CU

}  // namespace swf
