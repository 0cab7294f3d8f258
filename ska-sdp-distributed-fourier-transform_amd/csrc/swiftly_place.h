// SwiFTly on MI355X: the arithmetic that the forward subgrid-side kernels with a REGISTER accumulator share
// (sum_finish_facets_kernel's register form, swiftly_sumfinish.h; both group_finish kernels, swiftly_groupfinish.h),
// stated once.  The kernels differ in what is in flight when and in where their tables live, not in these lines: one
// bit changed here changes it in all of them.
//
// A lane owns the points t + T v of an m-point and of an xM-point transform (T threads per transform, PM = m / T and
// PX = xM / T points per lane).  Output e of the m-point transform is e = t (mod T), and its place in the padded axis,
// taken at its plain inverse-transform index p = (kk - m/2 + s') mod xM, is congruent to e modulo m: it lands in one of
// the SAME lane's inputs y[v] = axis[t + T v] of the xM-point transform, v = (e - t) / T + PM * c with c = p / m in
// [0, xM / m).  So add_to_subgrid's placement (core.py:274-285) is xM / m multiply-adds per output with the weights
// w * (c == c'), and the accumulator is the register image of the inverse transform's input.
#pragma once
#include "swiftly_fft.h"

namespace swf {

// y += weight(kk) * place(v): v is the value at centred index ck of an m-point axis, in slot SLOT of the lane's PM
// m-point slots; sp = s' of the facet or group; weight(kk) the weight of row kk
template <int LOGM, int LOGX, int SLOT, typename R, int PX, class Wt>
__device__ __forceinline__ void place_add(cx<R> (&y)[PX], int ck, int sp, cx<R> v, Wt&& weight) {
    constexpr int M = 1 << LOGM, X = 1 << LOGX, RATIO = X / M, PM = PX / RATIO;
    static_assert(PX == PM * RATIO && SLOT < PM, "accumulator slots");
    const int kk = (ck - sp) & (M - 1);            // row of G = Fn[kk] * F[(kk + s') mod m]
    const int p = (kk - (M >> 1) + sp) & (X - 1);  // plain inverse-transform index of the placed element
    const int c = p >> LOGM;
    const R w = weight(kk);
    static_for<0, RATIO>([&](auto cI) {
        constexpr int cc = decltype(cI)::value;
        const R wc = c == cc ? w : (R)0;
        y[SLOT + PM * cc].x += v.x * wc;
        y[SLOT + PM * cc].y += v.y * wc;
    });
}

// the `fin` of fft_phases<GM, R, 0>: output S (phase_scatter's slot number) = element e, weighted with fn[kk] and placed
template <class GM, int LOGX, int S, typename R, int PX, class FnP>
__device__ __forceinline__ void place_output(cx<R> (&y)[PX], int e, int sp, cx<R> v, FnP fn) {
    place_add<GM::LOGN, LOGX, last_phase_slot<GM>(S)>(y, e ^ (GM::N >> 1), sp, v, [&](int kk) { return fn[kk]; });
}

// inverse transform = conj . FFT . conj: the first conjugation, on the accumulator
template <typename R, int PX>
__device__ __forceinline__ void conj_regs(cx<R> (&y)[PX]) {
    static_for<0, PX>([&](auto vI) { y[decltype(vI)::value].y = -y[decltype(vI)::value].y; });
}
// finish_subgrid's crop (core.py:316-323): the output row / column of element e of the xM-point transform
// (st = (-(xM/2 - xA//2 + off)) mod xM; kept if below xA)
template <int X>
__device__ __forceinline__ int crop_index(int e, int st) {
    return ((e ^ (X >> 1)) + st) & (X - 1);
}

}  // namespace swf
