// Offset-to-index-map geometry of libswiftly_hip.so: how an image offset (a facet's off0 / off1, a subgrid's off0 / off1, a
// band start) becomes the integers a kernel's index map takes, as pure host functions of the sizes and plain integers (no
// handle, no HIP header, no allocation; plain C++17).  Every launch sequence takes its map numbers from here, so the
// convention lives here once; tests/test_geometry_cpu.py pins it to the oracle's closed forms without a GPU.
//
// One rule gives the integers their meaning (AxisMap, swiftly_rows.h): a centred transform-domain index ci of a transform
// of length n maps to memory as
//     q = (ci + a) mod n ;  valid iff q < len ;  idx = (q + c) mod mod
// and the reference's primitives (core.py:189-484) are transforms with these maps on their load and store side:
//
//   primitive             core.py   n    load map                          store map
//   prepare_facet         189-222   yN   facet_in_padded_facet             whole(yN)
//   extract_from_facet    224-253   --   (no transform: the window of the subgrid offset, window_of / window_column)
//   add_to_subgrid        255-285   m    whole(m)                          contribution_in_padded_subgrid, window Fn[q]
//   finish_subgrid        287-325   xM   whole(xM)                         subgrid_in_padded_subgrid
//   prepare_subgrid       328-368   xM   subgrid_in_padded_subgrid         whole(xM)
//   extract_from_subgrid  370-406   m    contribution_in_padded_subgrid,   whole(m)
//                                        window Fn[q]
//   add_to_facet          408-449   --   (no transform: the same window, scattered)
//   finish_facet          452-484   yN   whole(yN), or band_as_load_map    facet_in_padded_facet
//
// Notation: yN padded facet size, yB facet size, xM padded subgrid size, xA subgrid size, m = xM * yN / N contribution
// size, s = floor(subgrid_off * yN / N), sp = floor(facet_off * xM / N).
#pragma once

#include <cstdint>

#include "swiftly_caps.h"  // Sizes

namespace swf {

static inline int64_t floordiv(int64_t a, int64_t b) {  // Python's //
    int64_t q = a / b;
    if ((a % b != 0) && ((a < 0) != (b < 0))) q--;
    return q;
}
static inline int pmod(int64_t a, int64_t n) {  // Python's %, n > 0
    int64_t r = a % n;
    if (r < 0) r += n;
    return (int)r;
}

struct Map {  // AxisMap (swiftly_rows.h) without the window pointers
    int a, len, c, mod;
};
inline Map whole(int64_t n) { return Map{0, (int)n, 0, (int)n}; }  // every index, where it is

// ---------------------------------------------------------------------------------------------------------
// the facet inside the padded facet (prepare_facet load, core.py:213-221; finish_facet store, core.py:475-484): pixel y of
// the facet is centred index (yN/2 - yB/2 + y + facet_off) mod yN.  `facet_lo`: where the facet's windows start in the
// yN-point tables (1 / pswf[lo + y]).
inline int facet_lo(const Sizes& z, int64_t yB) { return (int)z.yN / 2 - (int)(yB / 2); }
inline Map facet_in_padded_facet(const Sizes& z, int64_t yB, int64_t facet_off) {
    return Map{pmod(-(facet_off + facet_lo(z, yB)), z.yN), (int)yB, 0, (int)yB};
}

// the contribution inside the padded subgrid (add_to_subgrid store, core.py:274-285; extract_from_subgrid load,
// core.py:390-406): element q of the Fn-weighted contribution is centred index (q + sp) mod m of the m-point transform and
// lands on padded-subgrid index (q + xM/2 - m/2 + sp) mod xM
inline int64_t facet_shift(const Sizes& z, int64_t facet_off) { return floordiv(facet_off * z.xM, z.N); }  // sp
inline int placement_start(const Sizes& z, int64_t sp) { return pmod((int)z.xM / 2 - (int)z.m / 2 + sp, z.xM); }  // of q = 0
inline Map contribution_in_padded_subgrid(const Sizes& z, int64_t facet_off) {
    const int64_t sp = facet_shift(z, facet_off);
    return Map{pmod(-sp, z.m), (int)z.m, placement_start(z, sp), (int)z.xM};
}

// the subgrid inside the padded subgrid (finish_subgrid store, core.py:313-325; prepare_subgrid load, core.py:359-368):
// pixel i of the subgrid is centred index (xM/2 - xA/2 + i + subgrid_off) mod xM
inline Map subgrid_in_padded_subgrid(const Sizes& z, int64_t xA, int64_t subgrid_off) {
    return Map{pmod(-((int)z.xM / 2 - (int)xA / 2 + subgrid_off), z.xM), (int)xA, 0, (int)xA};
}

// ---------------------------------------------------------------------------------------------------------
// bands: element d of a band row is column (band_start + d) mod yN of the padded facet, d < band_len
inline bool band_valid(int64_t yN, int64_t band_start, int64_t band_len) {  // a cyclic range of [0, yN)
    return band_len > 0 && band_len <= yN && band_start >= 0 && band_start < yN;
}
// a band row as the input of a yN-point transform (do_finish_facet): the rest of the padded axis is zero
inline Map band_as_load_map(const Sizes& z, int64_t band_start, int64_t band_len) {
    return Map{pmod(-band_start, z.yN), (int)band_len, 0, (int)band_len};
}

// ---------------------------------------------------------------------------------------------------------
// the contribution window of a subgrid offset on the padded facet axis (extract_from_facet, core.py:243-253; add_to_facet,
// core.py:430-449): position q of the m-wide contribution holds padded-facet column
//     base + ((q + rot) mod m), wrapped at yN;    rot = (-s) mod m, base = (yN/2 - m/2 + s) mod yN
// (the tables that subtract instead of add take pmod(s, m))
struct Window {
    int64_t s;
    int rot, base;
};
inline Window window_of(const Sizes& z, int64_t subgrid_off) {
    const int64_t s = floordiv(subgrid_off * z.yN, z.N);
    return Window{s, pmod(-s, z.m), pmod((int)z.yN / 2 - (int)z.m / 2 + s, z.yN)};
}
inline int window_column(const Sizes& z, const Window& w, int64_t q) {
    const int col = w.base + (int)((q + w.rot) % z.m);
    return col >= z.yN ? col - (int)z.yN : col;
}
// Do the positions [first, first + count) of the window come from the band?  The first position that does not, or -1
// (the whole window: first = 0, count = m).
inline int64_t window_in_band(const Sizes& z, const Window& w, int64_t first, int64_t count, int64_t band_start,
                              int64_t band_len) {
    for (int64_t q = first; q < first + count; q++) {
        int d = window_column(z, w, q) - (int)band_start;
        if (d < 0) d += (int)z.yN;
        if (d >= band_len) return q;
    }
    return -1;
}

// ---------------------------------------------------------------------------------------------------------
// the kernels address one batch item with 32-bit ELEMENT offsets: the largest one, count * stride (+ extra), fits
inline bool offsets_fit_32(uint64_t count, uint64_t stride, uint64_t extra = 0) {
    return count * stride + extra < (uint64_t(1) << 32);
}

}  // namespace swf
