// instantiations + dispatch of the lean column-tile pass (complex64; complex128 storage with float64 arithmetic)
#include <cstdlib>

#include "swiftly_colpass.h"
#include "swiftly_launch.h"

namespace swf {

// The single 512-point pass on 32-column tiles (ColPassArgs::tile32; r5): 512 threads and 64 KiB per workgroup instead of
// 1024 threads and 128 KiB.  Alone on the chip the two forms are equal (r3: 43.37 vs 43.29 ms per pass); in the overlapped
// wave loop K3 shares the CUs with the K2 workgroups of the following waves, which a whole-CU workgroup cannot: 64k pass
// 38.07 / 37.84 / 38.14 -> 37.79 / 37.68 / 37.95 ms (interleaved same-box pairs, gpurun_out/r5r).  SWIFTLY_COL512_TILE32=0
// switches it off (A/B runs).  (The same tiles for the two passes of K2's four-step, same session: pass A 38.2 / 37.6 ->
// 39.1 / 39.7 ms, pass B 37.7 / 38.4 -- not kept.)
using CGeo512Half = CGeo<9, 5, true, 32>;
static int col512_tile32() {
    static const int v = getenv("SWIFTLY_COL512_TILE32") ? atoi(getenv("SWIFTLY_COL512_TILE32")) : 1;
    return v;
}

// The piece-aware single pass (col_pass2_kernel, ColPassSrc2): the instances the forward slab path can reach -- complex64
// storage, plain mapped load; float arithmetic at 128 and 256 points (64-column tiles) and at 512 points on 32-column
// tiles, float64 arithmetic at 512 points.  Everything else has none: the caller launches once per piece.
bool col_pass_pieces_supported(int logn, const ColPassArgs& a) {
    if (a.c128 || a.gs || a.in_bdiv <= 0 || a.in_bs) return false;
    if (a.f64) return logn == 9 && a.twd;
    return logn == 7 || logn == 8 || (logn == 9 && a.tile32 && col512_tile32());
}
template <class G, typename RC>
static int launch_pieces(const ColPassArgs& a, const ColPassSrc2& s2, const ColZ& cz, int outer, int nbatch, hipStream_t s,
                         const cx<RC>* tw, const cx<RC>* tw_full) {
    dim3 grid((unsigned)((a.ncols + G::COLS - 1) / G::COLS), (unsigned)outer, (unsigned)nbatch);
    return launch_lds<col_pass2_kernel<G, RC>, G::LDS_BYTES>(grid, dim3(G::NT), s, a, s2, a.in, a.out, a.ld_win, a.ld_win2,
                                                             a.st_win, a.st_win2, a.st_rowmap, tw, tw_full, cz);
}
template <int LOGN>
static int launch_mode_pieces(const ColPassArgs& a, const ColPassSrc2& s2, const ColZ& cz, int outer, int nbatch,
                              hipStream_t s) {
    if (!col_pass_pieces_supported(LOGN, a)) return (int)hipErrorInvalidConfiguration;
    if constexpr (LOGN == 9) {
        if (a.f64) return launch_pieces<typename CGeoFor<9, double>::type, double>(a, s2, cz, outer, nbatch, s, a.twd, a.twd_full);
        return launch_pieces<CGeo512Half, float>(a, s2, cz, outer, nbatch, s, a.tw, a.tw_full);
    }
    if constexpr (LOGN == 7 || LOGN == 8)
        return launch_pieces<typename CGeoFor<LOGN>::type, float>(a, s2, cz, outer, nbatch, s, a.tw, a.tw_full);
    return (int)hipErrorInvalidConfiguration;
}

template <int LOGN, int MODE>
static int launch_mode(const ColPassArgs& a, const ColZ& cz, int outer, int nbatch, hipStream_t s) {
    using G = typename CGeoFor<LOGN>::type;
    if constexpr (LOGN == 9 && MODE == 2) {
        if (a.tile32 && !a.gs && col512_tile32()) {
            using GH = CGeo512Half;
            dim3 hgrid((unsigned)((a.ncols + GH::COLS - 1) / GH::COLS), (unsigned)outer, (unsigned)nbatch);
            return launch_lds<col_pass_kernel<GH, 2, true>, GH::LDS_BYTES>(hgrid, dim3(GH::NT), s, a, a.in, a.out, a.ld_win,
                                                                           a.ld_win2, a.st_win, a.st_win2, a.st_rowmap, a.tw,
                                                                           a.tw_full, cz);
        }
    }
    dim3 grid((unsigned)((a.ncols + G::COLS - 1) / G::COLS), (unsigned)outer, (unsigned)nbatch);
    if constexpr (MODE == 1 || G::HALF) {
        if (a.gs) return (int)hipErrorInvalidConfiguration;  // no gather-sum instance of this geometry: never fall through to the plain load
    }
    if constexpr (MODE != 1 && !G::HALF) {
        if (a.gs) {  // gather-sum load (backward pass); the source contributions are small and re-read: cacheable
            return launch_lds<col_pass_kernel<G, MODE, true, true>, G::LDS_BYTES>(grid, dim3(G::NT), s, a, a.in, a.out, a.ld_win,
                                                                                  a.ld_win2, a.st_win, a.st_win2, a.st_rowmap,
                                                                                  a.tw, a.tw_full, cz);
        }
    }
    if (MODE == 2 || a.scratch_nt)
        return launch_lds<col_pass_kernel<G, MODE, true>, G::LDS_BYTES>(grid, dim3(G::NT), s, a, a.in, a.out, a.ld_win, a.ld_win2,
                                                                        a.st_win, a.st_win2, a.st_rowmap, a.tw, a.tw_full, cz);
    return launch_lds<col_pass_kernel<G, (MODE == 2 ? 0 : MODE), false>, G::LDS_BYTES>(
        grid, dim3(G::NT), s, a, a.in, a.out, a.ld_win, a.ld_win2, a.st_win, a.st_win2, a.st_rowmap, a.tw, a.tw_full, cz);
}
// float64 arithmetic (ColPassArgs::f64): lengths 32 .. 512 (kColF64MinLog .. kColPassMaxLogF64, swiftly_rowroute.h)
template <int LOGN, int MODE>
static int launch_mode_f64(const ColPassArgs& a, const ColZ& cz, int outer, int nbatch, hipStream_t s) {
    if constexpr (LOGN < kColF64MinLog || LOGN > kColPassMaxLogF64) {
        return (int)hipErrorInvalidConfiguration;
    } else {
        using G = typename CGeoFor<LOGN, double>::type;
        if (!a.twd || (MODE == 0 && !a.twd_full)) return (int)hipErrorInvalidValue;
        if (a.gs) {
            using GG = typename CGeoFor<LOGN, double>::type_gs;
            if constexpr (MODE != 1 && !GG::HALF) {
                dim3 ggrid((unsigned)((a.ncols + GG::COLS - 1) / GG::COLS), (unsigned)outer, (unsigned)nbatch);
                return launch_lds<col_pass_kernel<GG, MODE, true, true, double>, GG::LDS_BYTES>(
                    ggrid, dim3(GG::NT), s, a, a.in, a.out, a.ld_win, a.ld_win2, a.st_win, a.st_win2, a.st_rowmap, a.twd,
                    a.twd_full, cz);
            } else {
                return (int)hipErrorInvalidConfiguration;
            }
        }
        dim3 grid((unsigned)((a.ncols + G::COLS - 1) / G::COLS), (unsigned)outer, (unsigned)nbatch);
        if (MODE == 2 || a.scratch_nt)
            return launch_lds<col_pass_kernel<G, MODE, true, false, double>, G::LDS_BYTES>(
                grid, dim3(G::NT), s, a, a.in, a.out, a.ld_win, a.ld_win2, a.st_win, a.st_win2, a.st_rowmap, a.twd, a.twd_full, cz);
        return launch_lds<col_pass_kernel<G, (MODE == 2 ? 0 : MODE), false, false, double>, G::LDS_BYTES>(
            grid, dim3(G::NT), s, a, a.in, a.out, a.ld_win, a.ld_win2, a.st_win, a.st_win2, a.st_rowmap, a.twd, a.twd_full, cz);
    }
}

// complex128 storage (ColPassArgs::c128): the float64-arithmetic geometries with cx<double> loads and stores; the LDS
// exchange already holds doubles, so the tiles and LDS sizes are those of launch_mode_f64 -- except 256 points, whose
// 64-column tile (1024 threads: 128 VGPRs at most) spills with 16-byte points: 32-column tiles, 512 threads, 64 KiB, and
// room for 256 VGPRs
template <int LOGN>
struct CGeoC128 : CGeoFor<LOGN, double>::type {};
template <>
struct CGeoC128<8> : CGeo<8, 4, true, 32, 8> {
    static constexpr int MINW = 2;
};
// Gather-sum load with complex128 storage (backward band schedule, accumulate_facet_columns): the same tiles.  Pass A of
// the four-steps of 1024 .. 32768 points (32 / 64 / 128 points) and the single passes of 64 .. 512 points; the 32-column
// tiles (128, 256 and 512 points) read their source rows per half-wave.
template <int LOGN, int MODE>
constexpr bool kColC128HasGs = (MODE == 0 && LOGN >= 5 && LOGN <= 7) || (MODE == 2 && LOGN >= 6 && LOGN <= kColPassMaxLogF64);
template <int LOGN, int MODE>
static int launch_mode_c128(const ColPassArgs& a, const ColZ& cz, int outer, int nbatch, hipStream_t s) {
    if constexpr (LOGN < kColF64MinLog || LOGN > kColPassMaxLogF64) {
        return (int)hipErrorInvalidConfiguration;
    } else {
        using G = CGeoC128<LOGN>;
        if (!a.twd || (MODE == 0 && !a.twd_full)) return (int)hipErrorInvalidValue;
        const cx<double>* in = reinterpret_cast<const cx<double>*>(a.in);
        cx<double>* out = reinterpret_cast<cx<double>*>(a.out);
        dim3 grid((unsigned)((a.ncols + G::COLS - 1) / G::COLS), (unsigned)outer, (unsigned)nbatch);
        if (a.gs) {  // never fall through to the plain load, which would read the encoded table as a row map
            if constexpr (kColC128HasGs<LOGN, MODE>) {
                return launch_lds<col_pass_kernel<G, MODE, true, true, double, double>, G::LDS_BYTES>(
                    grid, dim3(G::NT), s, a, in, out, a.ld_win, a.ld_win2, a.st_win, a.st_win2, a.st_rowmap, a.twd, a.twd_full, cz);
            } else {
                return (int)hipErrorInvalidConfiguration;
            }
        }
        if (MODE == 2 || a.scratch_nt)
            return launch_lds<col_pass_kernel<G, MODE, true, false, double, double>, G::LDS_BYTES>(
                grid, dim3(G::NT), s, a, in, out, a.ld_win, a.ld_win2, a.st_win, a.st_win2, a.st_rowmap, a.twd, a.twd_full, cz);
        return launch_lds<col_pass_kernel<G, (MODE == 2 ? 0 : MODE), false, false, double, double>, G::LDS_BYTES>(
            grid, dim3(G::NT), s, a, in, out, a.ld_win, a.ld_win2, a.st_win, a.st_win2, a.st_rowmap, a.twd, a.twd_full, cz);
    }
}

template <int LOGN>
static int launch_one(int mode, const ColPassArgs& a, const ColZ& cz, int outer, int nbatch, hipStream_t s,
                      const ColPassSrc2* src2) {
    if (src2) return mode == 2 ? launch_mode_pieces<LOGN>(a, *src2, cz, outer, nbatch, s) : (int)hipErrorInvalidConfiguration;
    if (a.c128) {
        if (mode == 0) return launch_mode_c128<LOGN, 0>(a, cz, outer, nbatch, s);
        if (mode == 1) return launch_mode_c128<LOGN, 1>(a, cz, outer, nbatch, s);
        return launch_mode_c128<LOGN, 2>(a, cz, outer, nbatch, s);
    }
    if (a.f64) {
        if (mode == 0) return launch_mode_f64<LOGN, 0>(a, cz, outer, nbatch, s);
        if (mode == 1) return launch_mode_f64<LOGN, 1>(a, cz, outer, nbatch, s);
        return launch_mode_f64<LOGN, 2>(a, cz, outer, nbatch, s);
    }
    if (mode == 0) return launch_mode<LOGN, 0>(a, cz, outer, nbatch, s);
    if (mode == 1) return launch_mode<LOGN, 1>(a, cz, outer, nbatch, s);
    return launch_mode<LOGN, 2>(a, cz, outer, nbatch, s);
}

template <int LO, int HI>
struct CDispatch {
    static int launch(int logn, int mode, const ColPassArgs& a, const ColZ& cz, int outer, int nbatch, hipStream_t s,
                      const ColPassSrc2* src2) {
        if (logn == LO) return launch_one<LO>(mode, a, cz, outer, nbatch, s, src2);
        if constexpr (LO < HI) return CDispatch<LO + 1, HI>::launch(logn, mode, a, cz, outer, nbatch, s, src2);
        return -1;
    }
};

int launch_col_pass(int logn, int mode, const ColPassArgs& a, const ColZ& cz, int outer, int nbatch, hipStream_t s,
                    const ColPassSrc2* src2) {
    return CDispatch<kColPassMinLog, kColPassMaxLog>::launch(logn, mode, a, cz, outer, nbatch, s, src2);
}
bool col_pass_f64_supported(int logn) { return col_f64_instance(logn); }

}  // namespace swf
