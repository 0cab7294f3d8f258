// Which kernel family a row transform of the C ABI runs (run_rows / run_rows_chunk, swiftly_abi.hip), as pure host functions
// of integers and booleans (no HIP, no environment, no pointer, no handle): the ladder between the entry points above
// (choose_k1, choose_b8) and the instance choosers below (swiftly_rowinst.h), stated once and tested without a GPU
// (tests/native/row_route_dump.cpp, tests/test_row_routes_cpu.py, tests/golden/row_routes.txt).
//
// The launch sites gather a RowCall, ask choose_row_route once and switch on the answer; a Refused route names its reason
// and swiftly_abi.hip turns that into the status and the text at one place.  The launchers keep their own refusals (an
// instance choose_band_instance / choose_lean_form does not have): a route says which family is asked, not that it takes it.
#pragma once

#include <cstdint>

#include "swiftly_caps.h"  // kMinLogN, kMaxLogNFloat, kBandMinLog, kBackwardBandMinLogYN

namespace swf {

// -- lengths of the kernel families the route chooses among -------------------------------------------------------
constexpr int kMaxLogNDouble = 13;  // single-workgroup double kernels, Bluestein and radix-Q double tables
// power-of-two complex128 transforms of the primitives (run_rows): 2^14 / 2^15 as four-steps -- along a strided axis
// through two fft_rows_kernel passes, along the contiguous axis through swiftly_rowslong.h
constexpr int kMaxLogNDoubleRows = 15;
// Transforms of length >= 2^kTwoPassMinLog along a STRIDED axis (rows contiguous) are decomposed into
// two passes of short transforms so that every access is >= 128 B contiguous.
constexpr int kTwoPassMinLog = 9;
constexpr int kRowPassMinLog = 13;  // the lean row kernels (swiftly_rowpass.h): 8192 ...
constexpr int kRowPassMaxLog = 15;  // ... 32768 points in one workgroup; 65536: the two-workgroup band kernel only
constexpr int kLongLogN1 = 7;       // complex128 long rows (swiftly_rowslong.h): n1 = 128 points per column of pass A
constexpr int kColPassMinLog = 2;   // the column-tile passes (swiftly_colpass.h)
constexpr int kColPassMaxLog = 10;  // 1024 points: 32-column tiles
constexpr int kColF64MinLog = 5;    // float64 arithmetic (ColPassArgs::f64, and complex128 storage): 32 ...
constexpr int kColPassMaxLogF64 = 9;  // ... 512 points
constexpr bool col_f64_instance(int logn) { return logn >= kColF64MinLog && logn <= kColPassMaxLogF64; }

constexpr int max_log_rows(bool dbl) { return dbl ? kMaxLogNDoubleRows : kMaxLogNFloat + 1; }  // 2^16: lean complex64 kernels only
// whether a length has a route at all: a power of two (logn >= 0) in the range of the precision, else a length with
// radix-Q tables in use or with Bluestein tables (both exist only where their kernels do)
constexpr bool row_length_supported(bool dbl, int logn, bool mixed, bool blu) {
    return logn >= 0 ? logn >= kMinLogN && logn <= max_log_rows(dbl) : mixed || blu;
}

// -- the generic kernel (fft_rows_kernel, launch_one of fft_rows_impl.h) --------------------------------------------
// Lengths with a real-load instance: complex64 prepare_facet of the plain band layout (why_not_real_facets), 64 .. 4096
// points (8192: the lean row kernel); complex128 (why_not_real_facets_f64): float64 rows, 64 .. 8192 points in one
// workgroup (16384 / 32768: pass A of swiftly_rowslong.h).
constexpr bool generic_has_real_load(bool dbl, int logn) {
    return logn >= kBandMinLog && (dbl ? logn <= kMaxLogNDouble : logn < kRowPassMinLog);
}
// ... and a real-store instance (the mapped store only): complex64 finish_facet of the plain band layout
// (why_not_real_facets_out), 64 .. 4096 points (8192 and longer: the lean row kernels); complex128
// (why_not_real_facets_out_f64): 64 .. 8192 points, and pass B of the long rows (128 / 256 points behind n1 = 128).
constexpr bool generic_has_real_store(bool dbl, int logn) {
    return logn >= kBackwardBandMinLogYN && (dbl ? logn <= kMaxLogNDouble : logn < kRowPassMinLog);
}

// -- the column-tile passes (col_transform, swiftly_abi_coltransform.hip) -------------------------------------------
// What a caller asks of them beyond the length: the gather-sum load, complex128 storage, float64 arithmetic and the
// stages that get it (swiftly_hip::col_f64_stages: 1 = pass A of a four-step, 2 = pass B, 4 = single pass).
struct ColAsk {
    bool gs = false, c128 = false, f64 = false;
    int f64_stages = 0;
};
enum ColSplitStatus { kColSplitOk = 0, kColOutOfRange, kColNoC128Instance, kColScratchTooLarge };
struct ColSplit {
    int status = kColSplitOk;
    bool two = false;    // four-step through a scratch of 2^logn * W elements
    int l1 = 0, l2 = 0;  // single pass: l1 = logn, l2 = 0
    bool f64 = false;
    int f64_one = 0, f64_a = 0, f64_b = 0;  // float64 arithmetic in the single pass / pass A / pass B
};
// Single pass or four-step, the halves, whether the length is in range and which passes compute in float64, for `W`
// adjacent columns.  Single pass up to 1024 points; the gather-sum load (backward pass) has complex64 instances for
// 64-column tiles only, i.e. up to 512 points: longer gather-sum transforms go through the four-step, whose pass A carries
// the load.  complex128 storage: float64 arithmetic in every pass, single pass up to 512 points -- with the gather-sum
// load too (32-column tiles at 128, 256 and 512 points), and pass A of its four-steps at 32 .. 128 points.
inline ColSplit col_split(int logn, const ColAsk& k, int64_t W) {
    ColSplit p;
    p.two = logn > (k.gs ? 9 : k.c128 ? kColPassMaxLogF64 : kColPassMaxLog);
    p.l1 = p.two ? logn / 2 : logn;  // (32768 = 128 x 256; 256 x 128 and 64 x 512 measured slower, r4)
    p.l2 = logn - p.l1;
    if (p.l1 < kColPassMinLog || p.l1 > kColPassMaxLog || (p.two && (p.l2 < kColPassMinLog || p.l2 > kColPassMaxLog)))
        p.status = kColOutOfRange;
    // float64 arithmetic where the caller asks for it and the instances exist (else float32, silently: same results to
    // float32 rounding)
    p.f64 = (k.f64 || k.c128) && (p.two ? (col_f64_instance(p.l1) && col_f64_instance(p.l2))
                                        : (col_f64_instance(logn) && !(k.gs && !k.c128 && logn > 8)));
    if (!p.status && k.c128 && !p.f64) p.status = kColNoC128Instance;
    const auto stage = [&](int bit) { return (p.f64 && (k.c128 || (k.f64_stages & bit))) ? 1 : 0; };
    p.f64_one = stage(4), p.f64_a = stage(1), p.f64_b = stage(2);
    if (!p.status && p.two && logn < 63 && (uint64_t(1) << logn) * (uint64_t)W >= (uint64_t(1) << 32)) p.status = kColScratchTooLarge;
    return p;
}

// -- the route ------------------------------------------------------------------------------------------------------
// The facts the choice reads (run_rows_chunk fills them from RowsArgs, OffTab and the handle's tables).
struct RowCall {
    bool dbl = false;  // complex128 (float64 rows where real_in / real_out)
    int64_t n = 0;     // transform length
    int logn = -1;     // its log2, or -1
    // sub-transform behind the radix-Q pass (qmul > 1), all Q of them in this launch (qadd < 0; no route depends on it)
    bool sub = false, all_j = false;
    bool rowfast = false, in_rs1 = false, out_rs1 = false;  // lanes along rows; in_rs == 1, out_rs == 1
    int64_t nrows = 0, in_cs = 0, out_cs = 0;
    int tab_use = 0, nbatch = 1;  // OffTab::use; items of this launch
    bool rm = false;              // rm_mod > 0
    bool in_rowmap = false, st_rowmap = false, row_win = false;
    bool ld_win = false, ld_win2 = false, st_win = false, st_win2 = false, st_win_bs = false;  // given / st_win_bs != 0
    int ld_a = 0, ld_len = 0, ld_c = 0, ld_mod = 0, st_a = 0, st_len = 0, st_c = 0, st_mod = 0;
    bool accumulate = false, real_in = false, real_out = false, raw_ld = false, raw_st = false;
    // twiddle tables of the precision that exist: 2^logn, and in complex64 2^(logn-1), 2^(logn-2) and the halves
    // 2^(logn/2), 2^(logn - logn/2) of a split
    bool tw = false, tw_m1 = false, tw_m2 = false, tw_h1 = false, tw_h2 = false;
    bool mixed = false;  // radix-Q tables exist and are to be used (use_mixed: SWIFTLY_NO_MIXED is the caller's to read)
    bool blu = false;    // Bluestein tables exist
    ColAsk col;          // what the call asks of the column passes (the primitives: nothing)
};

enum RowRouteKind {
    kRouteColPass = 0,    // col_transform: complex64 along the strided axis of contiguous rows
    kRouteLean,           // launch_row_pass<mode>: 8192 .. 32768 points in one workgroup
    kRouteBand32kPlain,   // launch_row_pass_band, plain store
    kRouteSplit32k,       // launch_row_pass_split
    kRouteBand32kMapped,  // launch_row_pass_band, mapped store (finish_* along the contiguous axis)
    kRouteBand64k,        // launch_row_pass_band_n(16): prepare_* loads / finish_* stores
    kRouteLongRowsF64,    // run_rows_long: 16384 / 32768 complex128 points along the contiguous axis
    kRouteGeneric,        // one launch of fft_rows_kernel
    kRouteFourStep,       // two launches of fft_rows_kernel through a scratch
    kRouteMixed,          // radix-Q pass, then power-of-two sub-transforms (which ask again)
    kRouteBluestein,      // two power-of-two transforms (which ask again) around the chirp products
    kRouteEmpty,          // no rows or no items: nothing to launch, status 0
    kRouteRefused,
};
enum RowRefusal {
    kRowTaken = 0,
    kRowLength,              // power of two outside the range of the precision
    kRowStride,              // transform length * column stride >= 2^32
    kRowNoConvolution,       // not a power of two, neither radix-Q nor Bluestein tables
    kRowNoTable,             // the handle holds no twiddle table of the length
    kRowRealInDecomposed,    // real input reaches a decomposed transform
    kRowRealOutNoStore,      // real output reaches a transform without a real store
    kRow64kLeanOnly,         // 65536 complex64 points outside the two-workgroup kernel / the column passes
    kRowLongMappedLoadOnly,  // complex128 long rows: raw / sub-transform input
    kRowNoGenericInstance,   // the generic kernel has no real-load / real-store instance of the length
};

struct RowRoute {
    int kind = kRouteRefused;
    int mode = 0;  // lean kernels: 0 identity store, 1 identity load, 2 both mapped
    bool single_store_window = false;  // mapped store of the band kernels: st_win * st_win2 folded into one window
    int refusal = kRowTaken;
};

inline RowRoute choose_row_route(const RowCall& c) {
    RowRoute r;
    const auto take = [&r](int kind) { r.kind = kind; return r; };
    const auto refuse = [&r](int why) { r.kind = kRouteRefused, r.refusal = why; return r; };
    const uint64_t lim = uint64_t(1) << 32, n = (uint64_t)c.n;

    // -- the call as a whole ------------------------------------------------------------------------------------------
    if (c.logn >= 0 && !row_length_supported(c.dbl, c.logn, false, false)) return refuse(kRowLength);
    if (n * (uint64_t)c.in_cs >= lim || n * (uint64_t)c.out_cs >= lim) return refuse(kRowStride);
    if (c.nrows <= 0 || c.nbatch <= 0) return take(kRouteEmpty);
    // -- real rows: a power of two along the contiguous axis in one launch, or nothing (the two passes of the complex128
    //    long rows count as one: A takes real_in, B real_out).  No entry point sends real rows along a strided axis or at
    //    another length; the ladder this function replaced would have read them as complex in the column passes, the
    //    radix-Q pass and the Bluestein kernels.
    const int logn = c.logn;
    if (logn < 0 && (c.real_in || c.real_out)) return refuse(c.real_in ? kRowRealInDecomposed : kRowRealOutNoStore);
    if (logn < 0) return c.mixed ? take(kRouteMixed) : c.blu ? take(kRouteBluestein) : refuse(kRowNoConvolution);
    if (!c.tw) return refuse(kRowNoTable);
    if (c.real_in && (c.sub || c.rowfast || c.raw_ld)) return refuse(kRowRealInDecomposed);
    if (c.real_out && (c.sub || c.rowfast)) return refuse(kRowRealOutNoStore);

    if (!c.dbl && !c.sub) {
        // -- column passes: the strided axis of row-major arrays, every element offset inside one item 32 bit ----------
        if (c.rowfast && c.in_rs1 && c.out_rs1 && !(c.tab_use & 8) && !c.rm && !c.in_rowmap) {
            const uint64_t W = (uint64_t)c.nrows;
            const ColSplit s = col_split(logn, c.col, c.nrows);
            const bool tables = !s.two || (c.tw_h1 && c.tw_h2);  // (s.l1 = logn / 2: the halves of a split)
            if (n * (uint64_t)c.in_cs + W < lim && n * (uint64_t)c.out_cs + W < lim && n * W < lim && !s.status && tables)
                return take(kRouteColPass);
        }
        // -- lean row kernels: the contiguous axis, one item, 8192 points and more ------------------------------------
        const bool lean_call = !c.rowfast && c.in_cs == 1 && c.out_cs == 1 && c.tab_use == 0 && c.nbatch <= 1 &&
                               logn >= kRowPassMinLog && logn <= kRowPassMaxLog + 1 && !c.ld_win2 && !c.st_win_bs &&
                               !c.st_rowmap &&
                               !(c.row_win && logn > kRowPassMaxLog);  // (the two-workgroup kernels take it through prepare_facet_band only)
        if (lean_call) {
            const int len = 1 << logn;
            const bool ident_ld = c.ld_a == 0 && c.ld_len == len && c.ld_c == 0 && !c.ld_win;
            const bool ident_st = c.st_a == 0 && c.st_len == len && c.st_c == 0 && !c.st_win && !c.st_win2;
            r.mode = ident_st ? 0 : (ident_ld ? 1 : 2);
            const bool prep_ld = c.ld_c == 0 && c.ld_mod == c.ld_len;  // load map of a prepare_* primitive (or identity)
            const bool fin_st = c.st_c == 0 && c.st_mod == c.st_len;   // store map of a finish_* primitive
            const bool plain = r.mode == 0 && !c.accumulate;
            const bool mapped = r.mode != 0 && fin_st && prep_ld && !c.ld_win;  // finish_* along the contiguous axis
            if (c.real_in) {  // real input: 8192-point rows of the plain band layout only (longer ones: prepare_facet_k1)
                if (logn == kRowPassMinLog && r.mode == 0) return take(kRouteLean);
            } else if (logn == 15 && plain && c.tw_m1 && prep_ld) {
                return take(kRouteBand32kPlain);
            } else if (logn == 15 && plain && c.tw_m1 && c.tw_m2) {
                return take(kRouteSplit32k);
            } else if (logn == 15 && mapped && c.tw_m1) {
                r.single_store_window = true;
                return take(kRouteBand32kMapped);
            } else if (logn == 16) {  // 65536-point rows: only the two-workgroup kernel exists
                if (c.tw_m1 && ((plain && prep_ld) || mapped)) {
                    r.single_store_window = mapped;
                    return take(kRouteBand64k);
                }
            } else {
                return take(kRouteLean);
            }
            r.mode = 0;
        }
    }
    // -- what is left: the generic kernel, the complex128 long rows and the four-step -----------------------------------
    // real output: every lean row kernel that takes it has been chosen above
    if (c.real_out && (c.raw_st || c.st_rowmap || c.accumulate || (!c.dbl && logn >= kRowPassMinLog))) return refuse(kRowRealOutNoStore);
    if (!c.dbl && logn > kMaxLogNFloat) return refuse(kRow64kLeanOnly);
    if (c.dbl && !c.rowfast && logn > kMaxLogNDouble)  // (hands real_in to its pass A and real_out to its pass B)
        return c.sub || c.raw_ld ? refuse(kRowLongMappedLoadOnly) : take(kRouteLongRowsF64);
    if (c.rowfast && logn >= kTwoPassMinLog) return take(kRouteFourStep);
    if (c.real_in ? !generic_has_real_load(c.dbl, logn) : c.real_out && !generic_has_real_store(c.dbl, logn))
        return refuse(kRowNoGenericInstance);
    return take(kRouteGeneric);
}

}  // namespace swf
