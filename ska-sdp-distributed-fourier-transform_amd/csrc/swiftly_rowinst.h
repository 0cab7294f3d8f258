// Which instance of the long-row kernels a call runs, as pure host functions of integers (no HIP, no environment, no
// pointer): the policy of launch_row_pass_band_n and the real-load / real-store gates of launch_row_pass (row_pass.hip),
// stated once and tested without a GPU (tests/native/band_instance_dump.cpp, tests/test_band_instances_cpu.py).
//
// Two rules the policy keeps by construction:
//  * Geometries round differently, so the geometry, the pair loads, the segment count and the rotation of a call never
//    depend on the TYPE of its rows (RowPassArgs::in_real / out_real) nor on where real rows lie (pitch, base): a real
//    call gets the choice of the complex call for the promoted row, with `real` / `real_st` set at the end.
//  * A real call differs from that complex call in the window path only: the complex K1 takes the window table at
//    SWIFTLY_K1_WIN4 = 1 (RGeoPre with W4) where the real K1 has no such instance and keeps the plain window loads; and
//    4-byte real loads (real = 2) never take W4.  Both paths multiply by the same window values.
//  * The window-rows store of real rows (BandCall::whole_real, a fact about the whole-row family like stage_columns) is the
//    complex window-rows call for the promoted row with real = 1, or a refusal (-2): it has 8-byte loads only.
#pragma once

namespace swf {

// the facts the choice reads (launch_row_pass_band_n fills it from RowPassArgs, the two environment knobs and the cache)
struct BandCall {
    int logn = 0;  // log2 of the full row length
    int ld_a = 0, ld_len = 0, ld_c = 0, ld_mod = 0;
    bool ld_win = false;                // a load window is given
    int band_sign = 0, band_half = 0;   // sign of band_len: + band store, 0 plain store, - mapped store
    bool conj_ld = false, conj_st = false, accumulate = false;
    bool in_real = false, out_real = false;
    bool pitch_odd = false;             // in_pitch & 1
    int base_align = 0;                 // address of the input & 15
    // window-rows store (RowPassArgs::win_full): what is tested of the group
    bool win_full = false;
    int win_logm = 0, nwin = 0;
    bool win_d = false, win_fn = false, win_tw_m = false, win_twc_m = false;
    int win4_level = 0;                 // SWIFTLY_K1_WIN4: 0 plain window loads, 1 window table, 2 + compact twiddles
    bool whole_enabled = false;         // SWIFTLY_K1_WHOLE
    bool has_cache = false;             // the caller owns a table cache ...
    bool has_twc = false;               // ... with compact twiddle sections
    bool table_available = false;       // Win4Cache::get would return a table
    int stage_columns = 0, max_windows = 0;  // row_pass_whole_stage_columns(), kWholeMaxWindows
    bool whole_real = false;            // the whole-row family has real window-rows instances (row_whole.hip)
};

enum BandStatus { kBandChosen = 0, kBandNone = -1, kBandNotWindowRows = -2 };
enum BandFamily { kBandTwoWorkgroup = 0, kBandWholeRow = 1 };
// geometries of the two-workgroup kernel (the aliases of row_pass.hip), and RGeoWhole of the whole-row kernel
enum BandGeoId { kBandGeo16k = 0, kBandGeo4, kBandGeo5, kBandGeo5Pre, kBandGeo5PreC, kBandGeo5C, kBandGeo64k, kBandGeoWhole };
constexpr int kBandStWindowRows = 3;  // `st` of the whole-row family's window-rows instances (its band store: 1)

struct BandInst {
    int status = kBandChosen;
    int family = kBandTwoWorkgroup, geo = kBandGeo16k;
    // template arguments of row_pass_band_kernel; of the whole-row family: nseg and st
    bool win = false;
    int st = 0;
    bool pair = false;
    int nseg = 0, cj = -1;
    bool w4 = false;
    int real = 0;
    bool real_st = false;
    // what the launcher puts into the arguments
    int seg_rot = 0;
    bool ld_win4 = false, twc = false;
    // the window table the launcher requests before it launches (key_ns = 0: none), also in front of a -2
    int key_c = 0, key_ns = 0, key_n = 0, key_seglen = 0;

    bool same_instance(const BandInst& o) const {
        return family == o.family && geo == o.geo && win == o.win && st == o.st && pair == o.pair && nseg == o.nseg &&
               cj == o.cj && w4 == o.w4 && real == o.real && real_st == o.real_st;
    }
    bool operator==(const BandInst& o) const {
        return status == o.status && same_instance(o) && seg_rot == o.seg_rot && ld_win4 == o.ld_win4 && twc == o.twc &&
               key_c == o.key_c && key_ns == o.key_ns && key_n == o.key_n && key_seglen == o.key_seglen;
    }
};

constexpr int kBandSegLen = 1024;  // points of a segment: a lane pair's 2 x 512 (32768-point rows), a lane's 1024 (65536)

// Cyclic run of input segments (seglen consecutive points of the n-point transform input) that can hold data under
// the load map of a prepare_* primitive: q = (j + n/2 + ld_a) mod n < ld_len.  Returns the length of the run and its
// first segment (0, all segments: the row has no empty segment).
inline int data_segment_run(int ld_a, int ld_len, int n, int seglen, int* first) {
    const int nseg = n / seglen, base = (int)(((long long)ld_a + n / 2) % n);
    int valid[64];
    int count = 0;
    for (int r = 0; r < nseg; r++) {
        const int lo = (int)(((long long)seglen * r + base) % n);
        valid[r] = ld_len > 0 && (lo < ld_len || lo + seglen > n);
        count += valid[r];
    }
    *first = 0;
    if (count == nseg || count == 0) return count == 0 ? 1 : nseg;
    for (int r = 0; r < nseg; r++)
        if (valid[r] && !valid[(r + nseg - 1) % nseg]) *first = r;
    int run = 0;
    while (run < nseg && valid[(*first + run) % nseg]) run++;
    return run == count ? run : nseg;  // two runs cannot happen for one cyclic range; be safe
}

inline BandInst choose_band_instance(const BandCall& c) {
    BandInst r;
    const auto refuse = [&r](int status) {  // (keeps the table request that came before the refusal)
        BandInst x;
        x.status = status;
        x.key_c = r.key_c, x.key_ns = r.key_ns, x.key_n = r.key_n, x.key_seglen = r.key_seglen;
        return x;
    };
    const bool band = c.band_sign > 0, mapped = c.band_sign < 0;
    // prepare_facet is an inverse transform (both conjugations), finish_facet a forward one (neither): the segment
    // instances have them compiled in (CJ)
    const bool inv = c.conj_ld && c.conj_st, fwd = !c.conj_ld && !c.conj_st;
    const bool out_real = c.out_real && !c.in_real;
    // adjacent-point loads need an even shift and length; 16 bytes of a complex row also an even pitch and a 16-byte
    // base.  Adjacent reals are a pair wherever the rows lie: one 8-byte load, or two 4-byte loads (real = 2).
    const bool pair_ok = !(c.ld_a & 1) && !(c.ld_len & 1) && (c.in_real || (!c.pitch_odd && (c.base_align & 15) == 0));
    const bool load8 = !c.pitch_odd && (c.base_align & 7) == 0;

    // -- what exists at all ----------------------------------------------------------------------------------------
    // real input: the forward K1 of the band pipeline (window, band store, the facet at the start of its rows)
    const bool real_windows = c.in_real && c.win_full && c.whole_real;  // (without whole_real: no such instance, as ever)
    if (c.in_real && !real_windows && (!c.ld_win || !band || c.win_full || c.ld_c != 0 || c.ld_mod != c.ld_len))
        return refuse(kBandNone);
    if (out_real && (!mapped || c.win_full)) return refuse(kBandNone);  // real output: the mapped store only
    if (c.win_full) {
        // window-rows store (whole-row kernel): 32768-point rows, 512-column windows, 16-byte loads
        if (c.logn != 15 || c.win_logm != 9 || c.nwin <= 0 || !c.win_d || !band) return refuse(kBandNotWindowRows);
        if (!pair_ok || !c.ld_win || !inv) return refuse(kBandNotWindowRows);
        // real rows: two adjacent reals are one 8-byte load (there is no real = 2 form), the facet at the start of its rows
        if (real_windows && (!load8 || c.ld_c != 0 || c.ld_mod != c.ld_len)) return refuse(kBandNotWindowRows);
    }

    // -- geometry --------------------------------------------------------------------------------------------------
    if (c.logn == 16) {
        r.geo = kBandGeo64k;
    } else if (c.logn == 14) {
        r.geo = kBandGeo16k;
    } else if (c.logn == 15) {
        // 512 threads x 32 points (two workgroups per CU) for the band store and the mapped store; 1024 x 16 (one per CU)
        // for the plain store, where the 512-thread form spills ~49 VGPRs
        r.geo = c.band_sign == 0 ? kBandGeo4 : kBandGeo5;
        r.pair = c.band_sign != 0 && pair_ok;
    } else {
        return refuse(kBandNone);
    }
    r.real = !c.in_real ? 0 : (r.pair && !load8) ? 2 : 1;

    // -- empty segments compiled out (pair geometry of the 32768-point rows, 65536-point geometry) -------------------
    int first = 0, run = 0;
    if (r.pair || r.geo == kBandGeo64k) run = data_segment_run(c.ld_a, c.ld_len, 1 << c.logn, kBandSegLen, &first);
    if (r.pair && band && c.ld_win && inv) {
        // forward K1: twiddle preload (RGeoPre); with a window table 16-byte window loads (W4), and with the compact
        // twiddle sections RGeoPreC or the whole-row kernel
        const int ns = run <= 16 ? 16 : run <= 22 ? 22 : run <= 24 ? 24 : 0;
        if (ns) {
            r.win = true, r.st = 1, r.nseg = ns, r.cj = 1, r.seg_rot = first;
            const bool wanted = c.has_cache && (c.in_real ? load8 && c.win4_level >= 2 && c.has_twc : c.win4_level != 0);
            if (wanted && c.table_available) {
                r.ld_win4 = true;
                r.twc = c.win4_level >= 2 && c.has_twc;
                r.key_n = 1 << c.logn, r.key_ns = ns, r.key_seglen = kBandSegLen;
                r.key_c = (int)(((long long)c.ld_a + r.key_n / 2 + (long long)first * kBandSegLen) % r.key_n);
            }
            if (r.twc && (c.in_real ? real_windows : c.win_full || c.whole_enabled)) {
                if (c.win_full && (c.nwin > c.max_windows || !c.win_fn || !c.win_tw_m || !c.win_twc_m ||
                                   2 * c.band_half > c.stage_columns))
                    return refuse(kBandNotWindowRows);
                r.family = kBandWholeRow, r.geo = kBandGeoWhole, r.pair = false, r.cj = -1;
                if (c.win_full) r.st = kBandStWindowRows;
                return r;
            }
            if (c.win_full) return refuse(kBandNotWindowRows);  // window-rows store: only the whole-row instances
            r.geo = r.twc ? kBandGeo5PreC : kBandGeo5Pre;
            r.w4 = r.ld_win4;
            return r;
        }
        if (c.win_full) return refuse(kBandNotWindowRows);
    } else if (r.pair && mapped && fwd) {
        // backward finish: compact twiddle sections (RGeoC) when the caller owns the tables; no preload (128 VGPRs)
        r.twc = c.has_cache && c.win4_level >= 2 && c.has_twc;
        const int ns = run <= 13 ? 13 : run <= 16 ? 16 : 0;
        if (ns) {
            r.nseg = ns, r.cj = 0, r.seg_rot = first;
            if (r.twc) r.geo = kBandGeo5C;
        }
    } else if (r.geo == kBandGeo64k && band && c.ld_win && inv && run <= 44) {
        r.nseg = 44, r.cj = 1, r.seg_rot = first;
    }

    // -- store form ------------------------------------------------------------------------------------------------
    if (mapped) {  // crop + window store of the finish_* primitives; it has no load window
        r.st = 2;
        if (out_real) {
            // real twins exist where a finish can arrive: the 32-points-per-lane geometries
            if (r.geo == kBandGeo16k || r.geo == kBandGeo4 || c.accumulate) return refuse(kBandNone);
            r.real_st = true;
        }
        return r;
    }
    r.win = c.ld_win;
    r.st = band ? 1 : 0;
    return r;
}

// -- the lean single-workgroup kernel (row_pass_kernel, launch_row_pass) -------------------------------------------
// Which form of the instance <logn, mode> a call runs: real load for 8192 points and MODE 0 only, real store for 8192 /
// 16384 points and MODE 1 / 2 without accumulate (longer real rows: the band row kernel above).  A mode other than 0 / 1
// is MODE 2, as launch_row_pass takes it.
enum LeanForm { kLeanNone = -1, kLeanComplex = 0, kLeanRealLoad = 1, kLeanRealStore = 2 };
inline LeanForm choose_lean_form(int logn, int mode, bool in_real, bool out_real, bool accumulate) {
    if (in_real) return logn == 13 && mode == 0 ? kLeanRealLoad : kLeanNone;
    if (out_real) return (logn == 13 || logn == 14) && (mode == 1 || mode == 2) && !accumulate ? kLeanRealStore : kLeanNone;
    return logn >= 13 && logn <= 15 ? kLeanComplex : kLeanNone;
}

}  // namespace swf
