// Prints what the functions of csrc/swiftly_rowinst.h return, for tests/test_band_instances_cpu.py: one request per line of
// stdin, one line of integers per answer.  Plain C++17, no HIP: only that header.
//
//   band <the 29 BandCall fields, in the order read below>  -> the 18 BandInst fields, in the order printed below
//   run  ld_a ld_len n seglen                               -> run first        (data_segment_run)
//   lean logn mode in_real out_real accumulate              -> LeanForm         (choose_lean_form)
#include <cstdio>
#include <iostream>
#include <string>

#include "swiftly_rowinst.h"

using namespace swf;

int main() {
    std::string what;
    while (std::cin >> what) {
        if (what == "band") {
            BandCall c;
            std::cin >> c.logn >> c.ld_a >> c.ld_len >> c.ld_c >> c.ld_mod >> c.ld_win >> c.band_sign >> c.band_half >> c.conj_ld >>
                c.conj_st >> c.accumulate >> c.in_real >> c.out_real >> c.pitch_odd >> c.base_align >> c.win_full >> c.win_logm >>
                c.nwin >> c.win_d >> c.win_fn >> c.win_tw_m >> c.win_twc_m >> c.win4_level >> c.whole_enabled >> c.has_cache >>
                c.has_twc >> c.table_available >> c.stage_columns >> c.max_windows;
            const BandInst r = choose_band_instance(c);
            std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", r.status, r.family, r.geo, r.win, r.st, r.pair, r.nseg,
                        r.cj, r.w4, r.real, r.real_st, r.seg_rot, r.ld_win4, r.twc, r.key_c, r.key_ns, r.key_n, r.key_seglen);
        } else if (what == "run") {
            int ld_a, ld_len, n, seglen, first = 0;
            std::cin >> ld_a >> ld_len >> n >> seglen;
            const int run = data_segment_run(ld_a, ld_len, n, seglen, &first);
            std::printf("%d %d\n", run, first);
        } else if (what == "lean") {
            int logn, mode;
            bool in_real, out_real, accumulate;
            std::cin >> logn >> mode >> in_real >> out_real >> accumulate;
            std::printf("%d\n", (int)choose_lean_form(logn, mode, in_real, out_real, accumulate));
        } else {
            std::fprintf(stderr, "unknown request %s\n", what.c_str());
            return 2;
        }
        if (!std::cin) {
            std::fprintf(stderr, "malformed %s request\n", what.c_str());
            return 2;
        }
    }
    return 0;
}
