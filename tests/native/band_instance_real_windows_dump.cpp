// Prints what choose_band_instance (csrc/swiftly_rowinst.h) answers for a BandCall WITH the field that says the whole-row
// family has real window-rows instances, for tests/test_band_instances_real_windows_cpu.py: one request per line of stdin,
// one line of integers per answer.  Plain C++17, no HIP: only that header.  (tests/native/band_instance_dump.cpp is the
// program of the 29 fields that came before the field; it never sets it.)
//
//   band <the 29 BandCall fields of band_instance_dump.cpp, in its order> whole_real  -> the 18 BandInst fields, in its order
#include <cstdio>
#include <iostream>
#include <string>

#include "swiftly_rowinst.h"

using namespace swf;

int main() {
    std::string what;
    while (std::cin >> what) {
        if (what != "band") {
            std::fprintf(stderr, "unknown request %s\n", what.c_str());
            return 2;
        }
        BandCall c;
        std::cin >> c.logn >> c.ld_a >> c.ld_len >> c.ld_c >> c.ld_mod >> c.ld_win >> c.band_sign >> c.band_half >> c.conj_ld >>
            c.conj_st >> c.accumulate >> c.in_real >> c.out_real >> c.pitch_odd >> c.base_align >> c.win_full >> c.win_logm >>
            c.nwin >> c.win_d >> c.win_fn >> c.win_tw_m >> c.win_twc_m >> c.win4_level >> c.whole_enabled >> c.has_cache >>
            c.has_twc >> c.table_available >> c.stage_columns >> c.max_windows >> c.whole_real;
        if (!std::cin) {
            std::fprintf(stderr, "malformed band request\n");
            return 2;
        }
        const BandInst r = choose_band_instance(c);
        std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", r.status, r.family, r.geo, r.win, r.st, r.pair, r.nseg,
                    r.cj, r.w4, r.real, r.real_st, r.seg_rot, r.ld_win4, r.twc, r.key_c, r.key_ns, r.key_n, r.key_seglen);
    }
    return 0;
}
