// Prints what the functions of csrc/swiftly_rowroute.h return, for tests/test_row_routes_cpu.py: one request per line of
// stdin, one line of integers per answer.  Plain C++17, no HIP: only that header.
//
//   route <the 46 RowCall fields, in the order read below>  -> kind mode single_store_window refusal   (choose_row_route)
//   split logn gs c128 f64 f64_stages W                     -> status two l1 l2 f64 f64_one f64_a f64_b  (col_split)
//   real  dbl logn                                          -> real-load real-store                    (the generic kernel)
//   length dbl logn mixed blu                               -> 1 when the length has a route at all     (row_length_supported)
#include <cstdio>
#include <iostream>
#include <string>

#include "swiftly_rowroute.h"

using namespace swf;

int main() {
    std::string what;
    while (std::cin >> what) {
        if (what == "route") {
            RowCall c;
            std::cin >> c.dbl >> c.n >> c.logn >> c.sub >> c.all_j >> c.rowfast >> c.in_rs1 >> c.out_rs1 >> c.nrows >> c.in_cs >> c.out_cs >>
                c.tab_use >> c.nbatch >> c.rm >> c.in_rowmap >> c.st_rowmap >> c.row_win >> c.ld_win >> c.ld_win2 >> c.st_win >> c.st_win2 >>
                c.st_win_bs >> c.ld_a >> c.ld_len >> c.ld_c >> c.ld_mod >> c.st_a >> c.st_len >> c.st_c >> c.st_mod >> c.accumulate >>
                c.real_in >> c.real_out >> c.raw_ld >> c.raw_st >> c.tw >> c.tw_m1 >> c.tw_m2 >> c.tw_h1 >> c.tw_h2 >> c.mixed >> c.blu >>
                c.col.gs >> c.col.c128 >> c.col.f64 >> c.col.f64_stages;
            const RowRoute r = choose_row_route(c);
            std::printf("%d %d %d %d\n", r.kind, r.mode, r.single_store_window, r.refusal);
        } else if (what == "split") {
            int logn;
            long long W;
            ColAsk k;
            std::cin >> logn >> k.gs >> k.c128 >> k.f64 >> k.f64_stages >> W;
            const ColSplit s = col_split(logn, k, W);
            std::printf("%d %d %d %d %d %d %d %d\n", s.status, s.two, s.l1, s.l2, s.f64, s.f64_one, s.f64_a, s.f64_b);
        } else if (what == "real") {
            bool dbl;
            int logn;
            std::cin >> dbl >> logn;
            std::printf("%d %d\n", generic_has_real_load(dbl, logn), generic_has_real_store(dbl, logn));
        } else if (what == "length") {
            bool dbl, mixed, blu;
            int logn;
            std::cin >> dbl >> logn >> mixed >> blu;
            std::printf("%d\n", row_length_supported(dbl, logn, mixed, blu));
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
