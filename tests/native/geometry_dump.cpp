// Prints what the functions of csrc/swiftly_geometry.h return, for tests/test_geometry_cpu.py: one request per line of
// stdin, one line of integers per answer.  Plain C++17, no HIP: only the two headers of pure host functions.
//
//   maps    N yN xM yB xA off                         -> lo | facet map | contribution map, sp, placement start | subgrid map
//   window  N yN xM off                               -> s rot base, then the source column of every position q < m
//   bandmap N yN xM band_start band_len               -> valid | band load map
//   inband  N yN xM off first count band_start band_len -> first position outside the band, or -1
//   fits    count stride extra                        -> 1 when count * stride + extra < 2^32
#include <cstdio>
#include <iostream>
#include <string>

#include "swiftly_caps.h"
#include "swiftly_geometry.h"

using namespace swf;

static void put(const Map& g) { std::printf(" %d %d %d %d", g.a, g.len, g.c, g.mod); }

int main() {
    std::string what;
    while (std::cin >> what) {
        if (what == "fits") {
            long long count, stride, extra;
            std::cin >> count >> stride >> extra;
            std::printf("%d\n", offsets_fit_32(count, stride, extra) ? 1 : 0);
            continue;
        }
        long long N, yN, xM;
        std::cin >> N >> yN >> xM;
        if (!check_sizes(N, yN, xM).empty()) {
            std::fprintf(stderr, "%s\n", check_sizes(N, yN, xM).c_str());
            return 2;
        }
        const Sizes z = make_sizes(N, yN, xM);
        if (what == "maps") {
            long long yB, xA, off;
            std::cin >> yB >> xA >> off;
            std::printf("%d", facet_lo(z, yB));
            put(facet_in_padded_facet(z, yB, off));
            put(contribution_in_padded_subgrid(z, off));
            std::printf(" %lld %d", (long long)facet_shift(z, off), placement_start(z, facet_shift(z, off)));
            put(subgrid_in_padded_subgrid(z, xA, off));
            std::printf("\n");
        } else if (what == "window") {
            long long off;
            std::cin >> off;
            const Window w = window_of(z, off);
            std::printf("%lld %d %d\n", (long long)w.s, w.rot, w.base);
            for (long long q = 0; q < z.m; q++) std::printf(q ? " %d" : "%d", window_column(z, w, q));
            std::printf("\n");
        } else if (what == "bandmap") {
            long long start, len;
            std::cin >> start >> len;
            std::printf("%d", band_valid(z.yN, start, len) ? 1 : 0);
            put(band_as_load_map(z, start, len));
            std::printf("\n");
        } else if (what == "inband") {
            long long off, first, count, start, len;
            std::cin >> off >> first >> count >> start >> len;
            std::printf("%lld\n", (long long)window_in_band(z, window_of(z, off), first, count, start, len));
        } else {
            std::fprintf(stderr, "unknown request %s\n", what.c_str());
            return 2;
        }
    }
    return 0;
}
