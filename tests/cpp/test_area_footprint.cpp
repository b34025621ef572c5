// test_area_footprint.cpp -- the area resize filter's per-axis footprint arithmetic exactly as the pre-pass kernel computes it (csrc/area_device.h,
// compiled here by the host compiler), printed for tests/test_area_footprint.py.  TEST INFRASTRUCTURE: no GPU.
//
//   test_area_footprint S D d [S D d ...]   ->   one line "S D d i0 i1 w(i0) w(i1) sum" per triple; sum = the weights of d added up over i0 .. i1
#include <cstdio>
#include <cstdlib>

#include "area_device.h"

int main(int argc, char** argv)
{
    if (argc < 4 || (argc - 1) % 3) return 2;
    for (int k = 1; k + 2 < argc; k += 3) {
        const int S = std::atoi(argv[k]), D = std::atoi(argv[k + 1]), d = std::atoi(argv[k + 2]);
        if (S < 1 || D < 1 || d < 0 || d >= D) return 3;
        const zly::AreaSpan a = zly::area_span(S, D, d);
        long long sum = 0;
        for (int i = a.i0; i <= a.i1; ++i) sum += zly::area_weight(a, D, i);
        std::printf("%d %d %d %d %d %d %d %lld\n", S, D, d, a.i0, a.i1, zly::area_weight(a, D, a.i0), zly::area_weight(a, D, a.i1), sum);
    }
    return 0;
}
