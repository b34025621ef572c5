// test_head_skip THR_BITS... -- prints csrc/head_skip.h's early-out bound for every threshold given as the hex bit pattern of an fp32 value,
// one line each: "<threshold bits> <bound bits> <bound>".  Bit patterns, so that tests/test_head_skip.py hands over and reads back exact values.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "head_skip.h"

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s THR_BITS_HEX...\n", argv[0]); return 2; }
    for (int i = 1; i < argc; ++i) {
        char* end = nullptr;
        const uint32_t tb = (uint32_t)std::strtoul(argv[i], &end, 16);
        if (end == argv[i] || *end) { std::fprintf(stderr, "%s: not a hex bit pattern\n", argv[i]); return 2; }
        float thr, bound;
        std::memcpy(&thr, &tb, 4);
        bound = zly::head_skip_logit(thr);
        uint32_t bb;
        std::memcpy(&bb, &bound, 4);
        std::printf("%08x %08x %.9g\n", (unsigned)tb, (unsigned)bb, (double)bound);
    }
    return 0;
}
