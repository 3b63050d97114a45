// csrc/mm_isect_device.h as plain host C++, a program of its own (tests/test_intersect_attack_host.py builds it with g++
// and -ffp-contract=off, plain and under the address and undefined-behaviour sanitizers, and runs it directly): the
// state of pairs of faces read from a file (argv[1]) or from stdin.  A record is 24 tokens separated by white space: the
// corners p1 q1 r1 p2 q2 r2 as 18 doubles (hexadecimal floating point, so that no digit is lost) and their six ids.
// One line of output a record: pair_state as an integer, the coincident bit included.
#include <cstdio>
#include <cstdlib>

#include "mm_isect_device.h"

using namespace mm::isect;

static bool token(std::FILE* f, char* buf)
{
    return std::fscanf(f, "%63s", buf) == 1;
}

int main(int argc, char** argv)
{
    std::FILE* f = argc > 1 ? std::fopen(argv[1], "r") : stdin;
    if (!f) { std::fprintf(stderr, "isect_device_host: cannot open %s\n", argv[1]); return 2; }
    char buf[64];
    long n = 0;
    for (;;) {
        double x[18];
        int id[6];
        int k = 0;
        for (; k < 24; ++k) {
            if (!token(f, buf)) break;
            char* end = nullptr;
            if (k < 18) x[k] = std::strtod(buf, &end);
            else id[k - 18] = (int)std::strtol(buf, &end, 10);
            if (end == buf || *end != '\0') { std::fprintf(stderr, "isect_device_host: record %ld: bad token '%s'\n", n, buf); return 2; }
        }
        if (k == 0) break;
        if (k != 24) { std::fprintf(stderr, "isect_device_host: record %ld is short\n", n); return 2; }
        const P3 p1{x[0], x[1], x[2]}, q1{x[3], x[4], x[5]}, r1{x[6], x[7], x[8]};
        const P3 p2{x[9], x[10], x[11]}, q2{x[12], x[13], x[14]}, r2{x[15], x[16], x[17]};
        std::printf("%d\n", pair_state(p1, q1, r1, id[0], id[1], id[2], p2, q2, r2, id[3], id[4], id[5]));
        ++n;
    }
    if (f != stdin) std::fclose(f);
    std::fprintf(stderr, "isect_device_host: %ld records\n", n);
    return 0;
}
