// The rule of gx_top_lines (gorp_amd/csrc/gx_top.hpp, plain C++) as a program of its own: cases on stdin, one per line, the answers on
// stdout in the same order; tests/test_top_host.py compares them with Python's sorted().  Built with -fsanitize=address,undefined
// -fno-sanitize-recover=undefined: the histograms are allocated with exactly their 256 bins, so a probe outside them is a report, and a
// negation of INT64_MIN would end the program.
//   K <smallest 0|1> <v>                top_key, and back; prints the key and top_value(key)
//   D <key> <d>                         top_digit; prints the digit
//   P <remaining> <pairs> (<bin> <count>)...
//                                       top_pick on a histogram that is zero but for the pairs; prints bin above remaining
//   S <smallest 0|1> <n_wanted> <count> <v>...
//                                       the full select on the host: top_begin, eight rounds of top_step over histograms built here
//                                       with top_in_prefix / top_digit, then top_chosen with every value's rank among its equals;
//                                       prints n_top, threshold value, above, ties taken, then the chosen values' places in the input
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "gx_top.hpp"

static void select(std::istringstream& in) {
    int smallest = 0;
    uint32_t n_wanted = 0;
    size_t count = 0;
    in >> smallest >> n_wanted >> count;
    std::vector<uint64_t> keys(count);
    for (size_t i = 0; i < count; ++i) {
        int64_t v = 0;
        in >> v;
        keys[i] = gx::top_key(v, smallest != 0);
    }
    gx::TopSelect s;
    gx::top_begin(s, n_wanted, count);
    for (uint32_t d = gx::TOP_DIGITS; d-- > 0u;) {
        std::unique_ptr<uint32_t[]> hist(new uint32_t[gx::TOP_BINS]());   // exactly 256 bins
        for (uint64_t k : keys)
            if (gx::top_in_prefix(k, s.prefix, d)) ++hist[gx::top_digit(k, d)];
        gx::top_step(s, hist.get(), d);
    }
    printf("%u %" PRId64 " %u %u", s.n_top, s.n_top ? gx::top_value(s.prefix, smallest != 0) : 0, s.above, s.n_top ? s.remaining : 0u);
    uint64_t equal_before = 0;
    for (size_t i = 0; i < count; ++i) {
        if (gx::top_chosen(s, keys[i], equal_before)) printf(" %zu", i);
        if (keys[i] == s.prefix) ++equal_before;
    }
    printf("\n");
}

int main() {
    std::string row;
    while (std::getline(std::cin, row)) {
        if (row.empty()) continue;
        std::istringstream in(row);
        std::string kind;
        in >> kind;
        if (kind == "K") {
            int smallest = 0;
            int64_t v = 0;
            in >> smallest >> v;
            const uint64_t k = gx::top_key(v, smallest != 0);
            printf("%" PRIu64 " %" PRId64 "\n", k, gx::top_value(k, smallest != 0));
        } else if (kind == "D") {
            uint64_t key = 0;
            uint32_t d = 0;
            in >> key >> d;
            printf("%u\n", gx::top_digit(key, d));
        } else if (kind == "P") {
            uint32_t remaining = 0, pairs = 0;
            in >> remaining >> pairs;
            std::unique_ptr<uint32_t[]> hist(new uint32_t[gx::TOP_BINS]());
            for (uint32_t p = 0; p < pairs; ++p) {
                uint32_t bin = 0, c = 0;
                in >> bin >> c;
                if (bin >= gx::TOP_BINS) return 2;
                hist[bin] = c;
            }
            const gx::TopPick p = gx::top_pick(hist.get(), remaining);
            printf("%u %u %u\n", p.bin, p.above, p.remaining);
        } else if (kind == "S") {
            select(in);
        } else {
            fprintf(stderr, "unknown case: %s\n", row.c_str());
            return 2;
        }
    }
    return 0;
}
