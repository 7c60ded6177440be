// by_key_test.cpp -- the rule of gx_lines_by_key (gorp_amd/csrc/gx_by_key.hpp) as a program of its own, built by
// tests/test_by_key_host.py with g++ -fsanitize=address,undefined and fed rows on stdin.
//
//   K <lines> <min_lines> <max_lines>          prints: by_key_kept
//   P <n_keys> <all_digits>                    prints: by_key_passes by_key_result_buffer, then the passes' shifts
//   S <n_keys> <all_digits> <m> <key number> x m
// the kernels' sort on the host -- per pass of the plan a count per digit, its exclusive scan, a scatter in input order, ping and pong
// -- over the entries (key number, place in the list), and the bounds by by_key_begin;
// prints: the sorted entries' places, then by_key_begin(j) for j = 0 .. min(n_keys, 5000) and, beyond that, for j = n_keys.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "gx_by_key.hpp"

using namespace gx;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char kind = 0;
        in >> kind;
        if (kind == 'K') {
            uint64_t lines = 0, lo = 0, hi = 0;
            in >> lines >> lo >> hi;
            printf("%d\n", by_key_kept(lines, lo, hi) ? 1 : 0);
        } else if (kind == 'P') {
            uint64_t n_keys = 0;
            uint32_t all = 0;
            in >> n_keys >> all;
            const uint32_t passes = by_key_passes(n_keys, all != 0);
            printf("%u %u", passes, by_key_result_buffer(passes));
            for (uint32_t p = 0; p < passes; ++p) printf(" %u", by_key_shift(p));
            printf("\n");
        } else if (kind == 'S') {
            uint64_t n_keys = 0, m = 0;
            uint32_t all = 0;
            in >> n_keys >> all >> m;
            std::vector<uint32_t> knum[2], place[2];
            for (int q = 0; q < 2; ++q) { knum[q].assign(m, 0xDEADBEEFu); place[q].assign(m, 0xDEADBEEFu); }
            for (uint64_t i = 0; i < m; ++i) {
                in >> knum[0][i];
                place[0][i] = static_cast<uint32_t>(i);
            }
            const uint32_t passes = by_key_passes(n_keys, all != 0);
            uint32_t cur = 0;
            for (uint32_t p = 0; p < passes; ++p) {
                const uint32_t shift = by_key_shift(p);
                uint64_t base[GQ_BINS + 1] = {};
                for (uint64_t i = 0; i < m; ++i) ++base[gq_digit(knum[cur][i], shift) + 1u];
                for (uint32_t b = 0; b < GQ_BINS; ++b) base[b + 1u] += base[b];
                for (uint64_t i = 0; i < m; ++i) {
                    const uint64_t to = base[gq_digit(knum[cur][i], shift)]++;
                    knum[cur ^ 1u].at(to) = knum[cur][i];
                    place[cur ^ 1u].at(to) = place[cur][i];
                }
                cur ^= 1u;
            }
            if (cur != by_key_result_buffer(passes)) return 3;
            for (uint64_t i = 0; i < m; ++i) printf("%u ", place[cur][i]);
            const uint64_t shown = n_keys < 5000u ? n_keys : 5000u;   // (2^30 keys: the first bounds and the last)
            for (uint64_t j = 0; j <= shown; ++j) printf("%llu ", static_cast<unsigned long long>(by_key_begin(knum[cur].data(), m, j)));
            if (shown < n_keys) printf("%llu ", static_cast<unsigned long long>(by_key_begin(knum[cur].data(), m, n_keys)));
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
