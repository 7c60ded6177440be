// top_groups_test.cpp -- the rule of gx_top_groups (gorp_amd/csrc/gx_top_groups.hpp) as a program of its own, built by
// tests/test_top_groups_host.py with g++ -fsanitize=address,undefined and fed rows on stdin.
//
//   S <smallest> <n_wanted> <m> <hi lo> x m      rank values as (int64 hi, uint64 lo) in key-number order, every one a candidate
// prints: plan digits_run n_top last_hi last_lo ties_left roundtrip_ok, then the chosen key numbers in rank order.
//   V <rank_by> <has_values> <lines> <numbers> <min> <max> <sum_lo32s> <sum_hi32s>      tg_rank_value on a slot's words
// prints: candidate hi lo
#include <algorithm>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "gx_top_groups.hpp"

using namespace gx;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char kind = 0;
        in >> kind;
        if (kind == 'S') {
            uint32_t smallest = 0, n_wanted = 0;
            uint64_t m = 0;
            in >> smallest >> n_wanted >> m;
            std::vector<TgKey> keys(m);
            bool roundtrip = true;
            TgKey key_or{0, 0}, key_and{~0ull, ~0ull};
            for (uint64_t j = 0; j < m; ++j) {
                int64_t hi = 0;
                uint64_t lo = 0;
                in >> hi >> lo;
                keys[j] = tg_key(hi, lo, smallest != 0);
                int64_t bh = 0;
                uint64_t bl = 0;
                tg_value(keys[j], smallest != 0, &bh, &bl);
                roundtrip = roundtrip && bh == hi && bl == lo;
                key_or.hi |= keys[j].hi; key_or.lo |= keys[j].lo;
                key_and.hi &= keys[j].hi; key_and.lo &= keys[j].lo;
            }
            TgSelect s{};
            tg_begin(s, n_wanted, m, key_or, key_and);
            uint32_t run = 0;
            for (uint32_t d = TG_DIGITS; d-- > 0u;) {
                std::vector<uint32_t> hist(TOP_BINS, 0u);
                if (tg_planned(s, d)) {
                    ++run;
                    for (uint64_t j = 0; j < m; ++j)
                        if (tg_in_prefix(keys[j], s.prefix, d)) ++hist[tg_digit(keys[j], d)];
                }
                tg_step(s, hist.data(), d, key_or);
            }
            std::vector<uint32_t> chosen;
            uint64_t equal = 0;
            for (uint64_t j = 0; j < m; ++j) {
                const bool eq = s.n_top != 0u && tg_equal(keys[j], s.prefix);
                if (tg_chosen(s, keys[j], equal)) chosen.push_back(static_cast<uint32_t>(j));
                if (eq) ++equal;
            }
            std::stable_sort(chosen.begin(), chosen.end(), [&](uint32_t a, uint32_t b) { return tg_above(keys[a], keys[b]); });
            int64_t last_hi = 0;
            uint64_t last_lo = 0, ties_left = 0;
            if (s.n_top) {
                tg_value(s.prefix, smallest != 0, &last_hi, &last_lo);
                ties_left = equal - s.remaining;
            }
            std::printf("%u %u %u %" PRId64 " %" PRIu64 " %" PRIu64 " %d", s.plan, run, s.n_top, last_hi, last_lo, ties_left, roundtrip && chosen.size() == s.n_top ? 1 : 0);
            for (uint32_t j : chosen) std::printf(" %u", j);
            std::printf("\n");
        } else if (kind == 'V') {
            uint32_t rank_by = 0, has_values = 0;
            uint64_t lines = 0, numbers = 0, lo32 = 0;
            int64_t mn = 0, mx = 0, hi32 = 0;
            in >> rank_by >> has_values >> lines >> numbers >> mn >> mx >> lo32 >> hi32;
            uint64_t head[GROUP_HEAD_WORDS] = {lines, group_first_word(0)};
            uint64_t stats[GROUP_STATS_WORDS] = {};
            stats[GROUP_S_NUMBERS] = numbers;
            stats[GROUP_S_MIN] = group_min_word(mn);
            stats[GROUP_S_MAX] = group_max_word(mx);
            stats[GROUP_S_LO] = lo32;
            stats[GROUP_S_HI] = static_cast<uint64_t>(hi32);
            int64_t hi = 0;
            uint64_t lo = 0;
            // (without values the stats words do not exist: a null pointer must not be read)
            const bool c = tg_rank_value(rank_by, has_values != 0, head, has_values ? stats : static_cast<uint64_t*>(nullptr), &hi, &lo);
            std::printf("%d %" PRId64 " %" PRIu64 "\n", c ? 1 : 0, hi, lo);
        } else {
            std::printf("?\n");
        }
    }
    return 0;
}
