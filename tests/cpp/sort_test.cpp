// sort_test.cpp -- the rule of gx_sort_lines (gorp_amd/csrc/gx_sort.hpp) as a program of its own, built by tests/test_sort_host.py
// with g++ -fsanitize=address,undefined and fed rows on stdin.
//
//   P <all_digits> <m> <key> x m               (keys in hex)
// prints: sort_plan's n_passes, sort_result_buffer, then the passes' digits
//   S <descending> <carry> <rest_last> <all_digits> <n> <value or x> x n
// the passes on the host, as the kernels make them: the candidate flags and their exclusive scan, the compaction of the stamped keys,
// the entries pass (class, place, pair; the rest lines behind the entries in both line buffers), the plan from the OR and AND of the
// entries' keys, per pass a count per digit, its exclusive scan and a scatter in input order, ping and pong, and the finish;
// prints: m carried rest leading n_passes already_ordered first_value last_value, then per output line "line value class".
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "gx_sort.hpp"

using namespace gx;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char kind = 0;
        in >> kind;
        if (kind == 'P') {
            uint32_t all = 0;
            uint64_t m = 0, key_or = 0, key_and = ~0ull;
            in >> all >> m;
            for (uint64_t i = 0; i < m; ++i) {
                uint64_t k = 0;
                in >> std::hex >> k;
                key_or |= k;
                key_and &= k;
            }
            const SortPlan p = sort_plan(key_or, key_and, m, all != 0);
            printf("%u %u", p.n_passes, sort_result_buffer(p.n_passes));
            for (uint32_t q = 0; q < p.n_passes; ++q) printf(" %u", static_cast<unsigned>(p.digit[q]));
            printf("\n");
        } else if (kind == 'S') {
            uint32_t descending = 0, carry = 0, rest_last = 0, all = 0;
            uint64_t n = 0;
            in >> descending >> carry >> rest_last >> all >> n;
            std::vector<uint8_t> cand(n, 0);
            std::vector<uint64_t> keys(n, 0xDEADBEEFDEADBEEFull), before(n + 1, 0);
            for (uint64_t i = 0; i < n; ++i) {
                std::string v;
                in >> v;
                if (v == "x") continue;
                cand[i] = 1;
                keys[i] = top_key(static_cast<int64_t>(std::stoll(v)), descending != 0);
            }
            for (uint64_t i = 0; i < n; ++i) before[i + 1] = before[i] + cand[i];
            std::vector<uint64_t> ckeys(before[n]);
            for (uint64_t i = 0; i < n; ++i)
                if (cand[i]) ckeys.at(before[i]) = keys[i];
            const uint64_t leading = sort_leading(before.data(), n);
            const uint64_t m = sort_entries(n, before[n], leading, carry != 0);
            std::vector<uint64_t> word[2];
            std::vector<uint32_t> lines[2];
            for (int q = 0; q < 2; ++q) { word[q].assign(m, 0xDEADBEEFDEADBEEFull); lines[q].assign(n, 0xDEADBEEFu); }
            std::vector<uint8_t> cls(n, 0xEE);
            uint64_t key_or = 0, key_and = ~0ull, key_min = ~0ull, key_max = 0, carried = 0, rest = 0;
            bool unordered = false;
            for (uint64_t i = 0; i < n; ++i) {
                const uint32_t c = sort_class(cand[i] != 0, before[i], carry != 0);
                cls[i] = static_cast<uint8_t>(c);
                if (c != SORT_REST) {
                    const uint64_t key = sort_entry_key(ckeys.data(), c, before[i]);   // (ASan: inside ckeys)
                    const uint64_t at = sort_entry_at(i, before[i], leading, carry != 0);
                    if (at >= m) return 4;
                    word[0].at(at) = key;
                    lines[0].at(at) = static_cast<uint32_t>(i);
                    key_or |= key;
                    key_and &= key;
                    key_min = key < key_min ? key : key_min;
                    key_max = key > key_max ? key : key_max;
                    carried += c == SORT_CARRIED ? 1u : 0u;
                    if (cand[i] && before[i] > 0 && key < ckeys.at(before[i] - 1)) unordered = true;
                } else {
                    ++rest;
                    const uint64_t at = sort_rest_at(i, before[i], m);
                    if (at < m) return 5;
                    lines[0].at(at) = static_cast<uint32_t>(i);
                    lines[1].at(at) = static_cast<uint32_t>(i);
                }
            }
            if (m + rest != n) return 6;
            const SortPlan p = sort_plan(key_or, key_and, m, all != 0);
            uint32_t cur = 0;
            for (uint32_t q = 0; q < p.n_passes; ++q) {
                const uint32_t d = p.digit[q];
                uint64_t base[GQ_BINS + 1] = {};
                for (uint64_t i = 0; i < m; ++i) ++base[bucket_digit(word[cur][i], d) + 1u];
                for (uint32_t b = 0; b < GQ_BINS; ++b) base[b + 1u] += base[b];
                for (uint64_t i = 0; i < m; ++i) {
                    const uint64_t to = base[bucket_digit(word[cur][i], d)]++;
                    word[cur ^ 1u].at(to) = word[cur][i];
                    lines[cur ^ 1u].at(to) = lines[cur][i];
                }
                cur ^= 1u;
            }
            if (cur != sort_result_buffer(p.n_passes)) return 3;
            printf("%llu %llu %llu %llu %u %d %lld %lld", static_cast<unsigned long long>(m), static_cast<unsigned long long>(carried),
                   static_cast<unsigned long long>(rest), static_cast<unsigned long long>(leading), p.n_passes, unordered ? 0 : 1,
                   m ? static_cast<long long>(top_value(key_min, descending != 0)) : 0ll, m ? static_cast<long long>(top_value(key_max, descending != 0)) : 0ll);
            const uint64_t lines_out = m + (rest_last ? rest : 0u);
            for (uint64_t j = 0; j < lines_out; ++j) {
                const uint32_t i = lines[cur].at(j);
                printf(" %u %lld %u", i, j < m ? static_cast<long long>(top_value(word[cur][j], descending != 0)) : 0ll, static_cast<unsigned>(cls.at(i)));
            }
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
