// The rule of gx_group_series (gorp_amd/csrc/gx_series.hpp, plain C++) as a program of its own, with the host policy (a plain
// compare-and-store) in place of the device's compare-and-swap: the very cell word, sort word, digit plan and find-or-insert code the
// kernels run.  Cases on stdin, one per line, the answers on stdout in the same order; tests/test_series_host.py compares them with the
// Python forms (tests/series_oracle.py).  Built with -fsanitize=address,undefined -fno-sanitize-recover=undefined: an overflow in a word
// or a probe past a table is a report.
//   C <n> <kslot> <bslot> ...              prints per pair word:kslot:bslot (the word and what it gives back)
//   S <n> <key> <rank> <n_buckets> ...     prints per triple sort_word
//   D <n> <n_keys> <n_buckets> ...         prints per pair series_digits
//   T <weak 0|1> <slots> <n> <kslot> <bucket> ...  runs the n (key slot, bucket number) lines through BOTH tables in order: the bucket word
//                                          into the bucket table, cell_word(kslot, bslot) into the cell table; prints per line bslot:cslot
//                                          ("full" where a table is), then "|" and every full bucket slot as slot:word, then "|" and every
//                                          full cell slot as slot:word
//   Z      prints sizeof(SeriesHead) sizeof(SeriesDev) SERIES_MAX_CELLS
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

#include "gx_series.hpp"

static int64_t read_i64(std::istringstream& in) {
    std::string s;
    in >> s;
    return static_cast<int64_t>(std::strtoll(s.c_str(), nullptr, 10));
}
static uint64_t read_u64(std::istringstream& in) {
    std::string s;
    in >> s;
    return static_cast<uint64_t>(std::strtoull(s.c_str(), nullptr, 10));
}

int main() {
    std::string row;
    while (std::getline(std::cin, row)) {
        if (row.empty()) continue;
        std::istringstream in(row);
        std::string kind;
        in >> kind;
        if (kind == "C") {
            const uint64_t n = read_u64(in);
            for (uint64_t i = 0; i < n; ++i) {
                const uint32_t k = static_cast<uint32_t>(read_u64(in)), b = static_cast<uint32_t>(read_u64(in));
                const uint64_t w = gx::cell_word(k, b);
                printf("%" PRIu64 ":%u:%u ", w, gx::cell_kslot(w), gx::cell_bslot(w));
            }
            printf("\n");
        } else if (kind == "S") {
            const uint64_t n = read_u64(in);
            for (uint64_t i = 0; i < n; ++i) {
                const uint64_t k = read_u64(in), r = read_u64(in), nb = read_u64(in);
                printf("%" PRIu64 " ", gx::sort_word(k, r, nb));
            }
            printf("\n");
        } else if (kind == "D") {
            const uint64_t n = read_u64(in);
            for (uint64_t i = 0; i < n; ++i) {
                const uint64_t k = read_u64(in), b = read_u64(in);
                printf("%u ", gx::series_digits(k, b));
            }
            printf("\n");
        } else if (kind == "T") {
            const int weak = static_cast<int>(read_u64(in));
            const uint32_t slots = static_cast<uint32_t>(read_u64(in));
            const uint64_t n = read_u64(in);
            std::unique_ptr<uint64_t[]> bwords(new uint64_t[slots]()), cwords(new uint64_t[slots]());   // exactly `slots` words each
            gx::BucketHostTable bt{bwords.get()}, ct{cwords.get()};
            for (uint64_t i = 0; i < n; ++i) {
                const uint32_t kslot = static_cast<uint32_t>(read_u64(in));
                const int64_t bucket = read_i64(in);
                const uint32_t bslot = gx::bucket_find_or_insert(bt, slots, gx::bucket_word(bucket), weak != 0);
                if (bslot == gx::GROUP_NONE) {
                    printf("full:full ");
                    continue;
                }
                const uint32_t cslot = gx::bucket_find_or_insert(ct, slots, gx::cell_word(kslot, bslot), weak != 0);
                if (cslot == gx::GROUP_NONE) printf("%u:full ", bslot);
                else printf("%u:%u ", bslot, cslot);
            }
            printf("|");
            for (uint32_t s = 0; s < slots; ++s)
                if (bwords[s]) printf(" %u:%" PRIu64, s, bwords[s]);
            printf(" |");
            for (uint32_t s = 0; s < slots; ++s)
                if (cwords[s]) printf(" %u:%" PRIu64, s, cwords[s]);
            printf("\n");
        } else if (kind == "Z") {
            printf("%zu %zu %" PRIu64 "\n", sizeof(gx::SeriesHead), sizeof(gx::SeriesDev), static_cast<uint64_t>(gx::SERIES_MAX_CELLS));
        } else {
            fprintf(stderr, "unknown case: %s\n", row.c_str());
            return 2;
        }
    }
    return 0;
}
