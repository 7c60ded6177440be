// The rule of gx_bucket_lines (gorp_amd/csrc/gx_bucket.hpp, plain C++) as a program of its own, with the host policy (a plain
// compare-and-store) in place of the device's compare-and-swap: the very bucket, hash, probing and digit-plan code the kernels run.
// Cases on stdin, one per line, the answers on stdout in the same order; tests/test_bucket_host.py compares them with Python's // on
// unbounded ints and a restatement of the probing (tests/bucket_oracle.py).  Built with -fsanitize=address,undefined
// -fno-sanitize-recover=undefined: a signed overflow in bucket_of or a probe past the table is a report.
//   B <n> <v> <origin> <width> ...     prints per triple the bucket, or "x" (out of range)
//   T <weak 0|1> <slots> <n> <word> ... inserts the n words (decimal, unsigned) in order; prints per word its slot or "full", then "@" and
//                                      the slot words it loaded, then "|" and every full slot as slot:word in slot order
//   H <weak 0|1> <n> <word> ...        prints every word's hash (decimal)
//   D <n> <min word> <max word> ...    prints per pair bucket_digits
//   W <n> <bucket> ...                 prints per bucket its word and the bucket the word gives back
//   Z      prints sizeof(BucketHead) sizeof(BucketDev) BUCKET_MAX_BUCKETS BUCKET_WG_LINES BUCKET_MAX_DIGITS
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "gx_bucket.hpp"

// the host policy, counting the words it loads
struct CountingTable {
    gx::BucketHostTable t;
    uint64_t loads = 0;
    uint64_t load(uint32_t slot) {
        ++loads;
        return t.load(slot);
    }
    uint64_t claim(uint32_t slot, uint64_t word) { return t.claim(slot, word); }
};

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
        if (kind == "B") {
            const uint64_t n = read_u64(in);
            for (uint64_t i = 0; i < n; ++i) {
                const int64_t v = read_i64(in), origin = read_i64(in);
                const uint64_t width = read_u64(in);
                int64_t b = 12345;
                if (gx::bucket_of(v, origin, width, &b)) printf("%" PRId64 " ", b);
                else fputs(b == 12345 ? "x " : "touched ", stdout);
            }
            printf("\n");
        } else if (kind == "T") {
            const int weak = static_cast<int>(read_u64(in));
            const uint32_t slots = static_cast<uint32_t>(read_u64(in));
            const uint64_t n = read_u64(in);
            std::unique_ptr<uint64_t[]> words(new uint64_t[slots]());   // exactly `slots` words
            CountingTable table{gx::BucketHostTable{words.get()}};
            for (uint64_t i = 0; i < n; ++i) {
                const uint64_t word = read_u64(in);
                table.loads = 0;
                const uint32_t slot = gx::bucket_find_or_insert(table, slots, word, weak != 0);
                if (slot == gx::GROUP_NONE) printf("full@%" PRIu64 " ", table.loads);
                else printf("%u@%" PRIu64 " ", slot, table.loads);
            }
            printf("|");
            for (uint32_t s = 0; s < slots; ++s)
                if (words[s]) printf(" %u:%" PRIu64, s, words[s]);
            printf("\n");
        } else if (kind == "H") {
            const int weak = static_cast<int>(read_u64(in));
            const uint64_t n = read_u64(in);
            for (uint64_t i = 0; i < n; ++i) printf("%" PRIu64 " ", gx::bucket_hash(read_u64(in), weak != 0));
            printf("\n");
        } else if (kind == "D") {
            const uint64_t n = read_u64(in);
            for (uint64_t i = 0; i < n; ++i) {
                const uint64_t a = read_u64(in), b = read_u64(in);
                printf("%u ", gx::bucket_digits(a, b));
            }
            printf("\n");
        } else if (kind == "W") {
            const uint64_t n = read_u64(in);
            for (uint64_t i = 0; i < n; ++i) {
                const int64_t b = read_i64(in);
                printf("%" PRIu64 ":%" PRId64 " ", gx::bucket_word(b), gx::bucket_number(gx::bucket_word(b)));
            }
            printf("\n");
        } else if (kind == "Z") {
            printf("%zu %zu %" PRIu64 " %u %u\n", sizeof(gx::BucketHead), sizeof(gx::BucketDev), static_cast<uint64_t>(gx::BUCKET_MAX_BUCKETS), gx::BUCKET_WG_LINES,
                   gx::BUCKET_MAX_DIGITS);
        } else {
            fprintf(stderr, "unknown case: %s\n", row.c_str());
            return 2;
        }
    }
    return 0;
}
