// The rule of gx_capture_stats (gorp_amd/csrc/gx_stats.hpp, plain C++) as a program of its own: cases on stdin, one per line, the
// answers on stdout in the same order; tests/test_stats_host.py compares them with Python's big integers.  Built with
// -fsanitize=address,undefined -fno-sanitize-recover=undefined: the edges are allocated with exactly their entries, so a probe outside
// them is a report, and a signed sum that left int64 would end the program -- that it does not is the proof that nothing wraps.
//   B <n_edges> <edge>... <v>           stats_bucket; prints the bucket
//   A <chunk> <runs> (<count> <what>)...
//                                       the accumulator over runs of `count` times `what` (a number, "u" = unset, "x" = no number),
//                                       a fresh accumulator every `chunk` lines merged into the total; prints
//                                       lines numbers unset not_numbers min max lo hi sum_hi sum_lo
//   C <lo> <hi>                         stats_sum128; prints sum_hi sum_lo
//   S <b|w> <value hex|-> <pair set 0|1> <n_edges> <edge>...
//                                       stats_add on one value; prints "unset", "nan" or the bucket, then numbers min max
// hex: two digits per unit (b: bytes) or four (w: 16-bit units); "-" is the empty string.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

#include "gx_stats.hpp"

struct Edges {
    std::unique_ptr<int64_t[]> p;   // exactly n entries (n = 0: a block of no bytes)
    uint32_t n = 0;
    explicit Edges(std::istringstream& in) {
        in >> n;
        p.reset(new int64_t[n]);
        for (uint32_t i = 0; i < n; ++i) in >> p[i];
    }
};

template <typename UNIT>
struct Units {
    std::unique_ptr<UNIT[]> p;
    uint32_t n = 0;
    explicit Units(const std::string& hex) {
        const size_t digits = 2 * sizeof(UNIT);
        n = hex == "-" ? 0u : static_cast<uint32_t>(hex.size() / digits);
        p.reset(new UNIT[n]);
        for (uint32_t i = 0; i < n; ++i) p[i] = static_cast<UNIT>(std::strtoul(hex.substr(i * digits, digits).c_str(), nullptr, 16));
    }
};

static void accumulate(std::istringstream& in) {
    uint64_t chunk = 0, runs = 0, in_chunk = 0;
    in >> chunk >> runs;
    gx::StatsAcc total, part;
    for (uint64_t r = 0; r < runs; ++r) {
        uint64_t count = 0;
        std::string what;
        in >> count >> what;
        const int64_t v = (what == "u" || what == "x") ? 0 : static_cast<int64_t>(std::strtoll(what.c_str(), nullptr, 10));
        for (uint64_t c = 0; c < count; ++c) {
            if (what == "u") part.add_unset();
            else if (what == "x") part.add_not_number();
            else part.add_number(v);
            if (++in_chunk == chunk) {
                total.merge(part);
                part = gx::StatsAcc();
                in_chunk = 0;
            }
        }
    }
    total.merge(part);
    uint64_t sum_lo = 0;
    int64_t sum_hi = 0;
    gx::stats_sum128(total.lo, total.hi, &sum_lo, &sum_hi);
    printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRId64 " %" PRId64 " %" PRIu64 " %" PRId64 " %" PRId64 " %" PRIu64 "\n", total.lines(), total.numbers,
           total.unset, total.not_numbers, total.min, total.max, total.lo, total.hi, sum_hi, sum_lo);
}

template <typename UNIT>
static void one_value(std::istringstream& in) {
    std::string value;
    int set = 0;
    in >> value >> set;
    const Units<UNIT> v(value);
    const Edges e(in);
    gx::StatsAcc a;
    const uint32_t b = gx::stats_add(a, set != 0, v.p.get(), v.n, e.p.get(), e.n);
    if (a.unset) printf("unset");
    else if (a.not_numbers) printf("nan");
    else printf("%u", b);
    printf(" %" PRIu64 " %" PRId64 " %" PRId64 "\n", a.numbers, a.min, a.max);
}

int main() {
    std::string row;
    while (std::getline(std::cin, row)) {
        if (row.empty()) continue;
        std::istringstream in(row);
        std::string kind, unit;
        in >> kind;
        if (kind == "B") {
            const Edges e(in);
            int64_t v = 0;
            in >> v;
            printf("%u\n", gx::stats_bucket(e.p.get(), e.n, v));
        } else if (kind == "A") {
            accumulate(in);
        } else if (kind == "C") {
            uint64_t lo = 0, sum_lo = 0;
            int64_t hi = 0, sum_hi = 0;
            in >> lo >> hi;
            gx::stats_sum128(lo, hi, &sum_lo, &sum_hi);
            printf("%" PRId64 " %" PRIu64 "\n", sum_hi, sum_lo);
        } else if (kind == "S") {
            in >> unit;
            if (unit == "w") one_value<uint16_t>(in);
            else one_value<uint8_t>(in);
        } else {
            fprintf(stderr, "unknown case: %s\n", row.c_str());
            return 2;
        }
    }
    return 0;
}
