// How a captured value is read as a number (gorp_amd/csrc/gx_number.hpp, plain C++) as a program of its own: cases on stdin, one per
// line, the answers on stdout in the same order; tests/test_number_host.py compares them with a restatement in Python
// (tests/number_oracle.py).  Built with -fsanitize=address,undefined: every value is allocated with exactly its units, so a read behind
// its end is a report, not a wrong answer that happens to come out right, and a signed step that wraps is one too.
//   N <b|w> <kind> <scale> <value hex|->                        number_parse; prints "no" or the number
//   T <b|w> <kind> <scale> <op> <negate> <value hex|-> <number>  number_where_test<true> under the packed format; prints 0 / 1
//   F <kind> <scale>                                            number_format_ok, and the packed byte's round trip; prints 0 / 1
// hex: two digits per unit (b: bytes) or four (w: 16-bit units); "-" is the empty string.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

#include "gx_number.hpp"

template <typename UNIT>
struct Units {
    std::unique_ptr<UNIT[]> p;   // exactly n units (n = 0: a block of no bytes)
    uint32_t n = 0;
    explicit Units(const std::string& hex) {
        const size_t digits = 2 * sizeof(UNIT);
        n = hex == "-" ? 0u : static_cast<uint32_t>(hex.size() / digits);
        p.reset(new UNIT[n]);
        for (uint32_t i = 0; i < n; ++i) p[i] = static_cast<UNIT>(std::strtoul(hex.substr(i * digits, digits).c_str(), nullptr, 16));
    }
};

template <typename UNIT>
void parse(std::istringstream& in) {
    uint32_t kind = 0, scale = 0;
    std::string value;
    in >> kind >> scale >> value;
    const Units<UNIT> v(value);
    int64_t out = 0, packed_out = 0;
    const bool ok = gx::number_parse(kind, scale, v.p.get(), v.n, &out);
    // (the kernels' entry gives the same answer)
    const bool packed_ok = gx::number_parse_packed<true>(gx::number_pack(kind, scale), v.p.get(), v.n, &packed_out);
    if (ok != packed_ok || (ok && out != packed_out)) printf("packed differs\n");
    else if (ok) printf("%" PRId64 "\n", out);
    else printf("no\n");
}

template <typename UNIT>
int term(std::istringstream& in) {
    uint32_t kind = 0, scale = 0, op = 0, negate = 0;
    int64_t number = 0;
    std::string value;
    in >> kind >> scale >> op >> negate >> value >> number;
    const Units<UNIT> v(value);
    const UNIT* no_literal = nullptr;
    const bool holds = gx::number_where_test<true>(gx::number_pack(kind, scale), op, v.p.get(), v.n, no_literal, 0u, number);
    return holds != (negate != 0) ? 1 : 0;
}

int main() {
    std::string row;
    while (std::getline(std::cin, row)) {
        if (row.empty()) continue;
        std::istringstream in(row);
        std::string what, unit;
        in >> what;
        if (what == "N") {
            in >> unit;
            if (unit == "w") parse<uint16_t>(in);
            else parse<uint8_t>(in);
        } else if (what == "T") {
            in >> unit;
            printf("%d\n", unit == "w" ? term<uint16_t>(in) : term<uint8_t>(in));
        } else if (what == "F") {
            uint32_t kind = 0, scale = 0;
            in >> kind >> scale;
            const bool ok = gx::number_format_ok(kind, scale);
            const uint8_t packed = gx::number_pack(kind, scale);
            if (ok && (gx::number_kind(packed) != kind || gx::number_scale(packed) != scale || packed > 0x7Fu)) printf("pack differs\n");
            else printf("%d\n", ok ? 1 : 0);
        } else {
            fprintf(stderr, "unknown case: %s\n", row.c_str());
            return 2;
        }
    }
    return 0;
}
