// The rule of gx_select_lines_where (gorp_amd/csrc/gx_where.hpp, plain C++) as a program of its own: cases on stdin, one per line, the
// answers on stdout in the same order; tests/test_where_host.py compares them with a restatement in Python.  Built with
// -fsanitize=address,undefined: every buffer is allocated with exactly its units, so a read behind a value's or a literal's end is a
// report, not a wrong answer that happens to come out right.
//   T <b|w> <op> <negate> <buffer hex|-> <begin> <end> <literal hex|-> <number>
//         the term on the value buffer[begin, end), the line being the whole buffer; prints 0 / 1
//   I <b|w> <value hex|->          where_parse_int64; prints "no" or the number
//   P <begin> <end> <line units>   where_pair_set; prints 0 / 1
// hex: two digits per unit (b: bytes) or four (w: 16-bit units); "-" is the empty string.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

#include "gx_where.hpp"

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
int term(std::istringstream& in) {
    uint32_t op = 0, negate = 0;
    int64_t begin = 0, end = 0, number = 0;
    std::string buffer, literal;
    in >> op >> negate >> buffer >> begin >> end >> literal >> number;
    const Units<UNIT> line(buffer), lit(literal);
    bool holds = false;
    if (gx::where_pair_set(begin, end, line.n))
        holds = gx::where_test(op, line.p.get() + begin, static_cast<uint32_t>(end - begin), lit.p.get(), lit.n, number);
    return holds != (negate != 0) ? 1 : 0;
}

template <typename UNIT>
void parse(std::istringstream& in) {
    std::string value;
    in >> value;
    const Units<UNIT> v(value);
    int64_t out = 0;
    if (gx::where_parse_int64(v.p.get(), v.n, &out)) printf("%" PRId64 "\n", out);
    else printf("no\n");
}

int main() {
    std::string row;
    while (std::getline(std::cin, row)) {
        if (row.empty()) continue;
        std::istringstream in(row);
        std::string kind, unit;
        in >> kind;
        if (kind == "T") {
            in >> unit;
            printf("%d\n", unit == "w" ? term<uint16_t>(in) : term<uint8_t>(in));
        } else if (kind == "I") {
            in >> unit;
            if (unit == "w") parse<uint16_t>(in);
            else parse<uint8_t>(in);
        } else if (kind == "P") {
            int64_t b = 0, e = 0;
            uint64_t units = 0;
            in >> b >> e >> units;
            printf("%d\n", gx::where_pair_set(b, e, units) ? 1 : 0);
        } else {
            fprintf(stderr, "unknown case: %s\n", row.c_str());
            return 2;
        }
    }
    return 0;
}
