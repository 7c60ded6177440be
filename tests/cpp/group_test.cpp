// The find-or-insert of gx_group_lines (gorp_amd/csrc/gx_group.hpp, plain C++) as a program of its own, with the host policy (a plain
// compare-and-store) in place of the device's compare-and-swap: the very probing code the kernel runs.  Cases on stdin, one per line,
// the answers on stdout in the same order; tests/test_group_host.py compares them with a Python dict.  Built with
// -fsanitize=address,undefined -fno-sanitize-recover=undefined: every value lives in a block of exactly its units, so a comparison
// that reads past a value -- a prefix of its neighbour, say -- is a report.
//   T <b|w> <weak 0|1> <slots> <n> <value hex|->...
//        inserts the n values in order, value i as line i; prints per value its slot or "full", then "|" and every full slot as
//        slot:line:tag in slot order
//   H <b|w> <weak 0|1> <n> <value hex|->...
//        prints every value's hash (decimal)
//   S <max_keys>
//        prints group_slots(max_keys)
// hex: two digits per unit (b: bytes) or four (w: 16-bit units); "-" is the empty string.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "gx_group.hpp"

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
static std::vector<Units<UNIT>> read_values(std::istringstream& in) {
    uint32_t n = 0;
    in >> n;
    std::vector<Units<UNIT>> v;
    v.reserve(n);
    for (uint32_t i = 0; i < n; ++i) {
        std::string hex;
        in >> hex;
        v.emplace_back(hex);
    }
    return v;
}

template <typename UNIT>
static void table_case(std::istringstream& in) {
    int weak = 0;
    uint32_t slots = 0;
    in >> weak >> slots;
    const std::vector<Units<UNIT>> values = read_values<UNIT>(in);
    std::unique_ptr<uint64_t[]> words(new uint64_t[slots]());   // exactly `slots` words
    gx::GroupHostTable table{words.get()};
    for (uint32_t i = 0; i < values.size(); ++i) {
        const UNIT* v = values[i].p.get();
        const uint32_t vn = values[i].n;
        const uint32_t slot = gx::group_find_or_insert(table, slots, gx::group_hash(v, vn, weak != 0), i, v, vn, [&](uint32_t rep, const UNIT* a, uint32_t an) {
            return gx::group_same_key(a, an, values[rep].p.get(), values[rep].n);
        });
        if (slot == gx::GROUP_NONE) printf("full ");
        else printf("%u ", slot);
    }
    printf("|");
    for (uint32_t s = 0; s < slots; ++s)
        if (words[s]) printf(" %u:%u:%u", s, gx::group_word_line(words[s]), gx::group_tag(words[s]));
    printf("\n");
}

template <typename UNIT>
static void hash_case(std::istringstream& in) {
    int weak = 0;
    in >> weak;
    const std::vector<Units<UNIT>> values = read_values<UNIT>(in);
    for (const Units<UNIT>& v : values) printf("%" PRIu64 " ", gx::group_hash(v.p.get(), v.n, weak != 0));
    printf("\n");
}

int main() {
    std::string row;
    while (std::getline(std::cin, row)) {
        if (row.empty()) continue;
        std::istringstream in(row);
        std::string kind, unit;
        in >> kind;
        if (kind == "T" || kind == "H") {
            in >> unit;
            if (kind == "T") {
                if (unit == "w") table_case<uint16_t>(in);
                else table_case<uint8_t>(in);
            } else {
                if (unit == "w") hash_case<uint16_t>(in);
                else hash_case<uint8_t>(in);
            }
        } else if (kind == "S") {
            uint64_t max_keys = 0;
            in >> max_keys;
            printf("%u\n", gx::group_slots(max_keys));
        } else {
            fprintf(stderr, "unknown case: %s\n", row.c_str());
            return 2;
        }
    }
    return 0;
}
