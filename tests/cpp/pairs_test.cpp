// The rule of gx_group_pairs (gorp_amd/csrc/gx_pairs.hpp, plain C++) as a program of its own, with the host policy (a plain
// compare-and-store) in place of the device's compare-and-swap: the very hash and probing code the kernel runs.  Cases on stdin, one
// per line, the answers on stdout in the same order; tests/test_pairs_host.py compares them with a Python dict and a restatement of the
// probing (tests/pairs_oracle.py).  Built with -fsanitize=address,undefined -fno-sanitize-recover=undefined: every second lives in a
// block of exactly its units, so a comparison that reads past one -- a prefix of its neighbour, say -- is a report.
//   T <b|w> <weak 0|1> <slots> <n> <key slot>:<second hex|->...
//        inserts the n pairs in order, pair i as line i; prints per pair its slot or "full", then "@" and the slot words it loaded, then
//        "|" and every full slot as slot:line:tag in slot order
//   H <b|w> <weak 0|1> <n> <key slot>:<second hex|->...
//        prints every pair's hash (decimal)
//   Z      prints sizeof(PairsHead) sizeof(PairsDev) PAIRS_MAX_PAIRS
// hex: two digits per unit (b: bytes) or four (w: 16-bit units); "-" is the empty string.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "gx_pairs.hpp"

template <typename UNIT>
struct Pair {
    uint32_t key_slot = 0;
    std::unique_ptr<UNIT[]> p;   // exactly n units (n = 0: a block of no bytes)
    uint32_t n = 0;
    explicit Pair(const std::string& text) {
        const size_t colon = text.find(':');
        key_slot = static_cast<uint32_t>(std::strtoul(text.substr(0, colon).c_str(), nullptr, 10));
        const std::string hex = text.substr(colon + 1);
        const size_t digits = 2 * sizeof(UNIT);
        n = hex == "-" ? 0u : static_cast<uint32_t>(hex.size() / digits);
        p.reset(new UNIT[n]);
        for (uint32_t i = 0; i < n; ++i) p[i] = static_cast<UNIT>(std::strtoul(hex.substr(i * digits, digits).c_str(), nullptr, 16));
    }
};

template <typename UNIT>
static std::vector<Pair<UNIT>> read_pairs(std::istringstream& in) {
    uint32_t n = 0;
    in >> n;
    std::vector<Pair<UNIT>> v;
    v.reserve(n);
    for (uint32_t i = 0; i < n; ++i) {
        std::string text;
        in >> text;
        v.emplace_back(text);
    }
    return v;
}

// the host policy, counting the words it loads
struct CountingTable {
    gx::PairsHostTable t;
    uint64_t loads = 0;
    uint64_t load(uint32_t slot) {
        ++loads;
        return t.load(slot);
    }
    uint64_t claim(uint32_t slot, uint64_t word) { return t.claim(slot, word); }
};

template <typename UNIT>
static void table_case(std::istringstream& in) {
    int weak = 0;
    uint32_t slots = 0;
    in >> weak >> slots;
    const std::vector<Pair<UNIT>> pairs = read_pairs<UNIT>(in);
    std::unique_ptr<uint64_t[]> words(new uint64_t[slots]());   // exactly `slots` words
    CountingTable table{gx::PairsHostTable{words.get()}};
    for (uint32_t i = 0; i < pairs.size(); ++i) {
        const UNIT* v = pairs[i].p.get();
        table.loads = 0;
        const uint32_t slot = gx::pair_find_or_insert(table, slots, pairs[i].key_slot, i, v, pairs[i].n, weak != 0, [&](uint32_t rep, uint32_t& key_slot, uint32_t& units) {
            key_slot = pairs[rep].key_slot;
            units = pairs[rep].n;
            return static_cast<const UNIT*>(pairs[rep].p.get());
        });
        if (slot == gx::GROUP_NONE) printf("full@%" PRIu64 " ", table.loads);
        else printf("%u@%" PRIu64 " ", slot, table.loads);
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
    const std::vector<Pair<UNIT>> pairs = read_pairs<UNIT>(in);
    for (const Pair<UNIT>& v : pairs) printf("%" PRIu64 " ", gx::pair_hash(gx::group_hash(v.p.get(), v.n, false), v.key_slot, weak != 0));
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
        } else if (kind == "Z") {
            printf("%zu %zu %" PRIu64 "\n", sizeof(gx::PairsHead), sizeof(gx::PairsDev), static_cast<uint64_t>(gx::PAIRS_MAX_PAIRS));
        } else {
            fprintf(stderr, "unknown case: %s\n", row.c_str());
            return 2;
        }
    }
    return 0;
}
