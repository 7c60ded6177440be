// lookup_test.cpp -- the rule of gx_lookup_lines (gorp_amd/csrc/gx_lookup.hpp) as a program of its own, built by tests/test_cpp_lookup.py
// with g++ alone (-fsanitize=address,undefined): the find-only probe against find-or-insert on a GroupHostTable with drawn dictionaries in
// 64- and 128-slot tables, under the weak hash too; chains that run past the last slot to slot 0; a miss ended by the first empty slot
// (the slots a probe reads are counted); duplicates inserted in every order giving the same entry_same; the empty entry; entries that
// are prefixes of each other; entries that differ in the last unit only; the classes and keep.  Prints "lookup rule ok".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "gx_lookup.hpp"

using namespace gx;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

typedef std::vector<uint8_t> Text;

static Text text(const std::string& s) { return Text(s.begin(), s.end()); }

// a dictionary on the host as the kernels hold one: the table, the lowest-entry words, every entry's slot
struct Dict {
    std::vector<Text> entries;
    uint32_t n_slots = 0;
    bool weak = false;
    std::vector<uint64_t> words, low;
    std::vector<uint32_t> slot_of_entry;
    mutable uint64_t loads = 0;

    // k_lookup_build over the entries in `order`: which duplicate claims a slot is the order's
    bool build(const std::vector<Text>& e, const std::vector<uint32_t>& order, uint32_t slots, bool weak_hash) {
        entries = e;
        n_slots = slots;
        weak = weak_hash;
        words.assign(slots, 0);
        low.assign(slots, 0);
        slot_of_entry.assign(e.size(), GROUP_NONE);
        GroupHostTable tab{words.data()};
        for (uint32_t j : order) {
            const Text& t = entries[j];
            // (data() of an empty vector may be null: group_hash and where_same read nothing of a value of no units)
            const uint32_t slot = group_find_or_insert(tab, n_slots, group_hash(t.data(), static_cast<uint32_t>(t.size()), weak), j, t.data(),
                                                       static_cast<uint32_t>(t.size()), [&](uint32_t rep, const uint8_t* a, uint32_t an) {
                                                           return group_same_key(a, an, entries[rep].data(), static_cast<uint32_t>(entries[rep].size()));
                                                       });
            if (slot == GROUP_NONE) return false;
            low[slot] = std::max(low[slot], lookup_low_word(j));
            slot_of_entry[j] = slot;
        }
        return true;
    }
    struct Loads {
        const Dict* d;
        uint64_t load(uint32_t slot) const { ++d->loads; return d->words.at(slot); }
    };
    uint32_t find(const Text& v) const {
        const Loads tab{this};
        return lookup_find(tab, n_slots, group_hash(v.data(), static_cast<uint32_t>(v.size()), weak), v.data(), static_cast<uint32_t>(v.size()),
                           [&](uint32_t rep, const uint8_t* a, uint32_t an) { return group_same_key(a, an, entries.at(rep).data(), static_cast<uint32_t>(entries[rep].size())); });
    }
    // what is delivered for a key: the lowest entry with its text, or LOOKUP_MISS
    uint32_t entry_of(const Text& v) const {
        const uint32_t slot = find(v);
        return slot == LOOKUP_MISS ? LOOKUP_MISS : lookup_low_entry(low.at(slot));
    }
    uint32_t same(uint32_t j) const { return lookup_low_entry(low.at(slot_of_entry.at(j))); }
};

static std::vector<uint32_t> ascending(size_t m) {
    std::vector<uint32_t> o(m);
    for (uint32_t j = 0; j < m; ++j) o[j] = j;
    return o;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t draw(uint32_t below) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<uint32_t>(rng_state >> 33) % below;
}

// the dictionary against a std::map filled with putIfAbsent, for keys drawn from the entries and around them
static int against_map(const Dict& d, const std::vector<Text>& keys) {
    std::map<Text, uint32_t> index;
    for (uint32_t j = 0; j < d.entries.size(); ++j) index.emplace(d.entries[j], j);   // (emplace keeps the first: putIfAbsent)
    for (uint32_t j = 0; j < d.entries.size(); ++j) CHECK(d.same(j) == index[d.entries[j]]);
    for (const Text& k : keys) {
        const auto it = index.find(k);
        d.loads = 0;
        const uint32_t got = d.entry_of(k);
        CHECK(got == (it == index.end() ? LOOKUP_MISS : it->second));
        CHECK(d.loads <= d.n_slots);                        // every slot at most once
        // find-only agrees with find-or-insert on a copy of the table: a hit is the same slot, a miss is where the key would go
        std::vector<uint64_t> copy = d.words;
        GroupHostTable tab{copy.data()};
        const uint32_t slot = group_find_or_insert(tab, d.n_slots, group_hash(k.data(), static_cast<uint32_t>(k.size()), d.weak), 0x3FFFFFFFu, k.data(),
                                                   static_cast<uint32_t>(k.size()), [&](uint32_t rep, const uint8_t* a, uint32_t an) {
                                                       return rep != 0x3FFFFFFFu && group_same_key(a, an, d.entries.at(rep).data(), static_cast<uint32_t>(d.entries[rep].size()));
                                                   });
        if (it != index.end()) CHECK(slot == d.find(k) && copy == d.words);
        else CHECK(slot != GROUP_NONE && d.words[slot] == 0 && copy[slot] != 0);
    }
    return 0;
}

int main() {
    // the words
    CHECK(lookup_word(0xABCD1234u, 0) == 0xABCD123400000001ull && lookup_word_entry(lookup_word(7, (1u << 30) - 1)) == (1u << 30) - 1 && lookup_word(0, 0) != 0);
    CHECK(lookup_low_entry(lookup_low_word(0)) == 0 && lookup_low_word(0) > lookup_low_word(1) && lookup_low_word((1u << 30) - 1) != 0);
    CHECK(LOOKUP_MISS == 0xFFFFFFFEu && LOOKUP_NONE == 0xFFFFFFFFu && group_slots(LOOKUP_MAX_ENTRIES) == (1u << 31) && group_slots(0) == 64);
    // the classes and keep
    CHECK(lookup_class(false, true, 5) == LOOKUP_SKIPPED && lookup_class(true, false, LOOKUP_NONE) == LOOKUP_UNSET && lookup_class(true, true, 5) == LOOKUP_HIT &&
          lookup_class(true, true, LOOKUP_MISS) == LOOKUP_IS_MISS);
    for (uint32_t cls = LOOKUP_SKIPPED; cls <= LOOKUP_IS_MISS; ++cls) {
        CHECK(!lookup_keeps(LOOKUP_KEEP_NOTHING, cls));
        CHECK(lookup_keeps(LOOKUP_KEEP_HITS, cls) == (cls == LOOKUP_HIT));
        CHECK(lookup_keeps(LOOKUP_KEEP_OTHERS, cls) == (cls == LOOKUP_UNSET || cls == LOOKUP_IS_MISS));
    }

    // drawn dictionaries in 64- and 128-slot tables, strong and weak: entries of 0 .. 5 units over a small alphabet, so that duplicates,
    // prefixes and texts that differ in the last unit all occur; keys drawn the same way hit and miss
    for (uint32_t round = 0; round < 200; ++round) {
        const uint32_t m = round % 2 ? 1 + draw(32) : 33 + draw(32);         // 64 slots up to 32 entries, 128 beyond
        std::vector<Text> entries(m), keys;
        for (Text& e : entries) {
            e.resize(draw(6));
            for (uint8_t& u : e) u = static_cast<uint8_t>('a' + draw(3));
        }
        for (uint32_t q = 0; q < 200; ++q) {
            Text k(draw(6));
            for (uint8_t& u : k) u = static_cast<uint8_t>('a' + draw(3));
            keys.push_back(k);
        }
        for (const Text& e : entries) keys.push_back(e);
        Dict d;
        CHECK(group_slots(m) == (m <= 32 ? 64u : 128u));
        CHECK(d.build(entries, ascending(m), group_slots(m), (round & 2) != 0));
        if (against_map(d, keys)) return 1;
        // the same entries inserted backwards and shuffled: other representatives, the same entry_same and the same answers
        std::vector<uint32_t> order = ascending(m);
        std::reverse(order.begin(), order.end());
        Dict r;
        CHECK(r.build(entries, order, group_slots(m), (round & 2) != 0));
        for (uint32_t j = m; j > 1; --j) std::swap(order[j - 1], order[draw(j)]);
        Dict s;
        CHECK(s.build(entries, order, group_slots(m), (round & 2) != 0));
        for (uint32_t j = 0; j < m; ++j) CHECK(r.same(j) == d.same(j) && s.same(j) == d.same(j));
        for (const Text& k : keys) CHECK(r.entry_of(k) == d.entry_of(k) && s.entry_of(k) == d.entry_of(k));
    }

    // duplicates in every order: three entries with one text among others, all 5! orders of insertion
    {
        const std::vector<Text> entries = {text("x"), text("dup"), text("y"), text("dup"), text("dup")};
        std::vector<uint32_t> order = ascending(5);
        uint32_t orders = 0;
        do {
            Dict d;
            CHECK(d.build(entries, order, 64, false));
            CHECK(d.same(0) == 0 && d.same(1) == 1 && d.same(2) == 2 && d.same(3) == 1 && d.same(4) == 1 && d.entry_of(text("dup")) == 1);
            CHECK(lookup_word_entry(d.words[d.slot_of_entry[1]]) == *std::find_if(order.begin(), order.end(), [](uint32_t j) { return j == 1 || j >= 3; }));
            ++orders;
        } while (std::next_permutation(order.begin(), order.end()));
        CHECK(orders == 120);
    }

    // chains that run past the last slot to slot 0, and a miss that ends at the first empty slot
    {
        std::vector<Text> last, inside;     // texts whose probe starts in the last three slots of a 64-slot table; in the first three
        for (uint32_t j = 0; last.size() < 6 || inside.size() < 6; ++j) {
            const Text t = text("w" + std::to_string(j));
            const uint32_t first = group_first_slot(group_hash(t.data(), static_cast<uint32_t>(t.size()), false), 64);
            if (first >= 61 && last.size() < 6) last.push_back(t);
            else if (first < 3 && inside.size() < 6) inside.push_back(t);
        }
        Dict d;
        CHECK(d.build(last, ascending(6), 64, false));
        uint32_t wrapped = 0;
        for (uint32_t j = 0; j < 6; ++j) wrapped += d.slot_of_entry[j] < 3 ? 1u : 0u;
        CHECK(wrapped >= 3 && d.words[0] != 0 && d.words[1] != 0 && d.words[2] != 0);   // six entries, three slots before the end: three and more went round to 0, 1, 2
        for (uint32_t j = 0; j < 6; ++j) CHECK(d.entry_of(last[j]) == j);
        for (const Text& k : inside) {                           // a miss that starts inside the chain: it reads up to the first empty slot and no further
            uint32_t s = group_first_slot(group_hash(k.data(), static_cast<uint32_t>(k.size()), false), 64);
            uint64_t expect = 1;
            for (; d.words[s] != 0; s = (s + 1u) & 63u) ++expect;
            d.loads = 0;
            CHECK(d.find(k) == LOOKUP_MISS && d.loads == expect && expect >= 2);
        }
        Dict none;
        CHECK(none.build({}, {}, 64, false) && none.find(text("anything")) == LOOKUP_MISS && none.loads == 1);   // m == 0: every key misses at its first slot
        // a table with no empty slot at all (never built by the call: the bound alone ends the probe)
        std::vector<Text> full(64);
        for (uint32_t j = 0; j < 64; ++j) full[j] = text("f" + std::to_string(j));
        Dict f;
        CHECK(f.build(full, ascending(64), 64, false));
        CHECK(f.find(text("absent")) == LOOKUP_MISS && f.loads == 64);
        for (uint32_t j = 0; j < 64; ++j) CHECK(f.entry_of(full[j]) == j);
    }

    // the empty entry; prefixes of each other; entries that differ in the last unit only -- strong and weak
    for (int weak = 0; weak < 2; ++weak) {
        const std::vector<Text> entries = {text("abc"), text(""), text("ab"), text("abd"), text("a"), text("abcd")};
        Dict d;
        CHECK(d.build(entries, ascending(entries.size()), 64, weak != 0));
        for (uint32_t j = 0; j < entries.size(); ++j) CHECK(d.entry_of(entries[j]) == j);
        CHECK(d.entry_of(text("abe")) == LOOKUP_MISS && d.entry_of(text("abcde")) == LOOKUP_MISS && d.entry_of(text("b")) == LOOKUP_MISS);
        Dict without;
        CHECK(without.build({text("abc"), text("ab")}, ascending(2), 64, weak != 0));
        CHECK(without.entry_of(text("")) == LOOKUP_MISS && without.entry_of(text("a")) == LOOKUP_MISS && without.entry_of(text("ab")) == 1);
    }
    printf("lookup rule ok\n");
    return 0;
}
