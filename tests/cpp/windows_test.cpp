// windows_test.cpp -- the rule of gx_group_windows (gorp_amd/csrc/gx_windows.hpp) as a program of its own, built by
// tests/test_cpp_windows.py with g++ alone (-fsanitize=address,undefined): the window's predicate over the corners of int64, the trip
// rule, the peak word's tie-break, the window's 128-bit sum, and a host replay of gallop + bisect (window_lo) against a linear scan -- on
// drawn runs and on runs where the key changes at e - 1, e - 2, e - 2^k.  Prints "windows rule ok".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gx_windows.hpp"

using namespace gx;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static bool holds(int64_t f, int64_t e, int64_t window) { return window_holds_times(f, e, window); }
static bool same_both_ways(int64_t f, int64_t e, int64_t window) { return window_holds_times(f, e, window) == window_holds(top_key(f, false), top_key(e, false), window); }

// an array that counts its reads and refuses one out of bounds (at() throws): what window_lo may touch
struct Counted {
    const std::vector<uint64_t>* v;
    mutable uint64_t* reads;
    uint64_t operator[](uint32_t i) const { ++*reads; return v->at(i); }
};

// entry e's window start by the definition: walk back while the key is the same and the time within the window
static uint32_t linear_lo(const std::vector<uint64_t>& key, const std::vector<uint64_t>& word, uint32_t e, int64_t window) {
    uint32_t lo = e;
    while (lo > 0 && key[lo - 1] == key[e] && word[e] - word[lo - 1] <= static_cast<uint64_t>(window)) --lo;
    return lo;
}

static uint32_t log2_ceil(uint32_t v) { uint32_t b = 0; while ((1ull << b) < v) ++b; return b; }

// every entry of an order (keys ascending, times ascending inside a key) through window_lo, against the linear scan; the loads are
// bounded by the window's own length, not by the entries before it
static int replay(const std::vector<uint64_t>& key, const std::vector<int64_t>& time, int64_t window) {
    const uint32_t m = static_cast<uint32_t>(key.size());
    std::vector<uint64_t> word(m);
    for (uint32_t e = 0; e < m; ++e) word[e] = top_key(time[e], false);
    uint32_t prev_lo = 0;
    for (uint32_t e = 0; e < m; ++e) {
        uint64_t reads = 0;
        const Counted k{&key, &reads}, t{&word, &reads};
        const uint32_t lo = window_lo(k, t, e, window);
        const uint32_t want = linear_lo(key, word, e, window);
        CHECK(lo == want && lo <= e);
        if (e > 0 && key[e - 1] == key[e]) CHECK(lo >= prev_lo);   // lo never decreases along a key
        prev_lo = lo;
        const uint32_t lines = e - lo + 1u;
        CHECK(reads <= 2u + 4u * (2u * log2_ceil(lines + 1u) + 2u));   // (key and time per probe: O(log window_lines))
        for (uint32_t f = lo; f <= e; ++f) CHECK(key[f] == key[e] && holds(time[f], time[e], window));
        if (lo > 0 && key[lo - 1] == key[e]) CHECK(!holds(time[lo - 1], time[e], window));
    }
    return 0;
}

int main() {
    const int64_t lo = INT64_MIN, hi = INT64_MAX;
    // the corners of int64
    CHECK(!holds(lo, hi, hi) && same_both_ways(lo, hi, hi));                                  // 2^64 - 1 exceeds every window
    CHECK(holds(5, 5, 0) && holds(lo, lo, 0) && holds(hi, hi, 0) && holds(-1, -1, hi));       // equal times are in every window
    CHECK(!holds(5, 6, 0) && !holds(-1, 0, 0) && !holds(lo, lo + 1, 0));                      // window 0: the same time alone
    CHECK(holds(lo, -1, hi) && !holds(lo, 0, hi) && holds(0, hi, hi) && !holds(-1, hi, hi));  // a difference of exactly INT64_MAX, and one more
    CHECK(holds(-100, -70, 30) && !holds(-100, -69, 30) && holds(hi - 30, hi, 30) && !holds(hi - 31, hi, 30) && holds(lo, lo + 30, 30) && !holds(lo, lo + 31, 30));
    const int64_t corners[] = {lo, lo + 1, -31, -30, -1, 0, 1, 30, 31, hi - 1, hi};
    const int64_t windows[] = {0, 1, 30, hi - 1, hi};
    for (const int64_t a : corners)
        for (const int64_t b : corners)
            for (const int64_t w : windows)
                if (a <= b) CHECK(same_both_ways(a, b, w));
    // the trip rule: the edge, not the level; threshold 0 never; threshold 1 at a key's head alone
    CHECK(window_trips(3, false, 2, 3) && !window_trips(4, false, 3, 3) && !window_trips(2, false, 1, 3) && window_trips(3, true, 0, 3) && window_trips(5, true, 9, 3));
    CHECK(!window_trips(1, true, 0, 0) && !window_trips(9, false, 0, 0));
    CHECK(window_trips(1, true, 0, 1) && !window_trips(1, false, 1, 1) && !window_trips(2, false, 1, 1));
    CHECK(window_trips(0xFFFFFFFFu, false, 0xFFFFFFFEu, 0xFFFFFFFFu) && !window_trips(0xFFFFFFFEu, true, 0, 0xFFFFFFFFu));
    {   // one key's counts 1 2 3 4 1 2 3 under threshold 3: trips at the third and again after the fall
        const uint32_t lines[] = {1, 2, 3, 4, 1, 2, 3};
        uint32_t trips = 0;
        for (uint32_t e = 0; e < 7; ++e) trips |= (window_trips(lines[e], e == 0, e ? lines[e - 1] : 0, 3) ? 1u : 0u) << e;
        CHECK(trips == ((1u << 2) | (1u << 6)));
    }
    // the peak word: the most lines, then the smallest entry; never 0
    CHECK(window_peak_word(4, 3) > window_peak_word(4, 13) && window_peak_word(5, 13) > window_peak_word(4, 3) && window_peak_word(1, 0) > window_peak_word(1, 1));
    CHECK(window_peak_word(1, 0xFFFFFFFFu) != 0 && window_peak_word(1, (1u << 30) - 1u) > 0);
    CHECK(window_peak_lines(window_peak_word(7, 9)) == 7 && window_peak_entry(window_peak_word(7, 9)) == 9 && window_peak_entry(window_peak_word(1, 0)) == 0);
    {
        const uint32_t lines[] = {1, 2, 4, 3, 4, 4, 1};
        uint64_t best = 0;
        for (uint32_t e = 0; e < 7; ++e) best = std::max(best, window_peak_word(lines[e], e));
        CHECK(window_peak_lines(best) == 4 && window_peak_entry(best) == 2);
    }
    // the window's sum from the columns' differences: 2 x INT64_MAX and 3 x INT64_MIN leave int64
    {
        StatsAcc a;
        a.add_number(hi);
        a.add_number(hi);
        WindowSum s = window_sum(2ull | (5ull << 32), a.lo, static_cast<uint64_t>(a.hi));
        CHECK(s.numbers == 2 && s.sum_hi == 0 && s.sum_lo == 0xFFFFFFFFFFFFFFFEull && s.reserved == 0);
        StatsAcc b;
        for (int q = 0; q < 3; ++q) b.add_number(lo);
        s = window_sum(3, b.lo, static_cast<uint64_t>(b.hi));
        CHECK(s.numbers == 3 && s.sum_hi == -2 && s.sum_lo == 0x8000000000000000ull);
        s = window_sum(0, 0, 0);
        CHECK(s.numbers == 0 && s.sum_lo == 0 && s.sum_hi == 0);
        // as a difference of two prefixes, modulo 2^64 per column
        StatsAcc p0, p1;
        p0.add_number(-7);
        p0.add_number(hi);
        p1 = p0;
        p1.add_number(lo);
        p1.add_number(-1);
        s = window_sum(4 - 2, p1.lo - p0.lo, static_cast<uint64_t>(p1.hi) - static_cast<uint64_t>(p0.hi));
        CHECK(s.numbers == 2 && s.sum_hi == -1 && s.sum_lo == 0x7FFFFFFFFFFFFFFFull);   // INT64_MIN - 1
    }
    static_assert(sizeof(WindowsDev2) == 32 && sizeof(WindowSum) == 32, "what the host copies");
    // gallop + bisect against the linear scan: a key change at e - 1, e - 2 and e - 2^k (+-1), with a window that holds everything
    for (uint32_t run = 1; run <= 300; ++run) {
        std::vector<uint64_t> key(40, 7);
        std::vector<int64_t> time(40, 0);
        for (uint32_t i = 0; i < run; ++i) { key.push_back(8); time.push_back(static_cast<int64_t>(i)); }
        if (replay(key, time, hi)) return 1;
        if (replay(key, time, 3)) return 1;
    }
    {   // the run begins at entry 0: the gallop reaches f = 0 and holds there
        std::vector<uint64_t> key(1025, 0);
        std::vector<int64_t> time(1025, 5);
        if (replay(key, time, 0)) return 1;
        for (uint32_t i = 0; i < 1025; ++i) time[i] = i < 3 ? lo : i < 1022 ? static_cast<int64_t>(i) : hi;
        if (replay(key, time, hi)) return 1;
    }
    // drawn orders, corners among the times
    uint64_t x = 88172645463325252ull;
    auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (int round = 0; round < 60; ++round) {
        const size_t m = round == 0 ? 1 : 1 + next() % 400;
        const uint64_t n_keys = 1 + next() % (round % 3 == 0 ? 3 : 60);
        std::vector<std::pair<uint64_t, int64_t>> pairs(m);
        for (size_t i = 0; i < m; ++i) {
            const uint64_t r = next();
            pairs[i] = {next() % n_keys, round % 4 == 1 ? corners[r % 11] : round % 4 == 2 ? static_cast<int64_t>(r) : static_cast<int64_t>(r % 2000) - 1000};
        }
        std::sort(pairs.begin(), pairs.end());
        std::vector<uint64_t> key(m);
        std::vector<int64_t> time(m);
        for (size_t i = 0; i < m; ++i) { key[i] = pairs[i].first; time[i] = pairs[i].second; }
        const int64_t window = round % 5 == 0 ? 0 : round % 5 == 1 ? hi : static_cast<int64_t>(next() % 300);
        if (replay(key, time, window)) return 1;
    }
    printf("windows rule ok\n");
    return 0;
}
