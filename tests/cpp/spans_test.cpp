// spans_test.cpp -- the rule of gx_group_spans (gorp_amd/csrc/gx_spans.hpp) as a program of its own, built by tests/test_cpp_spans.py
// with g++ alone (-fsanitize=address,undefined): the exact duration over the corners of int64, the state rule on every combination of
// neighbours, and a host replay of the passes -- the stable sort by the key number's digits, the heads, their scan -- against the loop
// the reference's caller writes, a std::map with put and remove, on random role strings.  Prints "spans rule ok".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#include "gx_bucket.hpp"
#include "gx_spans.hpp"

using namespace gx;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static bool fits(int64_t b, int64_t e, int64_t want) {
    int64_t d = 77;
    return span_duration(b, e, &d) && d == want;
}
static bool leaves(int64_t b, int64_t e) {
    int64_t d = 77;
    return !span_duration(b, e, &d) && d == 0;
}

// the stable LSD sort of (word, payload) pairs by the key number's lowest digits, as the kernels make it: a count per digit, its scan, a scatter
static uint32_t sort_by(std::vector<uint64_t> (&word)[2], std::vector<uint32_t> (&pay)[2], uint32_t n_digits) {
    uint32_t cur = 0;
    const size_t m = word[0].size();
    for (uint32_t q = 0; q < n_digits; ++q) {
        uint64_t base[GQ_BINS + 1] = {};
        for (size_t i = 0; i < m; ++i) ++base[bucket_digit(word[cur][i], q) + 1u];
        for (uint32_t b = 0; b < GQ_BINS; ++b) base[b + 1u] += base[b];
        for (size_t i = 0; i < m; ++i) {
            const uint64_t to = base[bucket_digit(word[cur][i], q)]++;
            word[cur ^ 1u].at(to) = word[cur][i];
            pay[cur ^ 1u].at(to) = pay[cur][i];
        }
        cur ^= 1u;
    }
    return cur;
}

struct Want {
    std::vector<uint32_t> state;
    std::vector<std::pair<uint32_t, uint32_t>> spans;   // (begin line, end line), in the order the ends arrive
    std::map<uint32_t, uint32_t> open;
};

static int replay(const std::vector<uint32_t>& key, const std::vector<uint32_t>& role, uint64_t n_keys, bool all_digits) {
    const size_t m = key.size();
    // the caller's loop: open.put on a begin, open.remove on an end
    Want w;
    w.state.assign(m, SPAN_S_NONE);
    for (size_t i = 0; i < m; ++i) {
        const uint32_t line = static_cast<uint32_t>(i);
        auto at = w.open.find(key[i]);
        if (role[i] == SPAN_BEGIN) {
            if (at != w.open.end()) w.state[at->second] = SPAN_S_SUPERSEDED;
            w.open[key[i]] = line;
        } else if (at == w.open.end()) {
            w.state[i] = SPAN_S_ORPHAN;
        } else {
            w.state[at->second] = SPAN_S_BEGIN;
            w.state[i] = SPAN_S_END;
            w.spans.emplace_back(at->second, line);
            w.open.erase(at);
        }
    }
    for (const auto& kv : w.open) w.state[kv.second] = SPAN_S_OPEN;
    std::stable_sort(w.spans.begin(), w.spans.end(), [&](const auto& a, const auto& b) { return key[a.second] != key[b.second] ? key[a.second] < key[b.second] : a.second < b.second; });
    // the passes: pairs in line order, the sort, the heads from the two neighbours, the scan of the span ends
    std::vector<uint64_t> kw[2];
    std::vector<uint32_t> ln[2];
    for (int q = 0; q < 2; ++q) { kw[q].assign(m, 0); ln[q].assign(m, 0); }
    for (size_t i = 0; i < m; ++i) { kw[0][i] = key[i]; ln[0][i] = static_cast<uint32_t>(i); }
    const uint32_t kd = spans_key_digits(n_keys, all_digits);
    CHECK(kd <= BY_KEY_MAX_PASSES && (!all_digits || kd == BY_KEY_MAX_PASSES));
    const uint32_t c = sort_by(kw, ln, kd);
    std::vector<uint64_t> before(m + 1, 0);
    std::vector<uint32_t> state(m);
    for (size_t e = 0; e < m; ++e) {
        CHECK(e == 0 || kw[c][e - 1] < kw[c][e] || (kw[c][e - 1] == kw[c][e] && ln[c][e - 1] < ln[c][e]));   // (key, line) order
        const bool prev = e > 0 && kw[c][e - 1] == kw[c][e], next = e + 1 < m && kw[c][e + 1] == kw[c][e];
        state[e] = span_state(role[ln[c][e]], prev, e > 0 ? role[ln[c][e - 1]] : 99u, next, e + 1 < m ? role[ln[c][e + 1]] : 99u);
        CHECK(state[e] == w.state[ln[c][e]]);
        before[e + 1] = before[e] + (state[e] == SPAN_S_END ? 1u : 0u);
    }
    CHECK(before[m] == w.spans.size());
    for (size_t e = 0; e < m; ++e) {
        if (state[e] != SPAN_S_END) continue;
        CHECK(e > 0 && state[e - 1] == SPAN_S_BEGIN && before[e] < w.spans.size());
        CHECK(w.spans[before[e]].first == ln[c][e - 1] && w.spans[before[e]].second == ln[c][e]);   // spans leave ordered by (key, end line)
    }
    for (size_t e = 0; e + 1 < m; ++e)
        if (state[e] == SPAN_S_BEGIN) CHECK(state[e + 1] == SPAN_S_END && before[e + 1] == before[e]);   // a begin's span: sbefore[e + 1]
    // a key's open line: its run's last entry, when that is a begin left open
    for (uint64_t j = 0; j < n_keys; ++j) {
        const uint64_t b = by_key_begin(kw[c].data(), m, j), e = by_key_begin(kw[c].data(), m, j + 1);
        const auto at = w.open.find(static_cast<uint32_t>(j));
        if (e > b && state[e - 1] == SPAN_S_OPEN) CHECK(at != w.open.end() && at->second == ln[c][e - 1]);
        else CHECK(at == w.open.end());
    }
    return 0;
}

int main() {
    const int64_t lo = INT64_MIN, hi = INT64_MAX;
    // the duration over the corners of int64: begin -> end
    CHECK(leaves(lo, hi));                  // 2^64 - 1
    CHECK(leaves(hi, lo));                  // -(2^64 - 1)
    CHECK(leaves(-1, hi));                  // 2^63: one more than INT64_MAX
    CHECK(fits(0, hi, hi));                 // 2^63 - 1: the largest
    CHECK(fits(0, lo, lo));                 // -2^63: the smallest
    CHECK(leaves(1, lo));                   // -2^63 - 1
    CHECK(fits(lo, -1, hi));                // 2^63 - 1 from the other end
    CHECK(leaves(lo, 0));                   // 2^63
    CHECK(fits(hi, -1, lo) && fits(hi, 0, -hi));
    CHECK(fits(5, 5, 0) && fits(lo, lo, 0) && fits(hi, hi, 0) && fits(-1, -1, 0));   // equal times give 0
    CHECK(fits(9, 2, -7) && fits(-9, -2, 7) && fits(lo, lo + 1, 1) && fits(hi, hi - 1, -1));
    const int64_t corners[] = {lo, lo + 1, -2, -1, 0, 1, 2, hi - 1, hi};
    for (const int64_t b : corners)
        for (const int64_t e : corners) {
            // the same decision from the signs alone: the difference leaves int64 only when the signs differ
            const bool mixed = (b < 0) != (e < 0);
            int64_t d = 0;
            const bool ok = span_duration(b, e, &d);
            if (!mixed) CHECK(ok && d == e - b);
            else if (e >= 0) CHECK(ok == (e <= hi + b) && (!ok || d == e - b));   // b < 0: e - b <= hi  <=>  e <= hi + b
            else CHECK(ok == (e >= lo + b) && (!ok || d == e - b));               // b >= 0: e - b >= lo  <=>  e >= lo + b
        }
    // a span's row: the classes, the zeros where a side is no number, out of range
    SpanRow r = span_row(SPAN_C_NUMBER, 100, SPAN_C_NUMBER, 40);
    CHECK(r.cls == SPAN_C_NUMBER && r.begin == 100 && r.end == 40 && r.duration == -60 && !r.out_of_range);
    r = span_row(SPAN_C_UNSET, 0, SPAN_C_NUMBER, 40);
    CHECK(r.cls == SPAN_C_UNSET && r.begin == 0 && r.end == 40 && r.duration == 0 && !r.out_of_range);
    r = span_row(SPAN_C_NUMBER, 7, SPAN_C_NAN, 0);
    CHECK(r.cls == SPAN_C_NAN && r.begin == 7 && r.end == 0 && r.duration == 0 && !r.out_of_range);
    r = span_row(SPAN_C_UNSET, 0, SPAN_C_NAN, 0);
    CHECK(r.cls == SPAN_C_NAN && !r.out_of_range);
    r = span_row(SPAN_C_NUMBER, lo, SPAN_C_NUMBER, hi);
    CHECK(r.cls == SPAN_C_NAN && r.begin == lo && r.end == hi && r.duration == 0 && r.out_of_range);
    for (uint32_t cls = 0; cls < 3; ++cls)
        for (uint32_t role = SPAN_BEGIN; role <= SPAN_END; ++role) CHECK(span_pack_class(span_pack(cls, role)) == cls && span_pack_role(span_pack(cls, role)) == role);
    // the state rule on every combination of neighbours (a neighbour of another key is no neighbour, whatever its role)
    for (uint32_t pr = 0; pr <= SPAN_END; ++pr)
        for (uint32_t nr = 0; nr <= SPAN_END; ++nr)
            for (int prev = 0; prev < 2; ++prev)
                for (int next = 0; next < 2; ++next) {
                    if ((prev && pr == 0) || (next && nr == 0)) continue;   // (a neighbour that is there has a role)
                    const uint32_t b = span_state(SPAN_BEGIN, prev, pr, next, nr), e = span_state(SPAN_END, prev, pr, next, nr);
                    CHECK(b == (!next ? SPAN_S_OPEN : nr == SPAN_END ? SPAN_S_BEGIN : SPAN_S_SUPERSEDED));
                    CHECK(e == (prev && pr == SPAN_BEGIN ? SPAN_S_END : SPAN_S_ORPHAN));
                }
    CHECK(span_state(SPAN_BEGIN, false, SPAN_BEGIN, false, SPAN_END) == SPAN_S_OPEN);     // the next entry is another key's END: no span
    CHECK(span_state(SPAN_END, false, SPAN_BEGIN, true, SPAN_END) == SPAN_S_ORPHAN);     // the entry before is another key's BEGIN: no span
    CHECK(spans_key_digits(0, false) == 0 && spans_key_digits(1, false) == 0 && spans_key_digits(2, false) == 1 && spans_key_digits(64, false) == 1 &&
          spans_key_digits(65, false) == 2 && spans_key_digits(1ull << 30, false) == 5 && spans_key_digits(1, true) == 5);
    static_assert(sizeof(SpansDev) == 64 && sizeof(SpansHead) % 16 == 0 && SPAN_BEGIN == 1u && SPAN_END == 2u, "what the host copies");
    // B B E E on one key: one span, one superseded begin, one orphan end
    if (replay({0, 0, 0, 0}, {SPAN_BEGIN, SPAN_BEGIN, SPAN_END, SPAN_END}, 1, false)) return 1;
    // key 0's last entry a BEGIN, key 1's first an END: neighbours in the sorted order, and no span
    if (replay({0, 1}, {SPAN_BEGIN, SPAN_END}, 2, false)) return 1;
    if (replay({1, 0}, {SPAN_END, SPAN_BEGIN}, 2, true)) return 1;
    // a host replay of the passes on random role strings
    uint64_t x = 88172645463325252ull;
    auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (int round = 0; round < 60; ++round) {
        const size_t m = round == 0 ? 0 : 1 + next() % 400;
        const uint64_t n_keys = 1 + next() % (round % 3 == 0 ? 3 : round % 3 == 1 ? 70 : 5000);
        const uint64_t begin_share = 1 + next() % 9;
        std::vector<uint32_t> key(m), role(m);
        for (size_t i = 0; i < m; ++i) {
            key[i] = static_cast<uint32_t>(next() % n_keys);
            role[i] = next() % 10 < begin_share ? SPAN_BEGIN : SPAN_END;
        }
        if (replay(key, role, n_keys, round % 2 == 1)) return 1;
    }
    printf("spans rule ok\n");
    return 0;
}
