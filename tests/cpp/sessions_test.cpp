// sessions_test.cpp -- the rule of gx_group_sessions (gorp_amd/csrc/gx_sessions.hpp) as a program of its own, built by
// tests/test_cpp_sessions.py with g++ alone (-fsanitize=address,undefined): the gap predicate over the corners of int64, the head rule,
// the plan helpers, and a host replay of the passes -- the two stable sorts by the plans' digits, the heads, their scan, the starts --
// against a std::stable_sort and a loop.  Prints "sessions rule ok".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gx_sessions.hpp"

using namespace gx;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static bool opens(int64_t prev, int64_t t, int64_t max_gap) { return session_opens(session_gap(prev, t), max_gap); }
static bool same_both_ways(int64_t prev, int64_t t, int64_t max_gap) {
    return session_opens(session_gap(prev, t), max_gap) == session_opens(session_gap_of(top_key(prev, false), top_key(t, false)), max_gap);
}

// the stable LSD sort of (word, payload) pairs by the given digits, as the kernels make it: a count per digit, its exclusive scan, a scatter
static uint32_t sort_by(std::vector<uint64_t> (&word)[2], std::vector<uint32_t> (&pay)[2], const uint8_t* digits, uint32_t n_digits) {
    uint32_t cur = 0;
    const size_t m = word[0].size();
    for (uint32_t q = 0; q < n_digits; ++q) {
        uint64_t base[GQ_BINS + 1] = {};
        for (size_t i = 0; i < m; ++i) ++base[bucket_digit(word[cur][i], digits[q]) + 1u];
        for (uint32_t b = 0; b < GQ_BINS; ++b) base[b + 1u] += base[b];
        for (size_t i = 0; i < m; ++i) {
            const uint64_t to = base[bucket_digit(word[cur][i], digits[q])]++;
            word[cur ^ 1u].at(to) = word[cur][i];
            pay[cur ^ 1u].at(to) = pay[cur][i];
        }
        cur ^= 1u;
    }
    return cur;
}

static int replay(const std::vector<uint32_t>& key, const std::vector<int64_t>& time, uint64_t n_keys, int64_t max_gap, bool all_digits) {
    const size_t m = key.size();
    std::vector<uint64_t> tw[2], kw[2];
    std::vector<uint32_t> tl[2], kp[2];
    for (int q = 0; q < 2; ++q) { tw[q].assign(m, 0); kw[q].assign(m, 0); tl[q].assign(m, 0); kp[q].assign(m, 0); }
    uint64_t t_or = 0, t_and = ~0ull;
    for (size_t i = 0; i < m; ++i) {
        tw[0][i] = top_key(time[i], false);
        tl[0][i] = static_cast<uint32_t>(i);
        t_or |= tw[0][i];
        t_and &= tw[0][i];
    }
    const SortPlan plan = sessions_time_plan(t_or, t_and, m, all_digits);
    CHECK(plan.n_passes <= SORT_MAX_PASSES && (!all_digits || m == 0 || plan.n_passes == SORT_MAX_PASSES));
    const uint32_t ct = sort_by(tw, tl, plan.digit, plan.n_passes);
    for (size_t p = 0; p < m; ++p) { kw[0][p] = key[tl[ct][p]]; kp[0][p] = static_cast<uint32_t>(p); }
    const uint32_t kd = sessions_key_digits(n_keys, all_digits);
    CHECK(kd <= BY_KEY_MAX_PASSES);
    uint8_t digits[BY_KEY_MAX_PASSES];
    for (uint32_t d = 0; d < kd; ++d) digits[d] = static_cast<uint8_t>(d);
    const uint32_t ck = sort_by(kw, kp, digits, kd);
    // against std::stable_sort by (key, time) over the lines in input order
    std::vector<uint32_t> want(m);
    for (size_t i = 0; i < m; ++i) want[i] = static_cast<uint32_t>(i);
    std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return key[a] != key[b] ? key[a] < key[b] : time[a] < time[b]; });
    std::vector<uint8_t> head(m);
    std::vector<uint64_t> before(m + 1, 0);
    uint64_t sessions_want = 0;
    for (size_t e = 0; e < m; ++e) {
        const uint32_t line = tl[ct].at(kp[ck].at(e));
        CHECK(line == want[e]);
        const bool h = e == 0 ? session_head(true, 0, 0, 0, 0, max_gap)
                              : session_head(false, static_cast<uint32_t>(kw[ck][e - 1]), static_cast<uint32_t>(kw[ck][e]), tw[ct].at(kp[ck][e - 1]), tw[ct].at(kp[ck][e]), max_gap);
        // the loop the caller writes, in 128-bit-free arithmetic on the sorted order: a new session at a new key or a gap above max_gap
        const bool w = e == 0 || key[want[e]] != key[want[e - 1]] ||
                       static_cast<uint64_t>(time[want[e]]) - static_cast<uint64_t>(time[want[e - 1]]) > static_cast<uint64_t>(max_gap);
        CHECK(h == w);
        head[e] = h ? 1 : 0;
        before[e + 1] = before[e] + head[e];
        sessions_want += w ? 1u : 0u;
    }
    CHECK(before[m] == sessions_want);
    for (size_t e = 0; e < m; ++e) {
        const uint64_t s = session_of(before[e], head[e] != 0);
        CHECK(s < before[m] && (e == 0 || s == session_of(before[e - 1], head[e - 1] != 0) + (head[e] ? 1u : 0u)));
    }
    return 0;
}

int main() {
    const int64_t lo = INT64_MIN, hi = INT64_MAX;
    // the corners of int64
    CHECK(opens(lo, hi, hi) && same_both_ways(lo, hi, hi));                 // 2^64 - 1 exceeds every max_gap
    CHECK(session_gap(lo, hi) == ~0ull && session_gap_of(top_key(lo, false), top_key(hi, false)) == ~0ull);
    CHECK(!opens(5, 5, 0) && !opens(lo, lo, 0) && !opens(hi, hi, 0) && !opens(-1, -1, hi));   // equal times never open a session
    CHECK(opens(5, 6, 0) && opens(-1, 0, 0) && opens(lo, lo + 1, 0));                           // max_gap 0: any step does
    CHECK(!opens(lo, -1, hi) && opens(lo, 0, hi) && !opens(0, hi, hi) && opens(-1, hi, hi));   // a difference of exactly INT64_MAX, and one more
    CHECK(!opens(-100, -70, 30) && opens(-100, -69, 30) && !opens(hi - 30, hi, 30) && opens(hi - 31, hi, 30) && !opens(lo, lo + 30, 30) && opens(lo, lo + 31, 30));
    const int64_t corners[] = {lo, lo + 1, -31, -30, -1, 0, 1, 30, 31, hi - 1, hi};
    const int64_t gaps[] = {0, 1, 30, hi - 1, hi};
    for (const int64_t a : corners)
        for (const int64_t b : corners)
            for (const int64_t g : gaps)
                if (a <= b) CHECK(same_both_ways(a, b, g));
    // the head rule
    CHECK(session_head(true, 7, 7, 0, 0, hi) && session_head(false, 1, 2, 5, 5, hi) && !session_head(false, 2, 2, 5, 5, 0) && session_head(false, 2, 2, 5, 6, 0));
    CHECK(session_of(0, true) == 0 && session_of(1, false) == 0 && session_of(1, true) == 1 && session_of(9, false) == 8);
    // the plan helpers
    CHECK(sessions_time_plan(0, ~0ull, 0, true).n_passes == 0 && sessions_time_plan(5, 5, 1, false).n_passes == 0 && sessions_time_plan(5, 5, 1, true).n_passes == 11);
    const SortPlan p = sessions_time_plan(top_key(0, false) | top_key(4096, false), top_key(0, false) & top_key(4096, false), 2, false);
    CHECK(p.n_passes == 1 && p.digit[0] == 2);
    CHECK(sessions_time_plan(top_key(lo, false) | top_key(hi, false), top_key(lo, false) & top_key(hi, false), 2, false).n_passes == 11);
    CHECK(sessions_key_digits(0, false) == 0 && sessions_key_digits(1, false) == 0 && sessions_key_digits(2, false) == 1 && sessions_key_digits(64, false) == 1 &&
          sessions_key_digits(65, false) == 2 && sessions_key_digits(4096, false) == 2 && sessions_key_digits(4097, false) == 3 &&
          sessions_key_digits(1ull << 30, false) == 5 && sessions_key_digits(1, true) == 5);
    static_assert(sizeof(SessionsDev) == 64 && sizeof(SessionsDev2) == 32 && sizeof(SessionsHead) % 16 == 0, "what the host copies");
    // a host replay of the passes on drawn entries, corners among them
    uint64_t x = 88172645463325252ull;
    auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (int round = 0; round < 40; ++round) {
        const size_t m = round == 0 ? 0 : 1 + next() % 300;
        const uint64_t n_keys = 1 + next() % (round % 3 == 0 ? 3 : 200);
        std::vector<uint32_t> key(m);
        std::vector<int64_t> time(m);
        for (size_t i = 0; i < m; ++i) {
            key[i] = static_cast<uint32_t>(next() % n_keys);
            const uint64_t r = next();
            time[i] = round % 4 == 1 ? corners[r % 11] : round % 4 == 2 ? static_cast<int64_t>(r) : static_cast<int64_t>(r % 2000) - 1000;
        }
        const int64_t gap = round % 5 == 0 ? 0 : round % 5 == 1 ? hi : static_cast<int64_t>(next() % 64);
        if (replay(key, time, n_keys, gap, round % 2 == 1)) return 1;
    }
    printf("sessions rule ok\n");
    return 0;
}
