// The rule of gx_group_quantiles (gorp_amd/csrc/gx_group_quantile.hpp, plain C++) as a program of its own: cases on stdin, one per
// line, the answers on stdout in the same order; tests/test_group_quantile_host.py compares them with Python
// (tests/group_quantile_oracle.py).  Built with -fsanitize=address,undefined -fno-sanitize-recover=undefined: every buffer is allocated
// with exactly its entries, so a probe outside a run or a scatter past the end is a report.
//   B <n_keys>                          gq_key_bits; prints the bits
//   S <n_keys> <all> <n_q> (<num> <den>)... <m> (<key number> <value>)...
//                                       the candidates' pairs in line order.  The OR and the AND of the value keys as the compaction
//                                       leaves them, gq_plan, a host LSD sort that runs the plan's passes as the kernels do (count,
//                                       bin-major bases, stable scatter between two buffers), then gq_pick per (key, quantile).
//                                       Prints: the value digits sorted as a bit mask, the key digits sorted, the buffer that holds
//                                       the result, 1 if the result is the pairs ordered by (key number, value, input place) else
//                                       0, then per key and quantile value rank below equal.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "gx_group_quantile.hpp"

struct Pairs {
    std::unique_ptr<uint64_t[]> v;
    std::unique_ptr<uint32_t[]> k, at;   // at: the pair's place in the input, to see the sort's stability
    explicit Pairs(size_t m) : v(new uint64_t[m]), k(new uint32_t[m]), at(new uint32_t[m]) {}
};

static void pass(const Pairs& in, Pairs& out, size_t m, gx::GqPass p) {
    std::unique_ptr<uint64_t[]> base(new uint64_t[gx::GQ_BINS + 1]);
    std::fill(base.get(), base.get() + gx::GQ_BINS + 1, 0);
    auto digit = [&](size_t i) { return p.on_key ? gx::gq_digit(in.k[i], p.shift) : gx::gq_digit(in.v[i], p.shift); };
    for (size_t i = 0; i < m; ++i) ++base[digit(i) + 1];
    for (uint32_t b = 0; b < gx::GQ_BINS; ++b) base[b + 1] += base[b];
    for (size_t i = 0; i < m; ++i) {
        const uint64_t to = base[digit(i)]++;
        out.v[to] = in.v[i];
        out.k[to] = in.k[i];
        out.at[to] = in.at[i];
    }
}

static int sort_and_pick(std::istringstream& in) {
    uint64_t n_keys = 0;
    uint32_t all = 0, n_q = 0;
    in >> n_keys >> all >> n_q;
    if (n_q > gx::QUANT_MAX) return 2;
    std::vector<gx::QuantAsk> asks(n_q);
    for (auto& a : asks) in >> a.num >> a.den;
    size_t m = 0;
    in >> m;
    Pairs buf[2] = {Pairs(m), Pairs(m)};
    uint64_t o = 0, a = ~0ull;
    for (size_t i = 0; i < m; ++i) {
        int64_t v = 0;
        uint32_t k = 0;
        in >> k >> v;
        if (k >= n_keys) return 2;
        buf[0].k[i] = k;
        buf[0].v[i] = gx::top_key(v, false);
        buf[0].at[i] = static_cast<uint32_t>(i);
        o |= buf[0].v[i];
        a &= buf[0].v[i];
    }
    if (!in) return 2;
    const gx::GqPlan plan = gx::gq_plan(m ? o ^ a : 0, n_keys, all != 0);
    if (plan.n_passes > gx::GQ_MAX_PASSES) return 3;
    uint64_t value_digits = 0, key_digits = 0;
    for (uint32_t p = 0; p < plan.n_passes; ++p) {
        pass(buf[p & 1u], buf[(p & 1u) ^ 1u], m, plan.pass[p]);
        if (plan.pass[p].on_key) ++key_digits;
        else value_digits |= 1ull << (plan.pass[p].shift / gx::GQ_DIGIT_BITS);
    }
    const Pairs& s = buf[gx::gq_result_buffer(plan)];
    // ordered by (key number, value, input place), and every input pair exactly once
    bool ordered = true;
    for (size_t i = 1; i < m; ++i) {
        const bool le = s.k[i - 1] != s.k[i] ? s.k[i - 1] < s.k[i] : s.v[i - 1] != s.v[i] ? s.v[i - 1] < s.v[i] : s.at[i - 1] < s.at[i];
        ordered = ordered && le;
    }
    std::vector<char> seen(m, 0);
    for (size_t i = 0; i < m; ++i) {
        if (s.at[i] >= m || seen[s.at[i]]) ordered = false;
        else seen[s.at[i]] = 1;
    }
    printf("%" PRIu64 " %" PRIu64 " %u %d", value_digits, key_digits, gx::gq_result_buffer(plan), ordered ? 1 : 0);
    for (uint64_t j = 0; j < n_keys; ++j)
        for (const auto& ask : asks) {
            const gx::QuantOut r = gx::gq_pick(s.k.get(), s.v.get(), m, static_cast<uint32_t>(j), ask.num, ask.den);
            printf(" %" PRId64 " %" PRIu64 " %" PRIu64 " %" PRIu64, r.value, r.rank, r.below, r.equal);
        }
    printf("\n");
    return 0;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        char what = 0;
        in >> what;
        if (what == 'B') {
            uint64_t n_keys = 0;
            in >> n_keys;
            printf("%u\n", gx::gq_key_bits(n_keys));
        } else if (what == 'S') {
            const int rc = sort_and_pick(in);
            if (rc) return rc;
        } else {
            return 2;
        }
    }
    return 0;
}
