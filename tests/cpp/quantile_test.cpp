// The rule of gx_capture_quantiles (gorp_amd/csrc/gx_quantile.hpp, plain C++) as a program of its own: cases on stdin, one per line,
// the answers on stdout in the same order; tests/test_quantile_host.py compares them with Python (tests/quantile_oracle.py).  Built with
// -fsanitize=address,undefined -fno-sanitize-recover=undefined: the histograms are allocated with exactly their bins, so a probe
// outside them is a report.
//   R <num> <den> <numbers>             quant_rank; prints the rank
//   P <remaining> <pairs> (<bin> <count>)...
//                                       the suffix pick -- every bin asks quant_picked for itself -- on a histogram that is zero but for
//                                       the pairs; prints bin above remaining, and ends the program with status 3 when not exactly one
//                                       bin is picked or the pick is not top_pick's
//   Q <n_q> (<num> <den>)... <count> <v>...
//                                       the whole select on the host as the kernels run it: quant_begin, and per digit quant_groups, a
//                                       histogram per group, the suffix pick and quant_step; prints per quantile value rank below equal,
//                                       then the number of groups before each of the eight digits, most significant first
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "gx_quantile.hpp"

// hist[0, 256): the bin every lane of k_quant_pick would find for itself
static bool suffix_pick(const uint32_t* hist, uint32_t remaining, gx::TopPick* out) {
    std::unique_ptr<uint64_t[]> S(new uint64_t[gx::TOP_BINS + 1]);
    S[gx::TOP_BINS] = 0;
    for (uint32_t b = gx::TOP_BINS; b-- > 0u;) S[b] = S[b + 1] + hist[b];
    uint32_t picked = 0;
    for (uint32_t b = 0; b < gx::TOP_BINS; ++b)
        if (gx::quant_picked(S[b], S[b + 1], remaining)) {
            *out = gx::quant_pick_of(b, S[b + 1], remaining);
            ++picked;
        }
    return picked == 1;
}

static int select(std::istringstream& in) {
    uint32_t n_q = 0;
    in >> n_q;
    if (n_q > gx::QUANT_MAX) return 2;
    std::vector<gx::QuantAsk> asks(n_q);
    for (auto& a : asks) in >> a.num >> a.den;
    size_t count = 0;
    in >> count;
    std::vector<uint64_t> keys(count);
    for (size_t i = 0; i < count; ++i) {
        int64_t v = 0;
        in >> v;
        keys[i] = gx::top_key(v, false);
    }
    std::unique_ptr<gx::QuantSelect[]> sel(new gx::QuantSelect[n_q]);   // exactly n_q states
    for (uint32_t q = 0; q < n_q; ++q) gx::quant_begin(sel[q], asks[q].num, asks[q].den, count);
    uint32_t groups_at[gx::TOP_DIGITS] = {};
    for (uint32_t d = gx::TOP_DIGITS; d-- > 0u;) {
        gx::QuantGroups g{};
        gx::quant_groups(sel.get(), n_q, d, g);
        groups_at[d] = g.n_groups;
        std::unique_ptr<uint32_t[]> hist(new uint32_t[static_cast<size_t>(g.n_groups) * gx::TOP_BINS]());
        for (uint64_t k : keys) {
            uint32_t at = g.n_groups, under = 0;
            for (uint32_t j = 0; j < g.n_groups; ++j)
                if (gx::top_in_prefix(k, sel[g.head[j]].prefix, d)) { at = j; ++under; }
            if (under > 1) return 3;   // the groups' prefixes differ above d
            if (at < g.n_groups) ++hist[at * gx::TOP_BINS + gx::top_digit(k, d)];
        }
        for (uint32_t q = 0; q < n_q; ++q) {
            if (sel[q].rank == 0u) continue;
            const uint32_t* h = hist.get() + static_cast<size_t>(g.group_of[q]) * gx::TOP_BINS;
            gx::TopPick p{};
            if (!suffix_pick(h, sel[q].remaining, &p)) return 3;
            gx::quant_step(sel[q], p, h[p.bin], d);
        }
    }
    for (uint32_t q = 0; q < n_q; ++q) {
        const gx::QuantOut o = gx::quant_out(sel[q], count);
        printf("%" PRId64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " ", o.value, o.rank, o.below, o.equal);
    }
    for (uint32_t d = gx::TOP_DIGITS; d-- > 0u;) printf("%u%s", groups_at[d], d ? " " : "");
    printf("\n");
    return 0;
}

int main() {
    std::string row;
    while (std::getline(std::cin, row)) {
        if (row.empty()) continue;
        std::istringstream in(row);
        std::string kind;
        in >> kind;
        if (kind == "R") {
            uint32_t num = 0, den = 1;
            uint64_t numbers = 0;
            in >> num >> den >> numbers;
            printf("%" PRIu64 "\n", gx::quant_rank(num, den, numbers));
        } else if (kind == "P") {
            uint32_t remaining = 0, pairs = 0;
            in >> remaining >> pairs;
            std::unique_ptr<uint32_t[]> hist(new uint32_t[gx::TOP_BINS]());
            for (uint32_t p = 0; p < pairs; ++p) {
                uint32_t bin = 0, c = 0;
                in >> bin >> c;
                if (bin >= gx::TOP_BINS) return 2;
                hist[bin] = c;
            }
            gx::TopPick p{};
            if (!suffix_pick(hist.get(), remaining, &p)) return 3;
            const gx::TopPick t = gx::top_pick(hist.get(), remaining);
            if (t.bin != p.bin || t.above != p.above || t.remaining != p.remaining) return 3;
            printf("%u %u %u\n", p.bin, p.above, p.remaining);
        } else if (kind == "Q") {
            const int rc = select(in);
            if (rc) return rc;
        } else {
            fprintf(stderr, "unknown case: %s\n", row.c_str());
            return 2;
        }
    }
    return 0;
}
