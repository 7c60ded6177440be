// gx_images.cpp -- the batch kernels' table images (GxLds tiers 0-4), their layouts per launch, and the kernel a batch gets.
// Host arithmetic only (no HIP): gx_api.cpp uploads what choose_tile_images builds and launches what plan_batch chooses.
#include "gx_images.hpp"

#include <array>
#include <cstdio>
#include <cstdlib>
#include <map>

namespace gx {

namespace {

// Longest run of ASCII byte values on which `loops(b)` holds, as lo | (0x7F - hi) << 8 (0x8000 = none): the
// form the kernel's SWAR range test consumes.  Of equally long runs the later one wins: for \w that is a-z rather
// than A-Z, and log text is mostly lower case.
template <typename F> uint16_t self_loop_interval(F loops) {
    int best_lo = 0, best_len = 0, run_lo = 0, run = 0;
    for (int b = 0; b < 128; ++b) {
        if (loops(b)) { if (run == 0) run_lo = b; ++run; if (run >= best_len) { best_len = run; best_lo = run_lo; } }
        else run = 0;
    }
    if (best_len < 4) return 0x8000;
    return static_cast<uint16_t>(best_lo | ((0x7F - (best_lo + best_len - 1)) << 8));
}

// ---- record tier ------------------------------------------------------------------------------------------
// A state's dense row, as a handful of class ranges.  Classes are renumbered first so that the sets the rows use
// (the classes of one successor: "digits", "\w", "not a blank", single literals) become contiguous id ranges
// wherever one ordering can serve them all (greedy partition refinement, heaviest sets first); a set that stays
// split simply takes several ranges.  A state is then
//     [header: 8 bytes, only when its info word is not -1]
//     record 0:  self range (plain self-loop, no program) + one exit range with its successor and program
//     record 1:  one more exit range (record 0 says that it exists)
// or, with three ranges and more besides the self range (the branching nodes of a trie of literals), one record per
// class, behind all the others: the walk reads record [state + class].  Every class in no range leads to the dead
// state, which is record 0 of the image for all its automata (a dead state has no successors and accepts nothing, so
// they are all alike).  A record is two dwords:
//     w0 = self_lo | self_span << 8 | exit_lo << 16 | exit_span << 24      (class c is inside iff c - lo <= span, unsigned;
//                                                                           lo = 255, span = 0: empty)
//     w1 = successor (record index, 16 bits) | program << 16 (8 bits) | flags << 24 (0x80: a second record follows,
//          2: a header precedes)
// A state's index is the index of its record 0; the self-loop byte interval (GxLds rows' ACC word) is looked up by the
// self range's first class in a small table.  The class map has 32-bit entries, class | class * 8 << 16 (the walk's
// range tests take the low byte, its address arithmetic the upper half).  The builder checks its own output against
// the dense rows, class by class, before it is used.
constexpr uint32_t REC_MORE = 0x80u << 24, REC_HDR = 2u << 24, REC_IDC = 254u, REC_EMPTY = 255u, REC_AT = 1088u;

bool records_from_dense(const Tables& T, const std::vector<uint32_t>& at, size_t rows, uint32_t cols, const std::vector<uint32_t>& dead_of_row,
                        const std::vector<std::array<uint64_t, 2>>& loop_set, bool simple, Image& img, GxLds& L, std::vector<uint32_t>& c_rule,
                        std::vector<uint32_t>* items_global, uint32_t* n_records) {
    const int ncls = T.ncls;
    const uint32_t ACC = ncls + 1, INFO = ncls + 2;
    auto has = [](const ClassSet& s, int c) { return (s[c >> 6] >> (c & 63)) & 1ull; };
    // the groups of every row: successor entry -> classes (the dead default is not a group)
    struct Group { uint32_t entry; ClassSet set; };
    std::vector<std::vector<Group>> groups(rows);
    std::map<ClassSet, uint64_t> weight;
    for (size_t r = 0; r < rows; ++r) {
        std::map<uint32_t, ClassSet> by_entry;
        for (int c = 0; c < ncls; ++c) {
            const uint32_t e = at[r * cols + c];
            if (e == dead_of_row[r]) continue;
            by_entry[e][c >> 6] |= 1ull << (c & 63);
        }
        for (auto& g : by_entry) {
            // the plain self-loop first: it takes item 0's self slot
            if (g.first == static_cast<uint32_t>(r)) groups[r].insert(groups[r].begin(), Group{g.first, g.second});
            else groups[r].push_back(Group{g.first, g.second});
            ++weight[g.second];
        }
    }
    // class order: as many of the sets as possible become id ranges (gx_hop.cpp: order_classes)
    const std::vector<int> new_id = order_classes(weight, ncls);
    // ranges (in new ids) of a class set
    auto ranges_of = [&](const ClassSet& S) {
        std::vector<char> in(ncls, 0);
        for (int c = 0; c < ncls; ++c) if (has(S, c)) in[new_id[c]] = 1;
        std::vector<std::pair<int, int>> out;
        for (int i = 0; i < ncls; ++i) if (in[i]) { int j = i; while (j + 1 < ncls && in[j + 1]) ++j; out.push_back({i, j}); i = j; }
        return out;
    };
    // pass 1: items per row -> indexes
    struct Slot { int lo, hi; uint32_t entry; };
    std::vector<std::vector<Slot>> exits(rows);   // everything but the first range of the plain self-loop
    std::vector<std::pair<int, int>> self0(rows, {-1, -1});
    std::vector<uint32_t> index_of(rows);
    size_t n_items = 0;
    L.rec_indexed = 0xFFFFFFFFu;  // (first index of the class-indexed states; none)
    // which exit shares item 0 with the self range decides how often a lane needs a second record: the one that
    // printable text takes most likely first (a field's blank before some control character's odd successor)
    std::vector<int> printable(ncls, 0), bytes_of(ncls, 0);
    for (int b = 0; b < 256; ++b) { ++bytes_of[T.cls256[b]]; if (b >= 0x20 && b < 0x7F) ++printable[T.cls256[b]]; }
    auto likelihood = [&](const ClassSet& S) {
        long p = 0, n = 0;
        for (int c = 0; c < ncls; ++c) if (has(S, c)) { p += printable[c]; n += bytes_of[c]; }
        return p * 1000 + n;
    };
    for (size_t r = 0; r < rows; ++r) {
        std::stable_sort(groups[r].begin(), groups[r].end(), [&](const Group& a, const Group& b) {
            const bool sa = a.entry == static_cast<uint32_t>(r), sb = b.entry == static_cast<uint32_t>(r);
            if (sa != sb) return sa;  // the plain self-loop stays first
            return likelihood(a.set) > likelihood(b.set);
        });
        for (auto& g : groups[r]) {
            auto rs = ranges_of(g.set);
            size_t from = 0;
            if (g.entry == static_cast<uint32_t>(r) && self0[r].first < 0) { self0[r] = rs[0]; from = 1; }
            for (size_t q = from; q < rs.size(); ++q) exits[r].push_back(Slot{rs[q].first, rs[q].second, g.entry});
        }
    }
    // States with three or more records (the branching nodes of a trie of literals, the start state) are laid out
    // INDEXED BY CLASS instead: one record per class, behind all the others, so that the walk finds the class's
    // successor with its first read (state index + class; a state's index says which layout it has).
    std::vector<char> indexed(rows, 0);
    // the dead states: every class leads back to the state itself (no group above), nothing accepted; they share record 0
    auto pure_dead = [&](size_t r) { return dead_of_row[r] == r && groups[r].empty() && at[r * cols + INFO] == 0xFFFFFFFFu; };
    for (size_t r = 0; r < rows; ++r)
        if (dead_of_row[r] >= rows || !pure_dead(dead_of_row[r])) return false;  // (every automaton the compiler emits has one)
    n_items = 1;
    for (int pass = 0; pass < 2; ++pass)
        for (size_t r = 0; r < rows; ++r) {
            if (pure_dead(r)) { index_of[r] = 0; continue; }
            const bool ix = exits[r].size() >= 3;
            indexed[r] = ix;
            if (ix != (pass == 1)) continue;
            const bool hdr = at[r * cols + INFO] != 0xFFFFFFFFu;
            if (pass == 1 && L.rec_indexed == 0xFFFFFFFFu) L.rec_indexed = static_cast<uint32_t>(n_items);
            if (hdr) ++n_items;
            index_of[r] = static_cast<uint32_t>(n_items);
            n_items += ix ? static_cast<size_t>(ncls) : std::max<size_t>(1, exits[r].size());
        }
    const bool wide = items_global != nullptr;  // records in global memory: 22-bit successors
    if (n_items > (wide ? 0x3FFFFFu : 65535u)) return false;
    *n_records = static_cast<uint32_t>(n_items);
    auto pack_w1 = [&](uint32_t target, uint32_t op, bool more, bool hdr) {
        return wide ? (target | op << 22 | (hdr ? 1u << 30 : 0u) | (more ? 1u << 31 : 0u)) : (target | op << 16 | (hdr ? REC_HDR : 0u) | (more ? REC_MORE : 0u));
    };
#ifdef GX_DEV
    if (getenv("GX_REC_STATS")) {
        size_t multi = 0, self_split = 0, self_states = 0;
        std::map<size_t, size_t> hist;
        for (size_t r = 0; r < rows; ++r) {
            ++hist[std::max<size_t>(1, exits[r].size())];
            if (exits[r].size() > 1) ++multi;
            if (self0[r].first >= 0) { ++self_states; for (auto& e : exits[r]) if (e.entry == static_cast<uint32_t>(r)) { ++self_split; break; } }
        }
        fprintf(stderr, "records: rows %zu items %zu multi-item states %zu self-loop states %zu of which split %zu\n", rows, n_items, multi, self_states, self_split);
        for (auto& hh : hist) fprintf(stderr, "  %zu items: %zu states\n", hh.first, hh.second);
    }
#endif
    // pass 2: emit
    std::vector<uint32_t> items(2 * n_items + 2, 0);  // (+ one: the second-record pass reads record [state + 1] of every state)
    items[0] = REC_EMPTY | (REC_EMPTY << 16);  // record 0: the dead state
    for (size_t r = 0; r < rows; ++r) {
        if (pure_dead(r)) continue;
        const uint32_t info = at[r * cols + INFO];
        const bool hdr = info != 0xFFFFFFFFu;
        if (hdr) { items[2 * (index_of[r] - 1)] = 0; items[2 * (index_of[r] - 1) + 1] = info; }
        auto op_field = [&](uint32_t entry, uint32_t& op) {  // the program as the records carry it
            op = entry >> 16;
            if (simple) op /= 128u;       // register + 1
            else if (op & 0x8000u) { if ((op & 0x7FFFu) > 127u) return false; op = 0x80u | (op & 0x7Fu); }
            else if (op > 127u) return false;
            return op <= 255u;
        };
        if (indexed[r]) {
            for (int c = 0; c < ncls; ++c) {  // record new_id[c]: class c's successor as a one-class exit (none: dead)
                const uint32_t id = static_cast<uint32_t>(new_id[c]), e = at[r * cols + c];
                uint32_t w0 = REC_EMPTY | (REC_EMPTY << 16), target = 0, op = 0;
                if (e != dead_of_row[r]) {
                    if (!op_field(e, op)) return false;
                    w0 = REC_EMPTY | (id << 16);
                    target = index_of[e & 0xFFFFu];
                }
                const uint32_t w1 = pack_w1(target, op, false, id == 0 && hdr);
                items[2 * (index_of[r] + id)] = w0;
                items[2 * (index_of[r] + id) + 1] = w1;
            }
            continue;
        }
        const size_t n = std::max<size_t>(1, exits[r].size());
        for (size_t q = 0; q < n; ++q) {
            uint32_t w0 = REC_EMPTY | (REC_EMPTY << 16), target = 0, op = 0;
            if (q == 0 && self0[r].first >= 0) w0 = (w0 & 0xFFFF0000u) | self0[r].first | (static_cast<uint32_t>(self0[r].second - self0[r].first) << 8);
            if (q < exits[r].size()) {
                const Slot& e = exits[r][q];
                w0 = (w0 & 0xFFFFu) | (static_cast<uint32_t>(e.lo) << 16) | (static_cast<uint32_t>(e.hi - e.lo) << 24);
                if (!op_field(e.entry, op)) return false;
                target = index_of[e.entry & 0xFFFFu];
            }
            const uint32_t w1 = pack_w1(target, op, q + 1 < n, q == 0 && hdr);
            items[2 * (index_of[r] + q)] = w0;
            items[2 * (index_of[r] + q) + 1] = w1;
        }
    }
    // self-loop interval words by the first class of the self range; states that share it must agree (else the
    // narrowest claim that is true for all of them: none)
    std::vector<uint32_t> acc_tab(ncls + 1, 0x8000u);
    {
        std::vector<std::vector<size_t>> by_lo(ncls);
        for (size_t r = 0; r < rows; ++r) if (self0[r].first >= 0) by_lo[self0[r].first].push_back(r);
        auto covers = [&](size_t r, int lo, int hi) {
            for (int b = lo; b <= hi; ++b) if (!(loop_set[r][b >> 6] >> (b & 63) & 1ull)) return false;
            return true;
        };
        for (int lo_c = 0; lo_c < ncls; ++lo_c) {
            uint32_t best = 0x8000u;
            int best_w = 0;
            for (size_t r : by_lo[lo_c]) {
                const uint32_t a = at[r * cols + ACC];
                if ((a & 0xFFFFu) == 0x8000u) continue;
                const int lo = static_cast<int>(a & 0xFFu), hi = 0x7F - static_cast<int>((a >> 8) & 0xFFu);
                bool all = true, hot = true;
                for (size_t q : by_lo[lo_c]) { all = all && covers(q, lo, hi); hot = hot && (at[q * cols + ACC] & 0x10000u); }
                if (all && hi - lo + 1 > best_w) { best_w = hi - lo + 1; best = (a & 0xFFFFu) | (hot ? 0x10000u : 0u); }
            }
            acc_tab[lo_c] = best;
        }
    }
    // check: every (row, class) decodes to the dense entry
    for (size_t r = 0; r < rows; ++r)
        for (int c = 0; c < ncls; ++c) {
            const uint32_t id = static_cast<uint32_t>(new_id[c]);
            uint32_t next = 0, op = 0;
            for (uint32_t q = index_of[r] + (index_of[r] >= L.rec_indexed ? id : 0u);; ++q) {
                const uint32_t w0 = items[2 * q], w1 = items[2 * q + 1];
                if (id - ((w0 >> 16) & 0xFFu) <= (w0 >> 24)) { next = wide ? (w1 & 0x3FFFFFu) : (w1 & 0xFFFFu); op = wide ? ((w1 >> 22) & 0xFFu) : ((w1 >> 16) & 0xFFu); break; }
                if (id - (w0 & 0xFFu) <= ((w0 >> 8) & 0xFFu)) { next = index_of[r]; break; }
                if (!(w1 & (wide ? 1u << 31 : REC_MORE))) break;
            }
            const uint32_t e = at[r * cols + c];
            uint32_t want_op = e >> 16;
            if (simple) want_op /= 128u; else if (want_op & 0x8000u) want_op = 0x80u | (want_op & 0x7Fu);
            if (next != index_of[e & 0xFFFFu] || op != want_op) throw GxError(GX_E_ARG, "internal: record tier does not reproduce the dense rows");
        }
    // image: class map (new ids; entry 256 = the identity class of masked bytes), interval table, items
    std::vector<uint32_t> cmap(REC_AT / 4, REC_IDC);
    for (int b = 0; b < 256; ++b) { const uint32_t id = static_cast<uint32_t>(new_id[T.cls256[b]]); cmap[b] = id | (id * 8u) << 16; }
    L.cmap = static_cast<uint32_t>(img.put(cmap));
    if (items_global) { L.rec = 0; items_global->swap(items); }  // records in global memory (tier 3)
    else { L.rec = static_cast<uint32_t>(img.put(items)); if (L.rec != REC_AT) throw GxError(GX_E_ARG, "internal: record image layout"); }
    L.acc_tab = static_cast<uint32_t>(img.put(acc_tab));
    L.at = 0;
    if (L.m_dead < rows) { L.m_start = index_of[L.m_start]; L.m_dead = index_of[L.m_dead]; }  // (absent from a capture-only image)
    if (L.u_start != 0xFFFFFFFFu) { L.u_start = index_of[L.u_start]; L.u_dead = index_of[L.u_dead]; }
    else for (size_t k = 0; k + 1 < c_rule.size(); k += 2) {
        c_rule[k] = index_of[c_rule[k]];  // per-extraction capture automata: the start states
    }
    return true;
}

// Build the table image of the tile kernel (layout: GxLds).
// tier 0: LDS tier, everything in one LDS-resident image, dense rows addressed by byte offset.
// tier 1: L2 tier, the dense rows go to a separate global-memory image (I.l2: match rows at 0, capture rows
//         at GxLds::c_base) and are addressed by state index; LDS keeps only the byte->class map, the per-extraction
//         start rows and the capture programs.
// tier 2: record tier, for automata whose dense rows do not fit LDS but whose states are sparse (a literal chain
//         link has one live class, a field state one self range and one exit): every state becomes a few 8-byte
//         range records in LDS (records_from_dense below; ~8.5 bytes per state instead of 4 * classes).
// tier 3: the same records in global memory (I.l2), where 64-512 KB of them live in the vector L1 / L2 caches.
// part 0: match automaton + capture automata in one image; 1: capture side alone (fused automaton); 2: match alone.
bool build_tile_image(TileImages& I, const Tables& T, uint32_t flags, int tier, int part = 0) {
    const bool global = tier == 1;
    const bool in_global = tier == 1 || tier == 3;  // automaton tables and final records in I.l2
    if (part != 2 && tier == 3) I.l2.clear();
    if (part != 2) {
        I.tile_ok = false;
        I.tile_global = in_global;
        I.has_mo = false;
    }
    if (T.n_rules > 32767) return false;
    const uint32_t cols = static_cast<uint32_t>(T.ncls) + 3u;
    const uint32_t RS = cols * 4u;
    // with the fused automaton present the per-extraction capture rows are not needed on the device
    // (GX_CREATE_NO_FUSED forces the two-pass layout, which otherwise only very large definitions get)
    const bool fused = T.union_ok && !(flags & GX_CREATE_NO_FUSED);
    if (part == 1 && !(fused && T.has_capture)) return false;  // the two-pass layout needs both sides
    const size_t m_rows = part == 1 ? 0 : static_cast<size_t>(T.m_states);
    size_t c_rows = 0;
    if (part == 2) c_rows = 0;
    else if (fused) c_rows = T.uni.n_states;
    else for (auto& r : T.rules) c_rows += r.n_states;
    const size_t rows = m_rows + c_rows;
    if (T.ncls > 252) return false;  // keeps the column offsets of a row (class * 4, + 3 extra columns) below 1024
    const uint32_t AT = 544;         // LDS tier: the rows follow the class map (u16[256] + the identity entry, padded)
    if (tier >= 2) {
        // a dense entry carries its successor's row in 16 bits; records in LDS have 16-bit successors too (in global memory: 22)
        if (rows > (tier == 3 ? 65536u : 65000u) || T.ncls > 250) return false;  // class ids 254 / 255 are reserved
    } else if (!global) {
        if (AT + rows * RS > 65536u) return false;  // successors are 16-bit LDS addresses
        if (rows * RS + T.ops_off.size() * 4 + T.ops.size() * 2 + 1024 > LDS_TABLE_BUDGET) return false;  // (+ the final records, below)
    } else {
        if (m_rows > 65536u || c_rows > 65536u) return false;  // state indexes are 16-bit per automaton table
        if (T.n_rules * 8 + T.ops_off.size() * 4 + T.ops.size() * 2 + 1024 > LDS_TABLE_BUDGET) return false;
    }
    // a state's successor field: LDS tier = LDS address of the row, L2 tier = state index
    const uint32_t UNIT = tier ? 1u : RS;
    const uint32_t ORG = tier ? 0u : AT;
    std::vector<uint32_t> dead_of_row(rows, 0);  // tier 2: the row every unlisted class of a row leads to

    Image img;
    GxLds L{};
    std::vector<uint16_t> cmap(272, static_cast<uint16_t>(T.ncls * 4));  // entry 256: the identity column, for bytes outside the line
    for (int b = 0; b < 256; ++b) cmap[b] = static_cast<uint16_t>(T.cls256[b] * 4);  // byte offset of the class's column
    L.cmap = static_cast<uint32_t>(img.put(cmap));  // offset 0
    L.ncls = static_cast<uint32_t>(T.ncls);
    L.row_bytes = RS;
    std::vector<uint32_t> at(rows * cols, 0);
    const uint32_t IDC = T.ncls, ACC = T.ncls + 1, INFO = T.ncls + 2;
    // per row: the ASCII bytes the state loops on (with no capture program), for the choice of the hot interval
    std::vector<std::array<uint64_t, 2>> loop_set(rows, std::array<uint64_t, 2>{0, 0});
    auto loop_interval = [&](size_t row_index, auto loops) {
        for (int b = 0; b < 128; ++b) if (loops(b)) loop_set[row_index][b >> 6] |= 1ull << (b & 63);
        return self_loop_interval(loops);
    };
    // match automaton rows
    for (int s = 0; s < static_cast<int>(m_rows); ++s) {
        uint32_t* row = &at[static_cast<size_t>(s) * cols];
        for (int c = 0; c < T.ncls; ++c) row[c] = ORG + T.m_next[static_cast<size_t>(s) * T.ncls + c] * UNIT;
        row[IDC] = ORG + static_cast<uint32_t>(s) * UNIT;
        row[ACC] = loop_interval(static_cast<size_t>(s), [&](int b) { return T.m_next[static_cast<size_t>(s) * T.ncls + T.cls256[b]] == static_cast<uint32_t>(s); });
        row[INFO] = static_cast<uint32_t>(T.m_accept_first[s]);
        dead_of_row[s] = static_cast<uint32_t>(T.m_dead);
    }
    L.m_start = ORG;
    L.m_dead = ORG + static_cast<uint32_t>(T.m_dead) * UNIT;
    L.c_base = global ? static_cast<uint32_t>(m_rows * RS) : 0u;
    // capture automata rows: the fused automaton, or one automaton per extraction
    std::vector<uint32_t> c_rule;
    size_t base_row = m_rows;
    bool too_many_programs = false;
    // are all capture programs of the tables we ship "one register := position"?
    auto is_single_set = [&](uint32_t op) {
        const uint32_t b = T.ops_off[op], e = T.ops_off[op + 1];
        return e - b == 1 && T.ops[2 * b + 1] == GX_SRC_POS && T.ops[2 * b] < 500;
    };
    bool simple = true;
    auto scan_simple = [&](const RuleTables& r) {
        for (uint32_t w : r.trans) if ((w >> 16) && !is_single_set(w >> 16)) simple = false;
    };
    if (part == 2) simple = true;
    else if (fused) scan_simple(T.uni);
    else for (auto& r : T.rules) scan_simple(r);
    L.simple_ops = simple ? 1u : 0u;
    // Final records, one per distinct (final tag list, extraction): u16 [begin tag, end tag] x max_groups padded to a
    // multiple of four groups (16 bytes), then the extraction and padding to the next 16 bytes; the tags as
    // line_result (gx_rows.hpp) wants them: 0 = unset, 1 = the line length, else the byte offset of the register's
    // column from the dummy column.  Record 0 = "no groups" for the lines that match nothing.  A row's info word is
    // the byte offset of its record.
    const size_t tag_slots = 8 * static_cast<size_t>((T.max_groups + 3) / 4), rec_len = tag_slots + 8;
    std::vector<uint16_t> fin_rec(rec_len, 0);
    fin_rec[tag_slots] = 0xFFFFu;
    std::map<std::pair<int32_t, int32_t>, uint32_t> rec_of;
    auto fin_record = [&](int32_t f, int32_t k_or_minus1) -> uint32_t {  // k < 0: the list starts with the extraction
        auto it = rec_of.find({f, k_or_minus1});
        if (it != rec_of.end()) return it->second;
        const int32_t k = k_or_minus1 >= 0 ? k_or_minus1 : static_cast<int32_t>(T.fin_tags[f]);
        const size_t t0 = k_or_minus1 >= 0 ? f : f + 1;
        const size_t at = fin_rec.size();
        fin_rec.resize(at + rec_len, 0);
        for (int g = 0; g < T.rules[k].n_groups; ++g)
            for (int e = 0; e < 2; ++e) {
                const uint16_t v = T.fin_tags[t0 + 2 * g + e];
                fin_rec[at + 2 * g + e] = v == GX_SRC_NIL ? 0 : v == GX_SRC_POS ? 1 : static_cast<uint16_t>((v + 1u) * 128u);
            }
        fin_rec[at + tag_slots] = static_cast<uint16_t>(k);
        rec_of[{f, k_or_minus1}] = static_cast<uint32_t>(at * 2);
        return static_cast<uint32_t>(at * 2);
    };
    int rule_being_emitted = -1;  // per-extraction capture automata: the rule; fused automaton: -1
    auto emit_rows = [&](const RuleTables& r) {
        // LDS tier: LDS addresses; L2 tier: state indexes within the capture rows; record tier: indexes over all rows
        const uint32_t base = ORG + static_cast<uint32_t>(global ? base_row - m_rows : base_row) * UNIT;
        for (int s = 0; s < r.n_states; ++s) {
            uint32_t* row = &at[(base_row + s) * cols];
            dead_of_row[base_row + s] = base + static_cast<uint32_t>(r.dead);
            for (int c = 0; c < T.ncls; ++c) {
                const uint32_t w = r.trans[static_cast<size_t>(s) * T.ncls + c];
                uint32_t op = w >> 16;
                if (simple) {
                    // byte offset of the register's column in the wave's register block: 0 = the dummy column
                    // ("no program"), (r + 1) * 128 = register r
                    op = op ? (T.ops[2 * T.ops_off[op]] + 1u) * 128u : 0u;
                } else if (op) {
                    // the common capture program "one register := position" is folded into the entry as 0x8000 | register
                    if (is_single_set(op)) op = 0x8000u | T.ops[2 * T.ops_off[op]];
                    else if (op >= 0x8000u) too_many_programs = true;
                }
                row[c] = (base + (w & 0xFFFFu) * UNIT) | (op << 16);
            }
            row[IDC] = base + static_cast<uint32_t>(s) * UNIT;
            row[ACC] = loop_interval(base_row + s,
                [&](int b) { return r.trans[static_cast<size_t>(s) * T.ncls + T.cls256[b]] == static_cast<uint32_t>(s); });
            row[INFO] = r.fin[s] >= 0 ? fin_record(r.fin[s], rule_being_emitted) : static_cast<uint32_t>(r.fin[s]);
        }
        base_row += r.n_states;
        return base;
    };
    L.u_start = 0xFFFFFFFFu;
    L.u_dead = 0xFFFFFFFFu;
    if (part == 2) {
        // match automaton alone
    } else if (fused) {
        const uint32_t base = emit_rows(T.uni);
        L.u_start = base;
        L.u_dead = base + static_cast<uint32_t>(T.uni.dead) * UNIT;
        for (auto& r : T.rules) { c_rule.push_back(0); c_rule.push_back(static_cast<uint32_t>(r.n_groups)); }
    } else {
        for (auto& r : T.rules) {
            rule_being_emitted = static_cast<int>(&r - &T.rules[0]);
            const uint32_t base = emit_rows(r);
            c_rule.push_back(base);
            c_rule.push_back(static_cast<uint32_t>(r.n_groups));
        }
    }
    if (too_many_programs) return false;  // too many distinct general programs for the 15-bit program field
    if (fin_rec.size() * 2 > 0xFFFFFFu) return false;
    if (tier == 0 && rows * RS + T.ops_off.size() * 4 + T.ops.size() * 2 + fin_rec.size() * 2 + 1024 > LDS_TABLE_BUDGET) return false;
    // Hot interval: among the self-loop intervals of all rows, the one that promises the longest skips -- width
    // squared (only runs of several 16-byte chunks pay off) times the number of states that loop on all of it.
    // Those states get bit 16 of their interval column; the tile kernel marks the staged chunks that lie inside the
    // interval and lets such a state jump over runs of them (gx_tile.hip).
    {
        auto covers = [&](size_t r, int lo, int hi) {
            for (int b = lo; b <= hi; ++b) if (!(loop_set[r][b >> 6] >> (b & 63) & 1ull)) return false;
            return true;
        };
        std::map<uint32_t, int> candidates;
        for (size_t r = 0; r < rows; ++r) if (at[r * cols + ACC] != 0x8000u) candidates[at[r * cols + ACC]] = 0;
        double best = 0;
        int best_lo = 0, best_hi = -1;
        for (auto& c : candidates) {
            const int lo = static_cast<int>(c.first & 0xFFu), hi = 0x7F - static_cast<int>((c.first >> 8) & 0xFFu);
            if (hi - lo + 1 < 16) continue;  // a run of such bytes seldom fills whole chunks
            int states = 0;
            for (size_t r = 0; r < rows; ++r) if (covers(r, lo, hi)) ++states;
            const double score = static_cast<double>(hi - lo + 1) * (hi - lo + 1) * states;
            if (score > best) { best = score; best_lo = lo; best_hi = hi; }
        }
        L.hot_lo4 = 0;
        L.hot_k4 = 0x80808080u;
        if (best_hi >= best_lo) {
            L.hot_lo4 = static_cast<uint32_t>(best_lo) * 0x01010101u;
            L.hot_k4 = static_cast<uint32_t>(0x7F - best_hi) * 0x01010101u;
            for (size_t r = 0; r < rows; ++r) if (covers(r, best_lo, best_hi)) at[r * cols + ACC] |= 0x10000u;
        }
    }
    if (c_rule.empty()) { c_rule.push_back(0); c_rule.push_back(0); }
    // tier 3: one global image per handle: [capture-side records + final records][match-only records]; GxLds::rec_g /
    // fin_tags are byte offsets into it
    const size_t g_base = I.l2.size();
    uint32_t n_records = 0;
    if (tier >= 2) {
        img.bytes.clear();  // the record tiers have their own class map (classes renumbered so that sets become ranges)
        std::vector<uint32_t> items_g;
        if (!records_from_dense(T, at, rows, cols, dead_of_row, loop_set, simple, img, L, c_rule, tier == 3 ? &items_g : nullptr, &n_records)) return false;
        if (tier == 2 && img.bytes.size() + T.ops_off.size() * 4 + T.ops.size() * 2 + fin_rec.size() * 2 + 1024 > LDS_TABLE_BUDGET) return false;
        if (tier == 3) {
            L.c_base = static_cast<uint32_t>(g_base);  // (byte offset of this image's records in the global image)
            const uint8_t* ib = reinterpret_cast<const uint8_t*>(items_g.data());
            I.l2.insert(I.l2.end(), ib, ib + items_g.size() * 4);
            while (I.l2.size() % 16) I.l2.push_back(0);
            L.fin_tags = static_cast<uint32_t>(I.l2.size());
            const uint8_t* fr = reinterpret_cast<const uint8_t*>(fin_rec.data());
            I.l2.insert(I.l2.end(), fr, fr + fin_rec.size() * 2);
            while (I.l2.size() % 16) I.l2.push_back(0);
        }
    } else if (global) {
        L.at = 0;
        I.l2.assign(reinterpret_cast<const uint8_t*>(at.data()), reinterpret_cast<const uint8_t*>(at.data() + at.size()));
        while (I.l2.size() % 16) I.l2.push_back(0);
        L.fin_tags = static_cast<uint32_t>(I.l2.size());  // L2 tier: the final records follow the rows in global memory
        const uint8_t* fr = reinterpret_cast<const uint8_t*>(fin_rec.data());
        I.l2.insert(I.l2.end(), fr, fr + fin_rec.size() * 2);
    } else {
        L.at = static_cast<uint32_t>(img.put(at));
        if (L.at != AT) throw GxError(GX_E_ARG, "internal: LDS table image layout");
    }
    L.c_rule = static_cast<uint32_t>(img.put(c_rule));
    L.ops_off = static_cast<uint32_t>(img.put(T.ops_off));
    std::vector<uint16_t> ops = T.ops;
    if (ops.empty()) ops.push_back(0);
    L.ops = static_cast<uint32_t>(img.put(ops));
    if (!in_global) L.fin_tags = static_cast<uint32_t>(img.put(fin_rec));
    L.tier = static_cast<uint32_t>(tier);
    while (img.bytes.size() % 16) img.bytes.push_back(0);
    L.table_bytes = static_cast<uint32_t>(img.bytes.size());
    int max_regs = 0;
    for (auto& r : T.rules) max_regs = std::max(max_regs, r.n_regs);
    if (fused) max_regs = T.uni.n_regs;
    if (part == 2) max_regs = 0;
    L.regs_wave_bytes = static_cast<uint32_t>(((max_regs + 1) * 64 * 2 + 15) & ~15);  // + the dummy column
    DenseImage& D = I.dense[part == 2 ? 1 : 0];
    D.L = L;
    D.bytes.swap(img.bytes);
    D.rows = static_cast<uint32_t>(rows);
    D.records = n_records;
    D.fused = part != 2 && fused && T.has_capture;
    (part == 2 ? I.has_mo : I.tile_ok) = true;
    return true;
}

}  // namespace

const std::vector<uint8_t>* TileImages::image(int id) const {
    if (id == IMG_DENSE) return tile_ok ? &dense[0].bytes : nullptr;
    if (id == IMG_DENSE + 1) return tile_ok && has_mo ? &dense[1].bytes : nullptr;
    if (id == IMG_L2) return tile_ok && tile_global ? &l2 : nullptr;
    const HopTier& H = hop[(id - IMG_HOP) / 3];
    if (!H.ok) return nullptr;
    const int part = (id - IMG_HOP) % 3;
    return part == HOP_FULL ? &H.img.full.bytes : part == HOP_SMALL ? &H.img.small.bytes : &H.img.global;
}

// Complete the layout for one batch: staging sized for 64 lines of the hinted length.
// wide: the kernel variant that reads UTF-16 code units (two prefetch registers per staged chunk: 13 KB of staging and 8 waves at most)
bool plan_tile_launch(const TileImages& I, uint32_t line_bytes_hint, GxLds* out, bool mo, bool wide) {
    if (!I.tile_ok) return false;
    return plan_tile_layout(I.dense[I.dense_of(mo)].L, line_bytes_hint, out, wide);
}
// the hop tier's layout: the same kernel, its own tables
bool plan_hop_launch(const TileImages& I, uint32_t line_bytes_hint, GxLds* out, bool mo, bool wide) {
    return I.hop[mo].ok && plan_tile_layout(I.hop[mo].full, line_bytes_hint, out, wide);
}
bool plan_tile_layout(GxLds L, uint32_t line_bytes_hint, GxLds* out, bool wide) {
    if (line_bytes_hint == 0) line_bytes_hint = 200;
    if (line_bytes_hint > 2000) line_bytes_hint = 2000;
    L.stage_bytes = (64u * line_bytes_hint + 64u + 15u) & ~15u;  // + slack: the walk reads ahead of the line
    if (L.stage_bytes > 16384u) L.stage_bytes = 16384u;  // the kernel prefetches a tile into <= 64 VGPRs per lane;
                                                          // longer lines go in several rounds or to the per-line kernel
    if (wide && L.stage_bytes > 13u * 1024u) L.stage_bytes = 13u * 1024u;   // (groups of longer lines go in several rounds)
    const uint32_t bitmap_bytes = L.tier == 4 ? 0u : GX_BITMAP_WAVE_BYTES;   // (the hop tier has no chunk bitmap)
    const uint32_t fixed = L.regs_wave_bytes + bitmap_bytes;
    if (L.table_bytes + 4 * (L.stage_bytes + fixed) > LDS_BYTES) return false;
    uint32_t nw = (LDS_BYTES - L.table_bytes) / (L.stage_bytes + fixed);
    if (nw > 12) nw = 12;  // 768 threads: leaves 170 VGPRs per lane for the prefetch registers
    if ((wide || L.stage_bytes > 13u * 1024u) && nw > 8) nw = 8;  // the 16 KB variant prefetches 64 VGPRs, the UTF-16 variant 104: 2 waves per SIMD
#ifdef GX_DEV
    if (getenv("GX_DEV_NWAVES") && static_cast<uint32_t>(atoi(getenv("GX_DEV_NWAVES"))) < nw) nw = static_cast<uint32_t>(atoi(getenv("GX_DEV_NWAVES")));
#endif
    // Whatever LDS is left goes to the staging areas, up to what the kernel variant's prefetch registers hold: a hint
    // that is a few bytes short (mean length, lines of 201 bytes announced as 200) then still stages whole groups.
    {
        const uint32_t kch = (L.stage_bytes + 1023u) / 1024u;
        const uint32_t cap = (wide ? 13u : kch <= 4 ? 4u : kch <= 8 ? 8u : kch <= 13 ? 13u : 16u) * 1024u;
        uint32_t room = ((LDS_BYTES - L.table_bytes - 32u) / nw - fixed) & ~15u;
        if (room > cap) room = cap;
        if (room > L.stage_bytes) L.stage_bytes = room;
    }
    L.nwaves = nw;
    L.regs = L.table_bytes;
    L.bitmap = L.regs + nw * L.regs_wave_bytes;
    L.counter = L.bitmap + nw * bitmap_bytes;
    L.stage = (L.counter + 16u + 15u) & ~15u;
    L.total_bytes = L.stage + nw * L.stage_bytes;
    if (L.total_bytes > LDS_BYTES) { L.stage_bytes -= 16u; L.total_bytes = L.stage + nw * L.stage_bytes; }
    *out = L;
    return true;
}

// Layout for the lane kernel (gx_lanes.hip): per wave the register block and the area its result rows go through.
bool plan_lanes_launch(const TileImages& I, GxLds* out, bool mo, bool compact, bool sorted, uint64_t n, int num_cus) {
    if (!I.tile_ok) return false;
    GxLds L = I.dense[I.dense_of(mo)].L;
    if (!mo && I.has_capture && L.u_start == 0xFFFFFFFFu) return false;  // walks the fused automaton
    const uint32_t slots = 2u * static_cast<uint32_t>(I.max_groups);
    const uint32_t rows = mo || !compact ? 0u : 64u * row_bytes(ROWS_U16, slots);  // (u16 or u8 rows; dense rows are stored lane by lane)
    L.stage_bytes = L.regs_wave_bytes;                       // (the register block)
    L.regs_wave_bytes = (L.regs_wave_bytes + rows + 16u + 15u) & ~15u;
    // length-sorted tiles (uneven lines, tables in global memory): a chunk's line order, 2 bytes per line, + two 64-entry tables
    L.sort_chunk = 0;
    L.sort_lds = 0;
    uint32_t sort_bytes = 0;
    if (sorted) {
        // (with the tables in LDS too the index array takes the place of a wave or two)
        for (uint32_t ch = L.tier == 2 ? 2048u : 8192u; ch >= 2048u; ch >>= 1)  // (records in LDS: 2 048 lines cost one wave, 8 192 two)
            if (L.table_bytes + 32u + 2u * ch + 512u + (L.tier == 2 ? 14u : 8u) * L.regs_wave_bytes <= LDS_BYTES) { L.sort_chunk = ch; sort_bytes = 2u * ch + 512u; break; }
    }
    // Chunks are what the workgroups share the batch in, and a chunk ends with a barrier, so its waves want several tiles
    // each (measured: 1 M lines of 50-2000 bytes on the LDS records: chunks of 8 192 lines 0.82 ms -- 122 chunks for 256
    // CUs --, 2 048 lines 0.52 ms, 1 024 lines 0.95 ms -- one tile per wave and chunk; configs[4], 2 M lines: 8 192 1.75 ms,
    // 1 984 1.82 ms).  Small batches take smaller chunks, down to 2 048 lines.
    if (L.sort_chunk && n)
        while (L.sort_chunk > 2048u && n / L.sort_chunk < static_cast<uint64_t>(num_cus > 0 ? num_cus : 256) / 2) L.sort_chunk >>= 1;
    if (L.table_bytes + 32u + sort_bytes + 4u * L.regs_wave_bytes > LDS_BYTES) return false;
    L.nwaves = std::min<uint32_t>(16u, (LDS_BYTES - L.table_bytes - 32u - sort_bytes) / L.regs_wave_bytes);
    L.sort_lds = L.table_bytes;  // (behind the tables)
    L.regs = L.table_bytes + sort_bytes;
    L.bitmap = 0;
    L.counter = L.regs + L.nwaves * L.regs_wave_bytes;
    L.stage = 0;
    L.total_bytes = L.counter + 16u;
    if (L.total_bytes > LDS_BYTES) return false;
    *out = L;
    return true;
}

// Layout for the slice kernel: a 64 x 80-byte slice buffer per wave, up to 16 waves.
bool plan_slice_launch(const TileImages& I, GxLds* out, bool mo) {
    if (!I.tile_ok) return false;
    if (I.has_capture && I.dense[0].L.u_start == 0xFFFFFFFFu) return false;  // the slice kernel walks the fused automaton
    GxLds L = I.dense[I.dense_of(mo)].L;
    L.stage_bytes = 64u * 80u;
    const uint32_t per_wave = L.stage_bytes + L.regs_wave_bytes;
    if (L.table_bytes + per_wave > LDS_BYTES) return false;
    uint32_t nw = (LDS_BYTES - L.table_bytes) / per_wave;
    if (nw > 16) nw = 16;
    L.nwaves = nw;
    L.regs = L.table_bytes;
    L.bitmap = 0;
    L.stage = L.regs + nw * L.regs_wave_bytes;
    L.total_bytes = L.stage + nw * L.stage_bytes;
    *out = L;
    return true;
}

// Layout for the hop slice kernel: the hop tier's tables, per wave a register block and a [64][144]-byte piece buffer.
bool plan_hop_slice_launch(const TileImages& I, GxLds* out, bool mo) {
    if (!I.hop[mo].ok) return false;
    GxLds L = I.hop[mo].small;
    L.stage_bytes = 64u * (GX_HOP_SLICE_BYTES + 16u) + 48u;  // (+ 48: a window read at a row's last bytes runs a few bytes past it)
    const uint32_t per_wave = L.stage_bytes + L.regs_wave_bytes;
    if (L.table_bytes + 4u * per_wave > LDS_BYTES) return false;
    uint32_t nw = (LDS_BYTES - L.table_bytes) / per_wave;
    if (nw > 12) nw = 12;   // (the kernel holds the loads of eight tested lines across its walk: three waves per SIMD by registers)
    L.nwaves = nw;
    L.regs = L.table_bytes;
    L.bitmap = 0;
    L.stage = L.regs + nw * L.regs_wave_bytes;
    L.total_bytes = L.stage + nw * L.stage_bytes;
    *out = L;
    return true;
}

// Layout for the resident one-line service (gx_service.hip): the dense rows in LDS, and either no captures or the fused automaton
// with simple programs; one wave, its staging area holds the longest request and the answer.
bool plan_service(const TileImages& I, GxLds* out) {
    const GxLds& D = I.dense[0].L;
    if (!I.tile_ok || I.tile_global || D.tier != 0 || I.max_groups > 32 || (I.has_capture && (D.u_start == 0xFFFFFFFFu || !D.simple_ops))) return false;
    GxLds L = D;
    L.nwaves = 1;
    L.stage_bytes = ((GX_SERVICE_MAX_BYTES + 8u + 64u + 15u) & ~15u) + 272u;   // (+ the answer's words: gx_service.hip)
    L.regs = L.table_bytes;
    L.bitmap = L.regs + L.regs_wave_bytes;
    L.counter = L.bitmap + GX_BITMAP_WAVE_BYTES;
    L.stage = (L.counter + 16u + 15u) & ~15u;
    L.total_bytes = L.stage + L.stage_bytes;
    if (L.total_bytes > LDS_BYTES) return false;
    *out = L;
    return true;
}

// kernel choice: automaton rows in LDS when they fit, else sparse range records in LDS, else dense rows in global
// memory (L2), else the per-line kernel alone.  Host work only (also done for host-only handles, where it is a check
// of the builders and feeds gx_stat).
TileImages choose_tile_images(const Tables& T, uint32_t flags) {
    TileImages I;
    I.has_capture = T.has_capture;
    I.max_groups = T.max_groups;
    // (a definition with an extraction that has no capture automaton: the per-line kernel alone -- it is the one that runs programs)
    const bool no_tiles = (flags & GX_CREATE_NO_TILES) != 0 || T.has_pike(), force_l2 = (flags & GX_CREATE_TIER_L2) != 0;
    const bool force_rec = (flags & GX_CREATE_TIER_RECORDS) != 0;
    auto build = [&](int tier, int part = 0) { return build_tile_image(I, T, flags, tier, part); };
    auto records = [&](int tier) {
        if (build(tier)) return true;
        // the fused automaton alone, and a second image with the match automaton alone for match-only batches
        return build(tier, 1) && build(tier, 2);
    };
    const bool force_recg = (flags & GX_CREATE_TIER_RECORDS_GLOBAL) != 0;
    bool ok = false;
    if (!no_tiles) {
        if (force_l2) ok = build(1);
        else if (force_recg) ok = records(3) || build(1);
        else if (force_rec) ok = records(2) || records(3) || build(1);
        else {
            // Measured on the 64-extraction definition of BASELINE configs[2] (10 M x 200-byte lines), captures / match only:
            // range records in LDS walked by the lane kernel 1.9 / 1.4 ms; dense rows in global memory (L2) under the tile
            // kernel 3.0 / 3.0 ms; records in LDS under the tile kernel 3.9 / 1.9 ms; records in global memory 4.0 ms.
            // Hence: dense rows in LDS when they fit; else records in LDS when they fit beside at least 8 waves of the
            // lane kernel; else dense rows in global memory for the capture side and, when they fit, LDS records for
            // match-only batches.
            ok = build(0);
            if (!ok) {
                GxLds L;
                ok = records(2) && plan_lanes_launch(I, &L, false, true) && L.nwaves >= 8u;
                if (!ok) {
                    ok = build(1);
                    if (ok) (void)build(2, 2);
                }
            }
        }
    }
    if (!ok) I.tile_ok = false;
    // The hop tier beside it, for capture batches: whenever the dense rows do not fit LDS (or on request).  Its hot records
    // may take what LDS leaves beside eight waves' staging areas of 200-byte lines.
    const bool forced = force_l2 || force_rec || force_recg;  // (a caller that names a tier gets that tier's kernels)
    const bool want_hop = (flags & GX_CREATE_TIER_HOP) != 0 || (ok && !forced && (I.dense[0].L.tier != 0 || I.tile_global));
    uint32_t hot_budget = 48u * 1024u;
#ifdef GX_DEV
    if (getenv("GX_DEV_HOT_BUDGET")) hot_budget = static_cast<uint32_t>(atoi(getenv("GX_DEV_HOT_BUDGET")));
#endif
    uint32_t small_budget = 12u * 1024u;   // the hop slice kernel's share of LDS for hot records
#ifdef GX_DEV
    if (getenv("GX_DEV_SMALL_BUDGET")) small_budget = static_cast<uint32_t>(atoi(getenv("GX_DEV_SMALL_BUDGET")));
#endif
    // one hop image, and its layouts: the tile kernel's (full) and the hop slice kernel's (small: fewer hot records, more waves)
    auto hop_tier = [&](bool match_automaton) {
        HopTier& H = I.hop[match_automaton];
        if (!build_hop_image(T, match_automaton, hot_budget, small_budget, H.img)) return;
        const HopImage& M = H.img;
        GxLds L{};
        L.ncls = M.ncls;
        L.row_bytes = M.row_bytes;
        L.c_base = M.hops_off;
        L.m_start = M.match_automaton ? M.start : 0u;
        L.m_dead = M.match_automaton ? M.dead : 0u;
        L.u_start = M.match_automaton ? 0xFFFFFFFFu : M.start;
        L.u_dead = M.match_automaton ? 0xFFFFFFFFu : M.dead;
        L.fin_tags = M.fin_off;
        L.fin_state_off = M.fin_state_off;
        L.fin_state_rec = M.fin_state_rec;
        L.simple_ops = 1;
        L.tier = 4;
        L.rec = HOP_AT;
        L.sort_chunk = M.n_reachable_hot;  // (hop tier: the states well-formed lines reach; rec_indexed of them are in LDS)
        L.hot_lo4 = 0;
        L.hot_k4 = 0x80808080u;
        L.regs_wave_bytes = static_cast<uint32_t>(((M.n_regs + 1) * 64 * 2 + 15) & ~15u);   // (the dummy column, then the registers)
        L.fin_unset = M.col_unset;
        for (int q = 0; q < 2; ++q) {
            const HopLds& P = q ? M.small : M.full;
            L.table_bytes = static_cast<uint32_t>(P.bytes.size());
            L.rec_indexed = P.n_hot;
            L.acc_tab = P.info_lds;   // int16 info words of the hot states
            L.at = P.fin_lds;         // final records in LDS (0: in the global image at fin_tags)
            L.hop_sets = P.sets_lds;  // the loop sets (the walk's second chance)
            (q ? H.small : H.full) = L;
        }
        GxLds P;
        H.ok = plan_tile_layout(H.full, 200, &P);
    };
    I.hop_reason = 4;   // not built: the dense rows fit LDS (or the caller named another tier)
    if (!no_tiles && want_hop && T.has_capture && !(flags & GX_CREATE_NO_FUSED)) {
        hop_tier(false);
        I.hop_reason = !I.hop[0].img.ok ? static_cast<int>(I.hop[0].img.refused) : I.hop[0].ok ? 0 : 5;   // (5: the tables leave no room in LDS for a wave)
    } else if (want_hop && !no_tiles) I.hop_reason = 1;
    // ... and of the match automaton alone, for match-only batches (PolyMatcher.match over a batch)
    if (!no_tiles && want_hop) hop_tier(true);
    return I;
}

BatchPlan plan_batch(const TileImages& I, const BatchShape& s, int num_cus) {
    BatchPlan p;
    const uint32_t kernel = s.kernel;
    const bool mo = s.match_only != 0 || !I.has_capture;
    const int dense = IMG_DENSE + I.dense_of(mo), hop = IMG_HOP + 3 * mo;
    const uint32_t image_tier = I.dense[I.dense_of(mo)].L.tier;
    auto plan = [&](int k, int image, int global, uint32_t fits, uint32_t limit, int by_length) {
        p.kernel = k, p.image = image, p.global = global, p.fits = fits, p.limit = limit, p.by_length = by_length;
        return p;
    };
    // the kernels that stage whole lines: a line fits a wave's staging area when its bytes + the 15 its address may add + the walk's
    // look-ahead do
    auto tiles = [&](int k, int image, int global) { return plan(k, image, global, p.L.stage_bytes >= 63u ? p.L.stage_bytes - 63u : 0u, p.L.stage_bytes, 0); };
    // the kernels that take a line a piece at a time: the lines they leave are longer than their 16-bit positions
    auto pieces = [&](int k, int image, int global, uint32_t limit) { return plan(k, image, global, limit, limit, 1); };
    const uint32_t hint = s.line_bytes_hint;
    if (s.wide) {
        if (s.want_states || s.match_only < 0 || s.n == 0) return p;
        if (hint <= 255u && !s.uneven && (kernel == GX_KERNEL_AUTO || kernel == GX_KERNEL_TILES || kernel == GX_KERNEL_HOPS)) {
            // UTF-16 code units, lines of ordinary length, tables that are dense rows in LDS or hop tables: the tile kernel reads the
            // units itself -- their low bytes are what it stages -- and flags the lines that hold a unit above 0xFF for the per-line
            // walk (k_extract_flagged, which leaves at once when there is none).  No copy of the batch, no synchronisation.
            // (The hop tier of capture batches needs the fused automaton's start state.)
            const bool use_hop = I.hop[mo].ok && kernel != GX_KERNEL_TILES;
            if (use_hop && plan_hop_launch(I, hint, &p.L, mo, true) && (mo || I.hop[0].full.u_start != 0xFFFFFFFFu))
                return tiles(GX_KERNEL_HOPS, hop + HOP_FULL, hop + HOP_GLOBAL);
            if (!use_hop && kernel != GX_KERNEL_HOPS && I.tile_ok && !I.tile_global && image_tier == 0 && plan_tile_launch(I, hint, &p.L, mo, true))
                return tiles(GX_KERNEL_TILES, dense, -1);
        }
        // UTF-16 code units, long or uneven lines, hop tables: the hop slice kernel reads the units itself (a loading lane fetches 16
        // units and stages their low bytes) and flags the lines that hold a unit above 0xFF, as the tile kernel above.
        if ((hint > 255u || s.uneven || kernel == GX_KERNEL_HOP_SLICES) && (kernel == GX_KERNEL_AUTO || kernel == GX_KERNEL_HOP_SLICES) &&
            plan_hop_slice_launch(I, &p.L, mo))
            return pieces(GX_KERNEL_HOP_SLICES, hop + HOP_SMALL, hop + HOP_GLOBAL, 65535u);
        // any other kernel: the units narrowed to a copy of their low bytes first
        p.narrow = kernel != GX_KERNEL_PER_LINE;
        return p;
    }
    // (gx_match_batch wants the product-DFA state a line ends in: the tile kernel on dense rows -- a row is a state -- gives it for
    // match-only batches; every other kernel and table keeps only the first accepting extraction)
    const bool want_states = s.want_states;
    if ((want_states && s.match_only != 1) || s.match_only < 0 || kernel == GX_KERNEL_PER_LINE) return p;
    // Which kernel (gx_batch_opts.kernel 0), by the tables and the mean line length.  Measured, one device (ms; captures /
    // match only):
    //   README definition (dense rows in LDS), 2 M lines of 50-2000 bytes: tiles 0.39, slices 0.73, lanes on sorted tiles 0.75;
    //     400 k lines of 50-20000 bytes (mean 3.4 KB): tiles 61.7 (lines beyond the staging area go one by one), slices 1.74, lanes 3.4
    //   512 extractions, 2 M lines of 50-2000 bytes (configs[4]), dense rows in L2: tiles 4.4 / 4.0, slices 2.39 / 2.20,
    //     lanes 2.19 / 2.07, lanes on length-sorted tiles 1.77 / 1.56 (on range records in global memory 2.18 / 1.81)
    //   64 extractions, 1 M such lines, records in LDS: slices 1.04 / 0.74, lanes 1.41 / 1.22, lanes on sorted tiles 0.52 / 0.47;
    //     200 k lines of 50-20000 bytes: slices 5.1, lanes 9.4
    //   64 extractions, 10 M lines of 200 bytes (configs[2]): records in LDS + lanes 1.52 / 1.18, dense rows in L2 + tiles 3.0 / 3.0
    // Hence: a mean above 1 KB -> slice kernel (64 bytes of every line at a time, a lane takes its next line as soon as it is
    // done); dense rows in LDS -> tile kernel; records in LDS -> lane kernel; anything else -> tile kernel, or above 255 bytes
    // the lane kernel; the lane kernel on tiles of lines of similar length above 255 bytes (gx_lanes.hip, SORTED).
    const bool long_lines = hint > 255u, very_long = hint > 1024u;
    const bool sorted = long_lines || s.uneven;  // tiles of lines of similar length (the lane kernel's SORTED mode)
    const int global = image_tier == 1 || image_tier == 3 ? IMG_L2 : -1;
    // hop tier: capture batches of definitions whose dense rows do not fit LDS, lines of ordinary length and evenness (the
    // tile kernel wants a tile's lines to be neighbours in memory and about as long as each other)
    // ... and for long or uneven lines the hop slice kernel: a piece of every lane's own line at a time, lanes refilled
    const bool have_hop = I.hop[mo].ok && !want_states;
    if (have_hop && (kernel == GX_KERNEL_HOP_SLICES || (kernel == GX_KERNEL_AUTO && (long_lines || s.uneven))) && plan_hop_slice_launch(I, &p.L, mo))
        return pieces(GX_KERNEL_HOP_SLICES, hop + HOP_SMALL, hop + HOP_GLOBAL, 65535u);   // (lines beyond the 16-bit positions)
    if (have_hop && (kernel == GX_KERNEL_HOPS || (kernel == GX_KERNEL_AUTO && !long_lines && !s.uneven)) && plan_hop_launch(I, hint, &p.L, mo))
        return tiles(GX_KERNEL_HOPS, hop + HOP_FULL, hop + HOP_GLOBAL);
    // (the slice kernel takes every line: no follow-up launch)
    if ((kernel == GX_KERNEL_SLICES || (kernel == GX_KERNEL_AUTO && very_long)) && !want_states && plan_slice_launch(I, &p.L, mo))
        return plan(GX_KERNEL_SLICES, dense, global, 0, 0, 0);
    // records in LDS: the lane kernel (every lane keeps its own line in registers, 16 waves share the tables)
    const bool lanes = (kernel == GX_KERNEL_LANES || (kernel == GX_KERNEL_AUTO && (image_tier == 2 || (image_tier != 0 && long_lines)))) && !want_states;
    if (lanes && plan_lanes_launch(I, &p.L, mo, s.packed, sorted, s.n, num_cus)) {
        // (long lines: tiles of lines of similar length, see gx_lanes.hip; where LDS has no room for that, the slice kernel)
        GxLds S;
        if (kernel == GX_KERNEL_AUTO && long_lines && p.L.sort_chunk == 0 && plan_slice_launch(I, &S, mo)) {
            p.L = S;
            return plan(GX_KERNEL_SLICES, dense, global, 0, 0, 0);
        }
        // (the lines the lane kernel leaves: longer than its 16-bit positions -- with compact rows, than the largest offset u16 rows hold)
        return pieces(GX_KERNEL_LANES, dense, global, s.packed ? static_cast<uint32_t>(row_max_offset(ROWS_U16)) : 65535u);
    }
    if ((!want_states || image_tier <= 1u) && plan_tile_launch(I, hint, &p.L, mo)) return tiles(GX_KERNEL_TILES, dense, global);
    return p;
}

}  // namespace gx
