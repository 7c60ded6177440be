// ASan/UBSan driver for the host-side compiler (no HIP): definitions -> regex strings -> tables -> blob -> tables; table images
// and the kernel a batch gets (gx_images.hpp); the launch slots' bookkeeping (gx_slots.hpp).
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "gx_common.hpp"
#include "gx_compile.hpp"
#include "gx_dsl.hpp"
#include "gx_hop.hpp"
#include "gx_images.hpp"
#include "gx_layout.hpp"
#include "gx_slots.hpp"
using namespace gx;

// ---- the hop tier's tables (gx_hop.hpp) walked on the host exactly as gx_hop_dev.hpp walks them, against the dense fused
// automaton: same extraction, same group spans, on lines sampled from the automaton and damaged copies of them ----
namespace {
struct Outcome { int id; std::vector<int> caps; bool operator==(const Outcome& o) const { return id == o.id && caps == o.caps; } };

Outcome dense_outcome(const Tables& T, const std::vector<uint8_t>& line) {
    const RuleTables& U = T.uni;
    std::vector<int> regs(static_cast<size_t>(U.n_regs) + 1, -1);
    uint32_t s = 0;
    for (size_t p = 0; p < line.size(); ++p) {
        const uint32_t w = U.trans[static_cast<size_t>(s) * T.ncls + T.cls256[line[p]]];
        s = w & 0xFFFFu;
        const uint32_t op = w >> 16;
        for (uint32_t j = T.ops_off[op]; op && j < T.ops_off[op + 1]; ++j)
            regs[T.ops[2 * j]] = T.ops[2 * j + 1] == GX_SRC_POS ? static_cast<int>(p) : regs[T.ops[2 * j + 1]];
    }
    Outcome o{U.fin[s] < 0 ? U.fin[s] : 0, {}};
    if (U.fin[s] < 0) return o;
    const int f = U.fin[s], k = T.fin_tags[f];
    o.id = k;
    for (int g = 0; g < T.rules[k].n_groups; ++g) {
        int v[2];
        for (int e = 0; e < 2; ++e) {
            const uint16_t t = T.fin_tags[f + 1 + 2 * g + e];
            v[e] = t == GX_SRC_POS ? static_cast<int>(line.size()) : t == GX_SRC_NIL ? -1 : regs[t];
        }
        if (v[0] < 0 || v[1] < 0) v[0] = v[1] = -1;
        o.caps.push_back(v[0]); o.caps.push_back(v[1]);
    }
    return o;
}

static size_t second_chances_total = 0;
Outcome hop_outcome(const Tables& T, const HopImage& H, const std::vector<uint8_t>& line, size_t* iterations, size_t* second_chances = &second_chances_total) {
    const uint32_t* rows = reinterpret_cast<const uint32_t*>(H.global.data());
    const uint32_t cols = H.row_bytes / 4;
    const uint8_t* hops = H.global.data() + H.hops_off;
    std::vector<uint8_t> cls(line.size() + 32, 0);   // (the staged bytes, as they are; H.full.bytes[b] = the class id of byte b)
    for (size_t i = 0; i < line.size(); ++i) cls[i] = line[i];
    std::vector<int> col(static_cast<size_t>(H.n_regs) + 2, -1);   // register columns (0 = the dummy)
    uint32_t s = H.start;
    size_t p = 0;
    const size_t e = line.size();
    while (p < e) {
        ++*iterations;
        uint32_t r[6];
        memcpy(r, hops + static_cast<size_t>(s) * HOP_REC_BYTES, HOP_REC_BYTES);
        const uint32_t run_lo = r[0] & 0xFFu, run_k = (r[0] >> 8) & 0xFFu, klen = (r[0] >> 16) & 0xFFu;
        size_t n = 0;
        while (n < 16 && p + n < e && run_k != 0x80u && cls[p + n] < 0x80u && cls[p + n] >= run_lo && cls[p + n] <= 0x7Fu - run_k) ++n;
        const size_t q = p + n;
        if (n == 16 || q >= e) { p = q; continue; }
        // (w1: target | off1 << 16 | off2 << 24; w2: column1 * 128 | column2 * 128 << 16; w3: tail pos | lo << 8 | span << 16; w4, w5: single bytes)
        const uint8_t* lits = reinterpret_cast<const uint8_t*>(&r[4]);
        bool ok = q + klen <= e;
        for (int j = 0; j < 8 && ok; ++j) ok = lits[j] == 0 || cls[q + j] == lits[j];
        {
            const uint32_t tb = cls[q + (r[3] & 0xFFu)], lo = (r[3] >> 8) & 0xFFu, span = (r[3] >> 16) & 0xFFu;
            ok = ok && tb >= lo && tb - lo <= span;
        }
        if (ok) {
            col[(r[2] & 0xFFFFu) >> 7] = static_cast<int>(q + ((r[1] >> 16) & 0xFFu));
            col[(r[2] >> 16) >> 7] = static_cast<int>(q + (r[1] >> 24));
            p = q + klen;
            s = r[1] & 0xFFFFu;
        } else {
            // the chain again with the tail byte against the union of the tail's byte set
            {
                const uint8_t* ts = H.full.bytes.data() + H.full.sets_lds + 8u * (r[3] >> 24);
                bool lits_ok = q + klen <= e;
                for (int j = 0; j < 8 && lits_ok; ++j) lits_ok = lits[j] == 0 || cls[q + j] == lits[j];
                const uint8_t tb = cls[q + (r[3] & 0xFFu)];
                bool in = false;
                for (int j = 0; j < 4; ++j) in = in || (ts[4 + j] != 0x80u && tb < 0x80u && tb >= ts[j] && tb <= 0x7Fu - ts[4 + j]);
                if (lits_ok && in && (r[3] >> 24) != 0) {
                    col[(r[2] & 0xFFFFu) >> 7] = static_cast<int>(q + ((r[1] >> 16) & 0xFFu));
                    col[(r[2] >> 16) >> 7] = static_cast<int>(q + (r[1] >> 24));
                    p = q + klen;
                    s = r[1] & 0xFFFFu;
                    ++*second_chances;
                    continue;
                }
            }
            // the second chance: the window at p against the union of the state's loop set (H.full.bytes at sets_lds: u8 lo[4], u8 k[4] per entry)
            const uint8_t* ls = H.full.bytes.data() + H.full.sets_lds + 8u * (r[0] >> 24);
            size_t nu = 0;
            auto in_union = [&](uint8_t b) { for (int j = 0; j < 4; ++j) if (ls[4 + j] != 0x80u && b < 0x80u && b >= ls[j] && b <= 0x7Fu - ls[4 + j]) return true; return false; };
            while (nu < 16 && p + nu < e && in_union(cls[p + nu])) ++nu;
            if (nu > n) { p = p + nu; ++*second_chances; continue; }
            const uint32_t x = rows[static_cast<size_t>(s) * cols + H.full.bytes[cls[q]]];
            col[x >> 16] = static_cast<int>(q);
            s = x & 0xFFFFu;
            p = s == H.dead ? e : q + 1;
        }
    }
    const int32_t info = static_cast<int32_t>(rows[static_cast<size_t>(s) * cols + H.ncls]);
    Outcome o{info < 0 ? info : 0, {}};
    if (H.match_automaton) { o.id = info; return o; }   // (the first accepting extraction, or -1)
    if (info < 0) return o;
    const uint16_t* rec = reinterpret_cast<const uint16_t*>(H.global.data() + H.fin_off + info);
    const size_t tag_slots = 8 * static_cast<size_t>((T.max_groups + 3) / 4);
    o.id = static_cast<int16_t>(rec[tag_slots]);
    for (int g = 0; g < T.rules[o.id].n_groups; ++g) {
        int v[2];
        for (int e2 = 0; e2 < 2; ++e2) {
            // (every tag names a column: a register's, "the length" = the dummy column 0, "unset" = H.col_unset)
            const uint16_t t = rec[2 * g + e2];
            v[e2] = t == H.col_unset ? -1 : t == 0 ? static_cast<int>(line.size()) : col[t / 128];
        }
        if (rec[2 * g] == H.col_unset || rec[2 * g + 1] == H.col_unset) v[0] = v[1] = -1;
        o.caps.push_back(v[0]); o.caps.push_back(v[1]);
    }
    return o;
}

// PolyMatcher.match on the dense match automaton: the first accepting extraction of the final state, or -1
Outcome dense_match(const Tables& T, const std::vector<uint8_t>& line) {
    uint32_t s = 0;
    for (uint8_t b : line) s = T.m_next[static_cast<size_t>(s) * T.ncls + T.cls256[b]];
    return Outcome{T.m_accept_first[s], {}};
}

// returns the number of lines checked (0: the definition is outside the hop tier's limits); throws on a difference
size_t check_hop_tier(const Tables& T, uint64_t seed) {
    size_t checked = 0, iterations = 0, bytes = 0;
    for (uint32_t budget : {48u * 1024u, 3u * HOP_REC_BYTES}) {   // (a tiny LDS budget: another state order)
        HopImage H, M;
        if (!build_hop_image(T, false, budget, 2u * HOP_REC_BYTES, H)) return 0;
        if (!build_hop_image(T, true, budget, 2u * HOP_REC_BYTES, M)) return 0;   // the match automaton alone
        if (H.small.bytes.size() > H.full.bytes.size() || memcmp(H.small.bytes.data(), H.full.bytes.data(), 256) != 0) throw std::runtime_error("hop tier: the two LDS images disagree");
        uint64_t rng = seed * 0x9E3779B97F4A7C15ull + budget;
        auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
        std::vector<std::vector<uint8_t>> of_class(T.ncls);
        for (int b = 0; b < 256; ++b) of_class[T.cls256[b]].push_back(static_cast<uint8_t>(b));
        for (int l = 0; l < 200; ++l) {
            // a walk through the live transitions of the dense automaton, then (two lines in three) some damage
            std::vector<uint8_t> line;
            uint32_t s = 0;
            const size_t want = next() % 150;
            while (line.size() < want) {
                std::vector<int> live;
                for (int c = 0; c < T.ncls; ++c) if ((T.uni.trans[static_cast<size_t>(s) * T.ncls + c] & 0xFFFFu) != static_cast<uint32_t>(T.uni.dead)) live.push_back(c);
                if (live.empty()) break;
                const int c = live[next() % live.size()];
                // (printable bytes first: they are what the chains are built for)
                uint8_t b = of_class[c][next() % of_class[c].size()];
                for (int tries = 0; tries < 8 && !(b >= 0x20 && b < 0x7F); ++tries) b = of_class[c][next() % of_class[c].size()];
                line.push_back(b);
                s = T.uni.trans[static_cast<size_t>(s) * T.ncls + c] & 0xFFFFu;
            }
            for (int d = static_cast<int>(next() % 3); d > 0 && !line.empty(); --d) {
                const size_t at = next() % line.size();
                switch (next() % 3) {
                case 0: line[at] = static_cast<uint8_t>(next()); break;
                case 1: line.erase(line.begin() + at); break;
                default: line.insert(line.begin() + at, line[next() % line.size()]);
                }
            }
            if (!(dense_outcome(T, line) == hop_outcome(T, H, line, &iterations)))
                throw std::runtime_error("hop tier and dense automaton disagree on a line of " + std::to_string(line.size()) + " bytes");
            if (!(dense_match(T, line) == hop_outcome(T, M, line, &iterations)))
                throw std::runtime_error("hop tier and dense match automaton disagree on a line of " + std::to_string(line.size()) + " bytes");
            ++checked;
            bytes += line.size();
        }
    }
    (void)iterations; (void)bytes;
    return checked;
}

// A planned LDS layout fits: its regions in ascending order inside LDS, the table image a multiple of 16 bytes.
bool layout_fits(const GxLds& L) {
    if (L.table_bytes % 16 || L.nwaves == 0 || L.total_bytes > LDS_BYTES) return false;
    uint32_t at = L.table_bytes;
    for (uint32_t r : {L.regs, L.bitmap, L.counter, L.stage, L.total_bytes}) {
        if (r == 0) continue;   // (a region the kernel does not have)
        if (r < at) return false;
        at = r;
    }
    return true;
}

const uint32_t FLAG_SETS[] = {0u, GX_CREATE_TIER_L2, GX_CREATE_TIER_RECORDS, GX_CREATE_TIER_RECORDS_GLOBAL, GX_CREATE_TIER_HOP, GX_CREATE_NO_FUSED,
                              GX_CREATE_TIER_RECORDS | GX_CREATE_NO_FUSED};

// choose_tile_images under `flags`, then plan_batch over a grid of batch shapes: every plan uses images that exist, and its layout fits.
// Returns the number of plans checked.
size_t check_plans(const Tables& T, uint32_t flags) {
    const TileImages I = choose_tile_images(T, flags);
    size_t checked = 0;
    for (uint32_t hint : {0u, 50u, 200u, 255u, 256u, 1500u, 4000u})
        for (int shape = 0; shape < 32; ++shape)
            for (uint32_t kernel = GX_KERNEL_AUTO; kernel <= GX_KERNEL_HOP_SLICES; ++kernel) {
                BatchShape s;
                s.line_bytes_hint = hint;
                s.uneven = shape & 1;
                s.wide = shape & 2;
                s.match_only = (shape >> 2) & 1;
                s.packed = shape & 8;
                s.want_states = (shape & 16) && s.match_only;
                s.n = 1u << 20;
                s.kernel = kernel;
                const BatchPlan p = plan_batch(I, s, 256);
                ++checked;
                if (p.narrow) {
                    if (!s.wide) throw std::runtime_error("plan_batch: bytes to narrow");
                    continue;
                }
                if (p.kernel == GX_KERNEL_PER_LINE) {
                    if (p.image >= 0 || p.global >= 0) throw std::runtime_error("plan_batch: the per-line kernel with table images");
                    continue;
                }
                if (p.image < 0 || !I.image(p.image) || (p.global >= 0 && !I.image(p.global)))
                    throw std::runtime_error("plan_batch: kernel " + std::to_string(p.kernel) + " on an image that does not exist");
                if (!layout_fits(p.L)) throw std::runtime_error("plan_batch: kernel " + std::to_string(p.kernel) + " with a layout that does not fit LDS");
            }
    GxLds L;
    if (plan_service(I, &L) && !layout_fits(L)) throw std::runtime_error("plan_service: a layout that does not fit LDS");
    return checked;
}

// The kernel AUTO gives a few batch shapes (GX_KERNEL_*; n: the UTF-16 units narrowed first), for a test to pin.
std::string pinned_plans(const Tables& T, uint32_t flags) {
    const TileImages I = choose_tile_images(T, flags);
    struct Row { bool wide; int match_only; bool states; uint32_t hint; bool uneven; uint32_t kernel; };
    const Row rows[] = {{false, 0, false, 200, false, 0}, {false, 0, false, 200, true, 0}, {false, 0, false, 400, false, 0},
                        {false, 0, false, 1500, false, 0}, {false, 1, false, 200, false, 0}, {false, 1, true, 200, false, 0},
                        {true, 0, false, 200, false, 0}, {true, 0, false, 1500, false, 0}, {false, 0, false, 200, false, GX_KERNEL_HOP_SLICES},
                        {false, 0, false, 200, false, GX_KERNEL_PER_LINE}};
    std::string out;
    for (const Row& r : rows) {
        BatchShape s;
        s.wide = r.wide;
        s.match_only = r.match_only;
        s.want_states = r.states;
        s.line_bytes_hint = r.hint;
        s.uneven = r.uneven;
        s.kernel = r.kernel;
        s.n = 1u << 20;
        const BatchPlan p = plan_batch(I, s, 256);
        out += p.narrow ? std::string(" n") : " " + std::to_string(p.kernel);
    }
    return out;
}

// The launch slots' bookkeeping over stream keys, as gx_api.cpp drives it.  Returns what went wrong (empty: nothing).
std::string check_launch_slots() {
    LaunchSlots S;
    uint32_t broken[2 * LaunchSlots::N] = {};   // a word and, N behind it, a count per slot
    S.broken = broken;
    S.broken_count = broken + LaunchSlots::N;
    int keys[40];
    // repeat calls from one key: the same slot, a new sequence number each time
    const LaunchSlots::Use a = S.take(&keys[0]), b = S.take(&keys[0]);
    if (a.slot != 0 || b.slot != 0 || a.shared || a.wait_shared || b.seq == a.seq || S.slot_of(&keys[0]) != 0) return "repeat calls from one key";
    // 31 distinct keys take slots 0-30; the keys after them share slot 31, each user after the first waiting for the one before
    for (int k = 1; k < 31; ++k)
        if (S.take(&keys[k]).slot != k) return "key " + std::to_string(k) + " did not take slot " + std::to_string(k);
    for (int k = 31; k < 40; ++k) {
        const LaunchSlots::Use u = S.take(&keys[k]);
        if (u.slot != LaunchSlots::N - 1 || !u.shared || u.wait_shared != (k > 31)) return "key " + std::to_string(k) + " did not share the last slot";
    }
    if (S.slot_of(&keys[30]) != 30 || S.slot_of(&keys[35]) != LaunchSlots::N - 1 || S.take(&keys[7]).slot != 7) return "slot_of";
    // a launch that broke its promise (its number in the word, one more in the count) is reported once and counted once
    if (S.consume_broken(3)) return "an unchanged count reported";
    broken[3] = 7, broken[LaunchSlots::N + 3] = 1;
    if (S.consume_broken(3) != 1 || S.consume_broken(3) || S.promises_broken.load() != 1) return "a break not reported exactly once";
    // the synchronous fix-up finds its own sequence number in the word: accounted for, not reported again (tests/cpp/slots_test.cpp
    // has the orders in which an earlier launch's break meets it)
    broken[5] = 9, broken[LaunchSlots::N + 5] = 1;
    const LaunchSlots::Verdict v = S.finished(5, 9, true);
    if (!v.mine || v.earlier || S.consume_broken(5) || S.promises_broken.load() != 2) return "a launch's own break";
    // words without counts: a changed word is reported once and counted once, then reads as seen; the synchronous fix-up marks its
    // own sequence number seen, and that word is not reported again
    LaunchSlots W;
    uint32_t words[LaunchSlots::N] = {};
    W.broken = words;
    if (W.consume_broken(3)) return "an unchanged word reported";
    words[3] = 7;
    if (!W.consume_broken(3) || W.consume_broken(3) || W.promises_broken.load() != 1) return "a changed word not reported exactly once";
    words[5] = 9;
    W.mark_seen(5, 9);
    if (W.consume_broken(5) || W.promises_broken.load() != 2) return "a word marked seen reported";
    words[6] = 4;
    const LaunchSlots::Verdict w = W.finished(6, 4, true);
    if (!w.mine || w.earlier || W.finished(6, 4, true).mine || W.promises_broken.load() != 3) return "a launch's own break, words alone";
    // sequence numbers skip 0 when they wrap
    S.next_seq = 0xFFFFFFFFu;
    if (S.take(&keys[0]).seq != 0xFFFFFFFFu || S.take(&keys[0]).seq != 1) return "sequence numbers through 0";
    // the default stream (a null key) owns a slot like any other; a handle without pinned words reports nothing
    LaunchSlots T;
    if (T.take(nullptr).slot != 0 || T.take(&keys[0]).slot != 1 || T.take(nullptr).slot != 0 || T.consume_broken(0)) return "null key";
    return "";
}
// The result-row formats (gx_layout.hpp): sizes as bench.py prints them, and encode / decode at the edges of every format.
std::string check_row_formats() {
    for (uint32_t g = 0; g <= 64; ++g) {
        if (row_bytes(ROWS_U8, 2 * g) != 1 + 2 * g || row_bytes(ROWS_U16, 2 * g) != 2 + 4 * g || row_bytes(ROWS_DENSE, 2 * g) != 4 + 8 * g)
            return "row_bytes";
    }
    const RowFormat fmts[3] = {ROWS_DENSE, ROWS_U16, ROWS_U8};
    for (RowFormat f : fmts) {
        for (int32_t v : {-1, 0, 253, 254, 255, 65533, 65534, 65535, 65536}) {
            const RowUnit u = encode_offset(f, v);
            const int32_t lim = row_max_offset(f);
            const int32_t want = v < 0 ? -1 : v > lim ? lim : v;
            if (u.unit > row_unset(f) || decode_offset(f, u.unit) != want || u.clipped != (v > lim ? 1u : 0u)) return "encode / decode of an offset";
            if (v >= 0 && u.unit == row_unset(f)) return "an offset stored as unset";
        }
        for (int32_t id : {-2 - 126, -2, -1, 0, 1, 126}) {
            if (decode_id(f, encode_id(f, id)) != id) return "encode / decode of a match id";
        }
    }
    if (row_unset(ROWS_U8) != 0xFFu || row_unset(ROWS_U16) != 0xFFFFu || row_max_offset(ROWS_U8) != 254 || row_max_offset(ROWS_U16) != 65534)
        return "the formats' limits";
    if (row_format(false, true) != ROWS_DENSE || row_format(true, false) != ROWS_U16 || row_format(true, true) != ROWS_U8) return "row_format";
    return "";
}
}  // namespace
int main(int argc, char** argv) {
    const std::string rows_wrong = check_row_formats();
    if (!rows_wrong.empty()) {
        printf("row formats: %s\n", rows_wrong.c_str());
        return 1;
    }
    const std::string slots_wrong = check_launch_slots();
    if (!slots_wrong.empty()) {
        printf("launch slots: %s\n", slots_wrong.c_str());
        return 1;
    }
    int ok = 0, bad = 0, mutated_ok = 0, mutated_bad = 0;
    size_t hop_lines = 0, hop_defs = 0, plans = 0;
    for (int a = 1; a < argc; ++a) {
        // --pin FILE: the kernel choice of a few batch shapes for that definition, as "pin FILE FLAGS: ..."
        const bool pin = strcmp(argv[a], "--pin") == 0 && a + 1 < argc;
        if (pin) ++a;
        std::ifstream f(argv[a]);
        std::stringstream ss; ss << f.rdbuf();
        const std::string text = ss.str();
        try {
            auto xs = dsl::read_definition(text, argv[a]);
            std::vector<ustr> au, jd;
            for (auto& x : xs) { std::string p, q; dsl::build_regex_strings(x, p, q); au.push_back(utf8_to_u16(p.c_str())); jd.push_back(utf8_to_u16(q.c_str())); }
            Tables T = compile_tables(au, &jd);
            auto blob = pack_blob(T);
            Tables U = unpack_blob(blob.data(), blob.size());
            (void)U;
            {   // GX_CREATE_PROGRAMS: every extraction that can be one kept as a program; the blob carries them and reads back the same
                Tables P = compile_tables(au, &jd, true);
                const auto pblob = pack_blob(P);
                const Tables Q = unpack_blob(pblob.data(), pblob.size());
                size_t programs = 0;
                for (auto& r : Q.rules) programs += r.pike ? 1 : 0;
                if (pack_blob(Q) != pblob || (P.ncls <= 256 && programs != Q.rules.size())) {
                    printf("programs: %s does not read back as it was written\n", argv[a]);
                    return 1;
                }
            }
            for (uint32_t flags : FLAG_SETS) {
                plans += check_plans(T, flags);
                if (pin) printf("pin %s %u:%s\n", argv[a], flags, pinned_plans(T, flags).c_str());
            }
            const size_t hop_checked = check_hop_tier(T, static_cast<uint64_t>(a));
            hop_lines += hop_checked;
            hop_defs += hop_checked ? 1 : 0;
            // damaged blobs (truncated, bytes overwritten): refused with an error or accepted, never walked out of bounds --
            // an accepted one is walked over every state and class the way the host-side matchers do
            uint64_t rng = 0x9E3779B97F4A7C15ull ^ blob.size();
            auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
            for (int m = 0; m < 60; ++m) {
                std::vector<uint8_t> b2 = blob;
                if (m % 3 == 0) b2.resize(next() % (b2.size() + 1));
                else for (int q = 0; q < 1 + m % 4 && !b2.empty(); ++q) b2[next() % b2.size()] = static_cast<uint8_t>(next());
                try {
                    Tables V = unpack_blob(b2.data(), b2.size());
                    size_t sink = 0;
                    for (int s = 0; s < V.m_states; ++s) {
                        for (int c = 0; c < V.ncls; ++c) sink += V.m_accept_first[V.m_next[static_cast<size_t>(s) * V.ncls + c]] + 2;
                        for (uint32_t i = V.m_accept_off[s]; i < V.m_accept_off[s + 1]; ++i) sink += V.m_accept_list[i];
                    }
                    auto walk = [&](const RuleTables& r) {
                        for (uint32_t w : r.trans) {
                            sink += r.fin[w & 0xFFFFu] + 3;
                            for (uint32_t j = V.ops_off[w >> 16]; (w >> 16) && j < V.ops_off[(w >> 16) + 1]; ++j) sink += V.ops[2 * j] + V.ops[2 * j + 1];
                        }
                    };
                    for (auto& r : V.rules) walk(r);
                    if (V.union_ok) walk(V.uni);
                    if (sink == 1) printf(" ");
                    ++mutated_ok;
                } catch (GxError&) { ++mutated_bad; }
            }
            (void)dsl::dump_json(text, argv[a], "flattened");
            ++ok;
        } catch (GxError& e) { ++bad; }
    }
    printf("asan driver: %d compiled, %d rejected; damaged blobs: %d accepted, %d refused\n", ok, bad, mutated_ok, mutated_bad);
    printf("batch plans: %zu checked\n", plans);
    printf("hop tier: %zu definitions, %zu lines agree with the dense automaton (%zu second chances on loop sets)\n", hop_defs, hop_lines, second_chances_total);
    return 0;
}
