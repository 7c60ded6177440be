// Exercises lookupLines() and textLookupLines() of include/gorp.hpp.
//   lookup_api_test          : host-only checks (the refusals in their order, no device is an error, never a CPU path) -- no GPU needed
//   lookup_api_test --gpu    : also runs the calls on the device
// Prints the sizes of gx_lookup_out and gx_lookup_totals for tests/test_lookup_host.py.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gorp.hpp"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

// a failed login: a time, a user, the bytes sent
static const char* DEF =
    "pattern %num \\d+\n"
    "pattern %word \\w+\n"
    "extract LoginFailed {\n  template [$ts(%num)] failed $user(%word) $size(%num)\n}\n"
    "extract LoginOk {\n  template [$ts(%num)] ok $user(%word)\n}\n";

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && strcmp(argv[1], "--gpu") == 0;
    using namespace gorp;
    printf("sizeof gx_lookup_out %zu gx_lookup_totals %zu\n", sizeof(gx_lookup_out), sizeof(gx_lookup_totals));
    auto def = DefinitionReader::reader(DEF).read(gpu ? 0 : GX_CREATE_HOST_ONLY);
    CHECK(def->getExtractions().size() == 2);

    Gorp::GroupParts byUser = def->groupParts();
    byUser.of("LoginFailed", "user", "size").of("LoginOk", "user");
    const std::vector<std::string> lines = {"[58] failed ann 1", "[10] failed bob 2", "[59] failed ann 3", "nothing here", "[61] failed eve 4", "[70] failed bob 5",
                                            "[60] ok ann", "[200] failed dan 6", "[130] ok eve"};
    const std::vector<std::string> watched = {"bob", "ann", "zed", "bob", ""};
    std::string bytes, text;
    std::vector<uint32_t> off(1, 0);
    for (const std::string& ln : lines) { bytes += ln; text += ln + "\n"; off.push_back(static_cast<uint32_t>(bytes.size())); }
    const uint8_t* b = reinterpret_cast<const uint8_t*>(bytes.data());
    std::vector<int32_t> ids(lines.size(), -1), caps(lines.size() * 2 * static_cast<size_t>(def->maxGroups()), -1);
    Gorp::Where small = def->where();
    small.on("LoginFailed", "size").lt(static_cast<int64_t>(4));
    if (!gpu) {
        // refusals need no device ...
        try { def->lookupLines(b, off.data(), lines.size(), ids.data(), nullptr, byUser, watched); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }                                   // parts on dense ids without capture rows
        gx_group_part one[1] = {{0, 1, -1, 0}};
        gx_group_part many[65];
        for (int q = 0; q < 65; ++q) many[q] = gx_group_part{0, 1, -1, 0};
        const char* eu = "bobann";
        uint32_t eo[3] = {0, 3, 6};
        uint32_t room[64];
        gx_lookup_totals totals{};
        gx_lookup_out out{};
        gx_batch_opts opts{};
        opts.struct_size = sizeof(opts);
        const gx_group_part* parts = one;
        uint32_t n_parts = 1, keep = GX_LOOKUP_KEEP_NOTHING, flags = 0;
        uint64_t n = lines.size(), m = 2;
        const void *units = eu, *eoff = eo;
        const int32_t* rows = caps.data();
        auto call = [&](gx_lookup_totals* t) {
            return gx_lookup_lines(def->handle(), b, off.data(), n, ids.data(), rows, parts, n_parts, nullptr, 0, units, eoff, m, keep, flags, &out, t, &opts);
        };
        auto said = [](const char* words) { return std::string(gx_last_error()).find(words) != std::string::npos; };
        // ... in their order: each is given together with everything behind it in the order, and the first one answers
        out.entry_stats = reinterpret_cast<gx_measure_stats*>(room);   // (no value_group)
        keep = 3;
        out.out_caps = reinterpret_cast<int32_t*>(room);
        opts.compact_results = 1;
        eoff = nullptr;
        m = (1ull << 30) + 1;
        n = 0xFFFFFFFFull;
        CHECK(call(nullptr) == GX_E_ARG && said("totals is NULL"));
        flags = 2;
        CHECK(call(&totals) == GX_E_ARG && said("unknown flag bits"));
        flags = GX_GROUP_WEAK_HASH;
        parts = many; n_parts = 65;
        CHECK(call(&totals) == GX_E_LIMIT && said("more than 64 parts"));
        parts = one; n_parts = 1;
        one[0].key_group = 9;
        CHECK(call(&totals) == GX_E_ARG && said("key_group"));
        one[0].key_group = 1;
        opts.utf8 = 2;
        CHECK(call(&totals) == GX_E_ARG && said("utf8"));
        opts.utf8 = 0;
        opts.no_sync = 1;
        CHECK(call(&totals) == GX_E_ARG && said("no_sync"));
        opts.no_sync = 0;
        CHECK(call(&totals) == GX_E_ARG && said("entry_stats without a value_group"));
        out.entry_stats = nullptr;
        CHECK(call(&totals) == GX_E_ARG && said("keep is not one of"));
        keep = GX_LOOKUP_KEEP_NOTHING;
        CHECK(call(&totals) == GX_E_ARG && said("GX_LOOKUP_KEEP_NOTHING"));              // a batch output (out_caps) and nothing to keep
        keep = GX_LOOKUP_KEEP_OTHERS;
        CHECK(call(&totals) == GX_E_ARG && said("out_caps on compact rows"));
        opts.compact_results = 0;
        CHECK(call(&totals) == GX_E_LIMIT && said("2^32 - 1 lines"));
        n = lines.size();
        CHECK(call(&totals) == GX_E_ARG && said("entry_offsets is NULL"));
        eoff = eo;
        CHECK(call(&totals) == GX_E_LIMIT && said("more than 2^30 entries"));
        m = 2;
        eo[1] = 7;                                                                        // entry 1 runs backwards
        CHECK(call(&totals) == GX_E_LIMIT && said("entry of 4 G code units"));
        eo[1] = 3;
        units = nullptr;
        CHECK(call(&totals) == GX_E_ARG && said("entry_units is NULL"));
        units = eu;
        rows = nullptr;
        CHECK(call(&totals) == GX_E_ARG && said("need caps"));
        rows = caps.data();
        off[3] = off[2] - 1;                                                              // line 2 runs backwards
        CHECK(call(&totals) == GX_E_LIMIT && said("4 G code units"));
        off[3] = off[2] + static_cast<uint32_t>(lines[2].size());
        out.out_caps = nullptr;
        out.out_bytes = const_cast<char*>(eu) + 2;                                        // an output inside the dictionary
        out.out_bytes_cap = 2;
        CHECK(call(&totals) == GX_E_ARG && said("overlaps"));
        out.out_bytes = nullptr;
        out.line_entry = reinterpret_cast<uint32_t*>(ids.data());                         // ... and one on an input
        CHECK(call(&totals) == GX_E_ARG && said("overlaps"));
        out.line_entry = room;
        // the text form: `out` may not carry batch outputs; kept outputs need a keep
        out.out_index = room;
        auto text_call = [&](uint32_t k, uint8_t* kept) {
            return gx_text_lookup_lines(def->handle(), reinterpret_cast<const uint8_t*>(text.data()), text.size(), one, 1, nullptr, 0, eu, eo, 2, k, 0, &out, kept, 64,
                                        nullptr, nullptr, &totals, nullptr, nullptr, nullptr);
        };
        CHECK(text_call(GX_LOOKUP_KEEP_HITS, nullptr) == GX_E_ARG && said("five batch outputs"));
        out.out_index = nullptr;
        CHECK(text_call(GX_LOOKUP_KEEP_NOTHING, reinterpret_cast<uint8_t*>(room)) == GX_E_ARG && said("GX_LOOKUP_KEEP_NOTHING"));
        CHECK(text_call(7, nullptr) == GX_E_ARG && said("keep is not one of"));
        // ... and behind them no device is an error, never a CPU path: n == 0, n_parts == 0 and n_entries == 0 are legal
        CHECK(call(&totals) == GX_E_DEVICE);
        CHECK(totals.entries == 0 && totals.lines == 0 && totals.lines_out == 0);
        n = 0;
        CHECK(call(&totals) == GX_E_DEVICE);
        n = lines.size(); n_parts = 0; parts = nullptr;
        CHECK(call(&totals) == GX_E_DEVICE);
        n_parts = 1; parts = one; m = 0; units = nullptr; eoff = nullptr;
        CHECK(call(&totals) == GX_E_DEVICE);
        CHECK(text_call(GX_LOOKUP_KEEP_HITS, reinterpret_cast<uint8_t*>(room)) == GX_E_DEVICE);
        try { def->lookupLines(b, off.data(), lines.size(), ids.data(), caps.data(), byUser, watched, GX_LOOKUP_KEEP_HITS, &small); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        try { def->textLookupLines(text, byUser, watched); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        printf("host-only checks ok\n");
        return 0;
    }
    def->extractBatch(b, off.data(), lines.size(), ids.data(), caps.data());
    CHECK((ids == std::vector<int32_t>{0, 0, 0, -1, 0, 0, 1, 0, 1}));
    const uint32_t MISS = GX_LOOKUP_MISS, NONE = GX_LOOKUP_NONE;
    Gorp::Lookup r = def->lookupLines(b, off.data(), lines.size(), ids.data(), caps.data(), byUser, watched);
    CHECK((r.lineEntry == std::vector<uint32_t>{1, 0, 1, NONE, MISS, 0, 1, MISS, MISS}) && (r.entrySame == std::vector<uint32_t>{0, 1, 2, 0, 4}));
    CHECK((r.entryLines == std::vector<uint64_t>{2, 3, 0, 0, 0}) && (r.entryFirstLine == std::vector<uint32_t>{1, 0, NONE, NONE, NONE}));
    CHECK(r.entryStats.size() == 5 && r.entryStats[0].numbers == 2 && r.entryStats[0].sum_lo == 7 && r.entryStats[1].lines == 2 && r.entryStats[1].sum_lo == 4 &&
          r.entryStats[3].lines == 0);
    CHECK(r.totals.entries == 5 && r.totals.distinct_entries == 4 && r.totals.hit_entries == 2 && r.totals.lines == 8 && r.totals.keyed == 8 && r.totals.unset == 0 &&
          r.totals.hits == 5 && r.totals.misses == 3 && r.totals.lines_out == 0 && r.index.empty() && r.offsets.empty());
    // wanted.contains(user): the watched users' lines as a batch
    r = def->lookupLines(b, off.data(), lines.size(), ids.data(), caps.data(), byUser, watched, GX_LOOKUP_KEEP_HITS);
    CHECK((r.index == std::vector<uint32_t>{0, 1, 2, 5, 6}) && r.totals.lines_out == 5 && (r.ids == std::vector<int32_t>{0, 0, 0, 0, 1}));
    CHECK(std::string(r.bytes.begin(), r.bytes.end()) == lines[0] + lines[1] + lines[2] + lines[5] + lines[6] && r.offsets.size() == 6 && r.offsets[5] == r.bytes.size());
    CHECK(r.caps.size() == 5 * 2 * static_cast<size_t>(def->maxGroups()) && r.caps[0] == caps[0]);
    // !blocked.contains(user), under a term: ann's line of size 3 and bob's do count, eve's and dan's (4, 6) do not; the ok lines have no term
    r = def->lookupLines(b, off.data(), lines.size(), ids.data(), caps.data(), byUser, watched, GX_LOOKUP_KEEP_OTHERS, &small);
    CHECK((r.index == std::vector<uint32_t>{8}) && r.totals.lines == 5 && r.totals.misses == 1 && r.lineEntry[4] == NONE && r.lineEntry[5] == NONE);
    // no entries at all: every keyed line is a miss
    r = def->lookupLines(b, off.data(), lines.size(), ids.data(), caps.data(), byUser, {}, GX_LOOKUP_KEEP_OTHERS);
    CHECK(r.totals.entries == 0 && r.totals.misses == 8 && r.index.size() == 8 && r.entrySame.empty());
    // whole files
    std::vector<uint64_t> counts;
    uint64_t n_lines = 0;
    Gorp::Lookup t = def->textLookupLines(text, byUser, watched, GX_LOOKUP_KEEP_HITS, nullptr, &counts, &n_lines);
    CHECK(n_lines == lines.size() && (counts == std::vector<uint64_t>{6, 2, 1, 0, 0, 0}));
    CHECK((t.lineEntry == std::vector<uint32_t>{1, 0, 1, NONE, MISS, 0, 1, MISS, MISS}) && (t.index == std::vector<uint32_t>{0, 1, 2, 5, 6}) && t.ids.empty());
    // (the text form keeps the lines' original bytes, terminators included, as gx_text_select writes them)
    CHECK(std::string(t.bytes.begin(), t.bytes.end()) == lines[0] + "\n" + lines[1] + "\n" + lines[2] + "\n" + lines[5] + "\n" + lines[6] + "\n");
    CHECK((t.entryLines == std::vector<uint64_t>{2, 3, 0, 0, 0}) && t.offsets.size() == 6 && t.offsets[5] == t.bytes.size() && t.totals.units_out == t.bytes.size());
    printf("GPU checks ok\n");
    return 0;
}
