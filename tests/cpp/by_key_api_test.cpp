// Exercises linesByKey() and textLinesByKey() of include/gorp.hpp, with the GroupParts builder reused.
//   by_key_api_test          : host-only checks (refusals, no device is an error, never a CPU path) -- no GPU needed
//   by_key_api_test --gpu    : also runs the calls on the device
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gorp.hpp"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

// the README definition (README.md:114-135)
static const char* DEF =
    "pattern %num \\d+\n"
    "pattern %word \\w+\n"
    "pattern %phrase \\S+\n"
    "extract PutRequest {\n  template [$timestamp(%num)]: $verb(PUT) $timeTakenInMsec(%num)ms $path(%phrase)\n}\n"
    "extract GetRequest {\n  template [$timestamp(%num)]: $verb(GET) $timeTakenInMsec(%num)ms $path(%phrase)\n}\n"
    "extract OtherRequest {\n  template [$timestamp(%num)]: $verb(%word) $timeTakenInMsec(%num)ms $path(%phrase)\n}\n";

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && strcmp(argv[1], "--gpu") == 0;
    using namespace gorp;
    auto def = DefinitionReader::reader(DEF).read(gpu ? 0 : GX_CREATE_HOST_ONLY);
    CHECK(def->getExtractions().size() == 3);

    Gorp::GroupParts byVerb = def->groupParts();
    byVerb.of("GetRequest", "verb", "timeTakenInMsec").of("PutRequest", "verb").of(2, 1, 2);
    Gorp::GroupParts byPath = def->groupParts();
    byPath.of("GetRequest", "path").of("OtherRequest", "path").of("PutRequest", "path");
    const std::vector<std::string> lines = {"[1]: GET 500ms /v1/a", "[2]: POST 499ms /v1/b", "[3]: PUT 900ms /v1/a", "nothing here", "[4]: POST 1ms /x",
                                            "[5]: GET 00501ms /v2/d", "[6]: HEAD 7ms /v1/a", "[7]: GET 77777ms /v1/", "[8]: GET 99999999999999999999ms /v1/a",
                                            "[9]: GET 500ms /v1/z", "[10]: POST 499ms /v1/b"};
    std::string bytes, text;
    std::vector<uint32_t> off(1, 0);
    for (const std::string& ln : lines) { bytes += ln; text += ln + "\n"; off.push_back(static_cast<uint32_t>(bytes.size())); }
    const uint8_t* b = reinterpret_cast<const uint8_t*>(bytes.data());
    std::vector<int32_t> ids(lines.size(), -1), caps(lines.size() * 2 * static_cast<size_t>(def->maxGroups()), -1);
    Gorp::Where v1 = def->where();
    v1.on("GetRequest", "path").startsWith("/v1/");
    if (!gpu) {
        // refusals need no device ...
        try { def->linesByKey(b, off.data(), lines.size(), ids.data(), nullptr, byVerb); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }                                   // parts on dense ids without capture rows
        try { def->linesByKey(b, off.data(), lines.size(), ids.data(), caps.data(), byVerb, 3, 2); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }                                   // min_lines above max_lines
        try { def->textLinesByKey(text, byPath, 2, 1); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }
        gx_group_part twice[2] = {{0, 0, -1, 0}, {0, 1, -1, 0}};
        gx_by_key_totals totals{};
        CHECK(gx_lines_by_key(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), twice, 2, nullptr, 0, 1, 0, 0, nullptr, nullptr, &totals, nullptr) == GX_E_ARG);
        CHECK(gx_lines_by_key(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), twice, 1, nullptr, 0, 1, 0, 4u, nullptr, nullptr, &totals, nullptr) == GX_E_ARG);
        CHECK(gx_lines_by_key(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), twice, 1, nullptr, 0, 1, 0, 0, nullptr, nullptr, nullptr, nullptr) == GX_E_ARG);
        gx_by_key_out into{};
        into.out_ids = ids.data();                                                             // an output that is an input
        into.cap_lines = lines.size();
        CHECK(gx_lines_by_key(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), twice, 1, nullptr, 0, 1, 0, 0, nullptr, &into, &totals, nullptr) == GX_E_ARG);
        // ... and behind them no device is an error, never a CPU path
        try { def->linesByKey(b, off.data(), lines.size(), ids.data(), caps.data(), byVerb, 2, 0, &v1); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        try { def->textLinesByKey(text, byPath, 1, 1); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        CHECK(gx_lines_by_key(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), twice, 1, nullptr, 0, 1, 0, GX_BY_KEY_ALL_DIGITS | GX_GROUP_WEAK_HASH,
                              nullptr, nullptr, &totals, nullptr) == GX_E_DEVICE);
        printf("host-only checks ok\n");
        return 0;
    }
    def->extractBatch(b, off.data(), lines.size(), ids.data(), caps.data());
    CHECK((ids == std::vector<int32_t>{1, 2, 0, -1, 2, 1, 2, 1, 1, 1, 2}));
    const size_t slots = 2 * static_cast<size_t>(def->maxGroups());
    // by verb, in order of appearance: GET (lines 0 5 7 8 9), POST (1 4 10), PUT (2), HEAD (6); line 3 has no key
    Gorp::LinesByKey g = def->linesByKey(b, off.data(), lines.size(), ids.data(), caps.data(), byVerb);
    CHECK((g.keys == std::vector<std::string>{"GET", "POST", "PUT", "HEAD"}) && (g.lines == std::vector<uint64_t>{5, 3, 1, 1}));
    CHECK((g.index == std::vector<uint32_t>{0, 5, 7, 8, 9, 1, 4, 10, 2, 6}) && (g.keyOutLines == std::vector<uint64_t>{0, 5, 8, 9, 10}));
    CHECK(g.byKey.keys_kept == 4 && g.byKey.lines_out == 10 && g.byKey.units_out == bytes.size() - lines[3].size() && g.byKey.group.n_keys == 4);
    CHECK(g.offsets.size() == 11 && g.offsets[0] == 0 && g.offsets[10] == g.bytes.size() && g.keyOutUnits[4] == g.bytes.size());
    for (size_t j = 0; j < g.index.size(); ++j) {
        const std::string& ln = lines[g.index[j]];
        CHECK(std::string(g.bytes.begin() + g.offsets[j], g.bytes.begin() + g.offsets[j + 1]) == ln);
        CHECK(g.ids[j] == ids[g.index[j]] && std::equal(g.caps.begin() + j * slots, g.caps.begin() + (j + 1) * slots, caps.begin() + g.index[j] * slots));
        CHECK(g.keyOutUnits[g.lineKey[g.index[j]]] <= g.offsets[j] && g.offsets[j + 1] <= g.keyOutUnits[g.lineKey[g.index[j]] + 1]);
    }
    CHECK(g.stats[0].numbers == 4 && g.stats[0].not_numbers == 1 && (g.lineKey == std::vector<uint32_t>{0, 1, 2, 0xFFFFFFFFu, 1, 0, 3, 0, 0, 0, 1}));
    // the keys with one line: PUT and HEAD
    g = def->linesByKey(b, off.data(), lines.size(), ids.data(), caps.data(), byVerb, 1, 1);
    CHECK((g.index == std::vector<uint32_t>{2, 6}) && (g.keyOutLines == std::vector<uint64_t>{0, 0, 0, 1, 2}) && g.byKey.keys_kept == 2 && g.keys.size() == 4);
    // at least five lines by path, GetRequest's under a term: /v1/a has four, so nothing is kept, and every key is still reported
    g = def->linesByKey(b, off.data(), lines.size(), ids.data(), caps.data(), byPath, 5, 0, &v1);
    CHECK(g.index.empty() && g.bytes.empty() && g.byKey.lines_out == 0 && g.byKey.keys_kept == 0 && g.keys.size() == g.keyOutLines.size() - 1 && g.keyOutLines.back() == 0);
    // by path with at least two lines: /v1/b (1 10) and /v1/a (0 2 6 8) -- in order of first appearance /v1/a, /v1/b
    g = def->linesByKey(b, off.data(), lines.size(), ids.data(), caps.data(), byPath, 2);
    CHECK((g.index == std::vector<uint32_t>{0, 2, 6, 8, 1, 10}) && g.byKey.keys_kept == 2 && g.keys[0] == "/v1/a" && g.keys[1] == "/v1/b");
    // whole files
    std::vector<uint64_t> counts;
    uint64_t n_lines = 0;
    Gorp::LinesByKey t = def->textLinesByKey(text, byVerb, 2, 0, nullptr, &counts, &n_lines);
    CHECK(n_lines == lines.size() && (counts == std::vector<uint64_t>{1, 5, 4, 1, 0, 0, 0, 0}));
    CHECK((t.index == std::vector<uint32_t>{0, 5, 7, 8, 9, 1, 4, 10}) && (t.keyOutLines == std::vector<uint64_t>{0, 5, 8, 8, 8}) && t.ids.empty());
    for (size_t j = 0; j < t.index.size(); ++j) CHECK(std::string(t.bytes.begin() + t.offsets[j], t.bytes.begin() + t.offsets[j + 1]) == lines[t.index[j]] + "\n");
    printf("GPU checks ok\n");
    return 0;
}
