// Exercises groupPairs() and textGroupPairs() of include/gorp.hpp, with the PairParts builder.
//   pairs_api_test          : host-only checks (refusals, no device is an error, never a CPU path) -- no GPU needed
//   pairs_api_test --gpu    : also runs the calls on the device
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <stdexcept>
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

    Gorp::PairParts verbPath = def->pairParts();
    verbPath.of("GetRequest", "verb", "path", "timeTakenInMsec").of("PutRequest", "verb", "path").of(2, 1, 3);
    CHECK((verbPath.seconds() == std::vector<int32_t>{3, 3, 3}) && verbPath.keys().parts().size() == 3 && verbPath.keys().hasValues());
    Gorp::PairParts verbAlone = def->pairParts();
    verbAlone.of("GetRequest", "verb", "").of("PutRequest", "verb", "");
    CHECK((verbAlone.seconds() == std::vector<int32_t>{-1, -1}));
    try { def->pairParts().of("GetRequest", "verb", "nothing"); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->pairParts().of(0, 1, 4); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->pairParts().of(0, 1, -2); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->pairParts().of("GetRequest", "verb", "path").of("GetRequest", "path", "verb"); CHECK(false); } catch (std::invalid_argument&) {}
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
        try { def->groupPairs(b, off.data(), lines.size(), ids.data(), nullptr, verbPath); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }                                   // parts on dense ids without capture rows
        gx_group_part one[2] = {{0, 1, -1, 0}, {1, 1, -1, 0}};
        const int32_t none[2] = {-1, -1}, bad[2] = {3, 4}, fine[2] = {3, -1};
        gx_pairs_totals totals{};
        gx_pairs_out into{};
        std::vector<uint32_t> line_pair(lines.size());
        into.line_pair = line_pair.data();
        into.max_pairs = lines.size();
        CHECK(gx_group_pairs(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), one, 2, nullptr, nullptr, 0, 0, nullptr, nullptr, &totals, nullptr) == GX_E_ARG);
        CHECK(gx_group_pairs(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), one, 2, bad, nullptr, 0, 0, nullptr, nullptr, &totals, nullptr) == GX_E_ARG);
        CHECK(gx_group_pairs(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), one, 2, none, nullptr, 0, 0, nullptr, &into, &totals, nullptr) == GX_E_ARG);
        CHECK(gx_group_pairs(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), one, 2, fine, nullptr, 0, 0, nullptr, &into, nullptr, nullptr) == GX_E_ARG);
        into.max_pairs = (1ull << 30) + 1;
        CHECK(gx_group_pairs(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), one, 2, fine, nullptr, 0, 0, nullptr, &into, &totals, nullptr) == GX_E_LIMIT);
        CHECK(gx_text_group_pairs(def->handle(), reinterpret_cast<const uint8_t*>(text.data()), text.size(), one, 2, bad, nullptr, 0, 0, nullptr, nullptr, &totals, nullptr,
                                  nullptr, nullptr) == GX_E_ARG);
        // ... and behind them no device is an error, never a CPU path
        into.max_pairs = lines.size();
        CHECK(gx_group_pairs(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), one, 2, fine, nullptr, 0, GX_GROUP_WEAK_HASH, nullptr, &into, &totals,
                             nullptr) == GX_E_DEVICE);
        CHECK(gx_group_pairs(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), one, 2, none, nullptr, 0, 0, nullptr, nullptr, &totals, nullptr) == GX_E_DEVICE);
        try { def->groupPairs(b, off.data(), lines.size(), ids.data(), caps.data(), verbPath, &v1); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        try { def->groupPairs(b, off.data(), lines.size(), ids.data(), caps.data(), verbAlone); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        try { def->textGroupPairs(text, verbPath); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        printf("host-only checks ok\n");
        return 0;
    }
    def->extractBatch(b, off.data(), lines.size(), ids.data(), caps.data());
    CHECK((ids == std::vector<int32_t>{1, 2, 0, -1, 2, 1, 2, 1, 1, 1, 2}));
    // by (verb, path), in order of appearance: (GET /v1/a) lines 0 8, (POST /v1/b) 1 10, (PUT /v1/a) 2, (POST /x) 4, (GET /v2/d) 5, (HEAD /v1/a) 6, (GET /v1/) 7,
    // (GET /v1/z) 9; line 3 has neither
    Gorp::Pairs g = def->groupPairs(b, off.data(), lines.size(), ids.data(), caps.data(), verbPath);
    CHECK((g.keys == std::vector<std::string>{"GET", "POST", "PUT", "HEAD"}) && (g.lines == std::vector<uint64_t>{5, 3, 1, 1}));
    CHECK((g.pairKey == std::vector<uint32_t>{0, 1, 2, 1, 0, 3, 0, 0}));
    CHECK((g.seconds == std::vector<std::string>{"/v1/a", "/v1/b", "/v1/a", "/x", "/v2/d", "/v1/a", "/v1/", "/v1/z"}));
    CHECK((g.pairFirstLine == std::vector<uint32_t>{0, 1, 2, 4, 5, 6, 7, 9}) && (g.pairLines == std::vector<uint64_t>{2, 2, 1, 1, 1, 1, 1, 1}));
    CHECK((g.keyPairs == std::vector<uint64_t>{4, 2, 1, 1}));                                  // distinct paths per verb
    CHECK((g.linePair == std::vector<uint32_t>{0, 1, 2, 0xFFFFFFFFu, 3, 4, 5, 6, 0, 7, 1}) && (g.lineKey == std::vector<uint32_t>{0, 1, 2, 0xFFFFFFFFu, 1, 0, 3, 0, 0, 0, 1}));
    CHECK(g.pairs.n_pairs == 8 && g.pairs.paired == 10 && g.pairs.unpaired == 0 && g.pairs.pairs_exact == 1 && g.pairs.group.n_keys == 4 && g.totals.keyed == 10);
    CHECK(g.stats.size() == 4 && g.stats[0].numbers == 4 && g.stats[0].not_numbers == 1);
    // the keys are groupLines' own
    Gorp::Groups alone = def->groupLines(b, off.data(), lines.size(), ids.data(), caps.data(), verbPath.keys());
    CHECK(alone.keys == g.keys && alone.lines == g.lines && alone.firstLine == g.firstLine && alone.lineKey == g.lineKey);
    // GetRequest's lines under a term: /v2/d leaves
    g = def->groupPairs(b, off.data(), lines.size(), ids.data(), caps.data(), verbPath, &v1);
    CHECK(g.pairs.n_pairs == 7 && (g.keyPairs == std::vector<uint64_t>{3, 2, 1, 1}) && g.linePair[5] == 0xFFFFFFFFu);
    // no part has a second: every keyed line is unpaired
    g = def->groupPairs(b, off.data(), lines.size(), ids.data(), caps.data(), verbAlone);
    CHECK((g.keys == std::vector<std::string>{"GET", "PUT"}) && g.pairs.n_pairs == 0 && g.pairs.unpaired == 6 && g.pairKey.empty() && (g.keyPairs == std::vector<uint64_t>{0, 0}));
    CHECK(g.linePair == std::vector<uint32_t>(lines.size(), 0xFFFFFFFFu));
    // whole files
    std::vector<uint64_t> counts;
    uint64_t n_lines = 0;
    Gorp::Pairs t = def->textGroupPairs(text, verbPath, nullptr, &counts, &n_lines);
    CHECK(n_lines == lines.size() && (counts == std::vector<uint64_t>{1, 5, 4, 1, 0, 0, 0, 0}));
    CHECK((t.pairKey == std::vector<uint32_t>{0, 1, 2, 1, 0, 3, 0, 0}) && (t.keyPairs == std::vector<uint64_t>{4, 2, 1, 1}) && t.seconds[3] == "/x" && t.linePair.size() == lines.size());
    printf("GPU checks ok\n");
    return 0;
}
