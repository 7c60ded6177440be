// Exercises topGroups() and textTopGroups() of include/gorp.hpp, with the GroupParts builder reused.
//   top_groups_api_test          : host-only checks (refusals, no device is an error, never a CPU path) -- no GPU needed
//   top_groups_api_test --gpu    : also runs the calls on the device
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

    // GetRequest and OtherRequest keyed by verb and measured; PutRequest's part only counts
    Gorp::GroupParts byVerb = def->groupParts();
    byVerb.of("GetRequest", "verb", "timeTakenInMsec").of("PutRequest", "verb").of(2, 1, 2);
    Gorp::GroupParts counted = def->groupParts();
    counted.of("GetRequest", "path");
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
        try { def->topGroups(b, off.data(), lines.size(), ids.data(), nullptr, byVerb, 10); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }                                   // parts on dense ids without capture rows
        try { def->topGroups(b, off.data(), lines.size(), ids.data(), caps.data(), byVerb, 10, 5); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }                                   // rank_by out of range
        try { def->textTopGroups(text, counted, 10, GX_RANK_SUM); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }                                   // a rank by numbers where no part has a value group
        try { def->topGroups(b, off.data(), lines.size(), ids.data(), caps.data(), byVerb, GX_TOP_GROUPS_MAX + 1); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_LIMIT); }
        try { def->textTopGroups(text, byVerb, GX_TOP_GROUPS_MAX + 1, GX_RANK_MAX, false); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_LIMIT); }
        gx_group_part twice[2] = {{0, 0, -1, 0}, {0, 1, -1, 0}};
        gx_top_groups_totals totals{};
        CHECK(gx_top_groups(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), twice, 2, nullptr, 0, GX_RANK_LINES, 3, 0, 0, nullptr, &totals, nullptr) == GX_E_ARG);
        CHECK(gx_top_groups(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), twice, 1, nullptr, 0, GX_RANK_LINES, 3, 0, 4u, nullptr, &totals, nullptr) == GX_E_ARG);
        CHECK(gx_top_groups(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), twice, 1, nullptr, 0, GX_RANK_LINES, 3, 0, 0, nullptr, nullptr, nullptr) == GX_E_ARG);
        // ... and behind them no device is an error, never a CPU path
        try { def->topGroups(b, off.data(), lines.size(), ids.data(), caps.data(), byVerb, 10, GX_RANK_SUM, true, &v1, true); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        try { def->textTopGroups(text, counted, 0); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        printf("host-only checks ok\n");
        return 0;
    }
    def->extractBatch(b, off.data(), lines.size(), ids.data(), caps.data());
    CHECK((ids == std::vector<int32_t>{1, 2, 0, -1, 2, 1, 2, 1, 1, 1, 2}));
    // in order of appearance: GET (5 lines: 500, 501, 77777, one beyond int64, 500), POST (3: 499, 1, 499), PUT (1, counts only), HEAD (1: 7)
    Gorp::TopGroups g = def->topGroups(b, off.data(), lines.size(), ids.data(), caps.data(), byVerb, 3, GX_RANK_LINES, true, nullptr, true);
    CHECK((g.keys == std::vector<std::string>{"GET", "POST", "PUT"}) && (g.lines == std::vector<uint64_t>{5, 3, 1}) && (g.keyNumber == std::vector<uint32_t>{0, 1, 2}));
    CHECK(g.top.candidates == 4 && g.top.n_top == 3 && g.top.units_top == 10 && g.top.last_lo == 1 && g.top.last_hi == 0 && g.top.ties_left == 1);
    CHECK(g.totals.n_keys == 4 && g.stats[0].numbers == 4 && g.stats[0].not_numbers == 1 && g.stats[2].lines == 0);
    CHECK((g.lineRank == std::vector<uint32_t>{0, 1, 2, 0xFFFFFFFFu, 1, 0, 0xFFFFFFFFu, 0, 0, 0, 1}));
    // by the sum of the numbers: GET 79278, POST 999, HEAD 7; PUT has no number and is no candidate
    g = def->topGroups(b, off.data(), lines.size(), ids.data(), caps.data(), byVerb, 10, GX_RANK_SUM);
    CHECK((g.keys == std::vector<std::string>{"GET", "POST", "HEAD"}) && g.top.candidates == 3 && g.top.last_lo == 7 && g.top.ties_left == 0 && g.lineRank.empty());
    CHECK(g.stats[0].sum_lo == 79278 && g.stats[1].sum_lo == 999 && (g.firstLine == std::vector<uint32_t>{0, 1, 6}));
    // the smallest minimum first: POST 1, HEAD 7, GET 500
    g = def->topGroups(b, off.data(), lines.size(), ids.data(), caps.data(), byVerb, 2, GX_RANK_MIN, false);
    CHECK((g.keys == std::vector<std::string>{"POST", "HEAD"}) && (g.keyNumber == std::vector<uint32_t>{1, 3}) && g.top.last_lo == 7);
    // keyed by path, with terms: GetRequest's lines whose path starts with /v1/ -- /v1/a twice, then the ties in order of appearance
    g = def->topGroups(b, off.data(), lines.size(), ids.data(), caps.data(), counted, 2, GX_RANK_LINES, true, &v1);
    CHECK((g.keys == std::vector<std::string>{"/v1/a", "/v1/"}) && (g.lines == std::vector<uint64_t>{2, 1}) && g.top.ties_left == 1 && g.stats.empty());
    // nothing wanted: the totals alone
    g = def->topGroups(b, off.data(), lines.size(), ids.data(), caps.data(), byVerb, 0);
    CHECK(g.keys.empty() && g.top.candidates == 4 && g.top.n_top == 0 && g.top.group.n_keys == 4);
    // whole files
    std::vector<uint64_t> counts;
    uint64_t n_lines = 0;
    Gorp::TopGroups t = def->textTopGroups(text, byVerb, 2, GX_RANK_MAX, true, nullptr, true, &counts, &n_lines);
    CHECK(n_lines == lines.size() && (counts == std::vector<uint64_t>{1, 5, 4, 1, 0, 0, 0, 0}));
    CHECK((t.keys == std::vector<std::string>{"GET", "POST"}) && t.stats[0].max == 77777 && t.top.last_lo == 499 && t.lineRank.size() == lines.size() && t.lineRank[2] == 0xFFFFFFFFu);
    printf("GPU checks ok\n");
    return 0;
}
