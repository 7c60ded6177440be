// Exercises groupQuantiles() and textGroupQuantiles() of include/gorp.hpp, with the GroupParts builder reused.
//   group_quantile_api_test          : host-only checks (refusals, no device is an error, never a CPU path) -- no GPU needed
//   group_quantile_api_test --gpu    : also runs the calls on the device
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

static bool row(const gx_quantile_out& o, int64_t value, uint64_t rank, uint64_t below, uint64_t equal) {
    return o.value == value && o.rank == rank && o.below == below && o.equal == equal;
}

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && strcmp(argv[1], "--gpu") == 0;
    using namespace gorp;
    auto def = DefinitionReader::reader(DEF).read(gpu ? 0 : GX_CREATE_HOST_ONLY);
    CHECK(def->getExtractions().size() == 3);

    // GetRequest and OtherRequest keyed by verb and measured; PutRequest's part only counts
    Gorp::GroupParts byVerb = def->groupParts();
    byVerb.of("GetRequest", "verb", "timeTakenInMsec").of("PutRequest", "verb").of(2, 1, 2);
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
    const std::vector<gx_quantile> ends_and_median = {{0, 1}, {1, 2}, {1, 1}, {1, 2}};
    if (!gpu) {
        // refusals need no device ...
        try { def->groupQuantiles(b, off.data(), lines.size(), ids.data(), nullptr, byVerb, ends_and_median); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }                                   // parts on dense ids without capture rows
        try { def->groupQuantiles(b, off.data(), lines.size(), ids.data(), caps.data(), byVerb, {{1, 0}}); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }                                   // den == 0
        try { def->textGroupQuantiles(text, byVerb, {{3, 2}}); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }                                   // num > den
        try { def->groupQuantiles(b, off.data(), lines.size(), ids.data(), caps.data(), byVerb, std::vector<gx_quantile>(GX_QUANTILE_MAX + 1, gx_quantile{1, 2})); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_LIMIT); }
        try { def->textGroupQuantiles(text, byVerb, std::vector<gx_quantile>(GX_QUANTILE_MAX + 1, gx_quantile{1, 2})); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_LIMIT); }
        gx_group_part twice[2] = {{0, 0, -1, 0}, {0, 1, -1, 0}};
        gx_group_totals totals{};
        gx_quantile half{1, 2};
        CHECK(gx_group_quantiles(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), twice, 2, nullptr, 0, &half, 1, 0, nullptr, nullptr, &totals, nullptr) == GX_E_ARG);
        CHECK(gx_group_quantiles(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), twice, 1, nullptr, 0, nullptr, 1, 0, nullptr, nullptr, &totals, nullptr) == GX_E_ARG);
        // ... and behind them no device is an error, never a CPU path
        try { def->groupQuantiles(b, off.data(), lines.size(), ids.data(), caps.data(), byVerb, ends_and_median, &v1); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        try { def->textGroupQuantiles(text, byVerb, {}); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        printf("host-only checks ok\n");
        return 0;
    }
    def->extractBatch(b, off.data(), lines.size(), ids.data(), caps.data());
    CHECK((ids == std::vector<int32_t>{1, 2, 0, -1, 2, 1, 2, 1, 1, 1, 2}));
    Gorp::GroupQuantiles g = def->groupQuantiles(b, off.data(), lines.size(), ids.data(), caps.data(), byVerb, ends_and_median);
    // in order of appearance: GET (500, 501, 77777, one beyond int64, 500), POST (499, 1, 499), PUT (counts only), HEAD (7)
    CHECK((g.keys == std::vector<std::string>{"GET", "POST", "PUT", "HEAD"}) && (g.lines == std::vector<uint64_t>{5, 3, 1, 1}));
    CHECK(g.nQuantiles == 4 && g.quantiles.size() == 16 && g.stats[0].numbers == 4 && g.stats[0].not_numbers == 1 && g.stats[2].lines == 0);
    CHECK(row(g.at(0, 0), 500, 1, 0, 2) && row(g.at(0, 1), 500, 2, 0, 2) && row(g.at(0, 2), 77777, 4, 3, 1) && row(g.at(0, 3), 500, 2, 0, 2));
    CHECK(row(g.at(1, 0), 1, 1, 0, 1) && row(g.at(1, 1), 499, 2, 1, 2) && row(g.at(1, 2), 499, 3, 1, 2));
    CHECK(row(g.at(2, 0), 0, 0, 0, 0) && row(g.at(2, 2), 0, 0, 0, 0));
    CHECK(row(g.at(3, 0), 7, 1, 0, 1) && row(g.at(3, 1), 7, 1, 0, 1) && row(g.at(3, 2), 7, 1, 0, 1));
    // the groups are groupLines' own
    Gorp::Groups plain = def->groupLines(b, off.data(), lines.size(), ids.data(), caps.data(), byVerb);
    CHECK(plain.keys == g.keys && plain.lines == g.lines && plain.firstLine == g.firstLine && plain.lineKey == g.lineKey);
    CHECK(memcmp(plain.stats.data(), g.stats.data(), plain.stats.size() * sizeof(gx_measure_stats)) == 0);
    // keyed by path, with terms: GetRequest's lines whose path starts with /v1/; no quantiles at all
    Gorp::GroupParts byPath = def->groupParts();
    byPath.of("GetRequest", "path", "timeTakenInMsec").of("PutRequest", "path");
    g = def->groupQuantiles(b, off.data(), lines.size(), ids.data(), caps.data(), byPath, {{1, 2}}, &v1);
    CHECK((g.keys == std::vector<std::string>{"/v1/a", "/v1/", "/v1/z"}) && (g.lines == std::vector<uint64_t>{3, 1, 1}));
    CHECK(row(g.at(0, 0), 500, 1, 0, 1) && row(g.at(1, 0), 77777, 1, 0, 1) && row(g.at(2, 0), 500, 1, 0, 1));
    g = def->groupQuantiles(b, off.data(), lines.size(), ids.data(), caps.data(), byPath, {});
    CHECK(g.quantiles.empty() && g.keys.size() == 4);
    // whole files
    std::vector<uint64_t> counts;
    uint64_t n_lines = 0;
    Gorp::GroupQuantiles t = def->textGroupQuantiles(text, byVerb, ends_and_median, nullptr, &counts, &n_lines);
    CHECK(n_lines == lines.size() && (counts == std::vector<uint64_t>{1, 5, 4, 1, 0, 0, 0, 0}));
    CHECK((t.keys == std::vector<std::string>{"GET", "POST", "PUT", "HEAD"}) && row(t.at(0, 2), 77777, 4, 3, 1) && row(t.at(1, 1), 499, 2, 1, 2) && row(t.at(2, 1), 0, 0, 0, 0));
    printf("GPU checks ok\n");
    return 0;
}
