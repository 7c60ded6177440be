// Exercises groupLines(), textGroupLines() and the GroupParts builder of include/gorp.hpp.
//   group_api_test          : host-only checks (names resolve, refusals, no device is an error, never a CPU path) -- no GPU needed
//   group_api_test --gpu    : also runs the calls on the device
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
    CHECK(sizeof(gx_group_part) == 16 && sizeof(gx_group_out) == 64 && sizeof(gx_group_totals) == 48);

    // names resolve to (extraction, key group, value group)
    Gorp::GroupParts byVerb = def->groupParts();
    byVerb.of("GetRequest", "verb", "timeTakenInMsec").of("PutRequest", "verb").of(2, 1, 2);
    const std::vector<gx_group_part>& p = byVerb.parts();
    CHECK(p.size() == 3 && byVerb.hasValues());
    CHECK(p[0].extraction == 1 && p[0].key_group == 1 && p[0].value_group == 2 && p[0].reserved == 0);
    CHECK(p[1].extraction == 0 && p[1].key_group == 1 && p[1].value_group == -1);
    CHECK(p[2].extraction == 2 && p[2].key_group == 1 && p[2].value_group == 2);
    CHECK(!def->groupParts().of("GetRequest", "path").hasValues());
    try { def->groupParts().of("Nobody", "path"); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->groupParts().of("GetRequest", "nothing"); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->groupParts().of("GetRequest", "verb", "nothing"); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->groupParts().of(3, 0); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->groupParts().of(0, 4); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->groupParts().of(0, 1, 4); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->groupParts().of("GetRequest", "verb").of(1, 3); CHECK(false); } catch (std::invalid_argument&) {}   // two parts for one extraction

    const std::vector<std::string> lines = {"[1]: GET 500ms /v1/a", "[2]: POST 499ms /v1/b", "[3]: PUT 900ms /v1/a", "nothing here", "[4]: POST 1ms /x",
                                            "[5]: GET 00501ms /v2/d", "[6]: HEAD 7ms /v1/a", "[7]: GET 77777ms /v1/", "[8]: GET 99999999999999999999ms /v1/a"};
    std::string bytes, text;
    std::vector<uint32_t> off(1, 0);
    for (const std::string& ln : lines) { bytes += ln; text += ln + "\n"; off.push_back(static_cast<uint32_t>(bytes.size())); }
    const uint8_t* b = reinterpret_cast<const uint8_t*>(bytes.data());
    std::vector<int32_t> ids(lines.size(), -1), caps(lines.size() * 2 * static_cast<size_t>(def->maxGroups()), -1);
    Gorp::Where v1 = def->where();
    v1.on("GetRequest", "path").startsWith("/v1/");
    if (!gpu) {
        // refusals need no device ...
        try { def->groupLines(b, off.data(), lines.size(), ids.data(), nullptr, byVerb); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }                                   // parts on dense ids without capture rows
        gx_group_part twice[2] = {{0, 0, -1, 0}, {0, 1, -1, 0}};
        gx_group_totals totals{};
        CHECK(gx_group_lines(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), twice, 2, nullptr, 0, 0, nullptr, &totals, nullptr) == GX_E_ARG);
        CHECK(gx_group_lines(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), twice, 1, nullptr, 0, 2, nullptr, &totals, nullptr) == GX_E_ARG);
        // ... and behind them no device is an error, never a CPU path
        try { def->groupLines(b, off.data(), lines.size(), ids.data(), caps.data(), byVerb, &v1); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        try { def->textGroupLines(text, byVerb); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        printf("host-only checks ok\n");
        return 0;
    }
    def->extractBatch(b, off.data(), lines.size(), ids.data(), caps.data());
    CHECK((ids == std::vector<int32_t>{1, 2, 0, -1, 2, 1, 2, 1, 1}));
    Gorp::Groups g = def->groupLines(b, off.data(), lines.size(), ids.data(), caps.data(), byVerb);
    // in order of appearance: GET (lines 0, 5, 7, 8), POST (1, 4), PUT (2), HEAD (6)
    CHECK((g.keys == std::vector<std::string>{"GET", "POST", "PUT", "HEAD"}) && (g.firstLine == std::vector<uint32_t>{0, 1, 2, 6}));
    CHECK((g.lines == std::vector<uint64_t>{4, 2, 1, 1}) && (g.lineKey == std::vector<uint32_t>{0, 1, 2, 0xFFFFFFFFu, 1, 0, 3, 0, 0}));
    CHECK(g.totals.n_keys == 4 && g.totals.key_units == 14 && g.totals.lines == 8 && g.totals.keyed == 8 && g.totals.unset == 0 && g.totals.exact == 1);
    // GET's numbers: 500, 501, 77777 and a value beyond int64; PUT's part only counts
    CHECK(g.stats.size() == 4 && g.stats[0].lines == 4 && g.stats[0].numbers == 3 && g.stats[0].not_numbers == 1 && g.stats[0].min == 500 && g.stats[0].max == 77777);
    CHECK(g.stats[0].sum_lo == 500 + 501 + 77777 && g.stats[0].sum_hi == 0 && g.stats[1].sum_lo == 500 && g.stats[1].min == 1);
    CHECK(g.stats[2].lines == 0 && g.stats[2].min == INT64_MAX && g.stats[2].max == INT64_MIN && g.stats[3].sum_lo == 7);
    // keyed by path, with terms: GetRequest's lines whose path starts with /v1/, and every PutRequest line
    Gorp::GroupParts byPath = def->groupParts();
    byPath.of("GetRequest", "path").of("PutRequest", "path");
    g = def->groupLines(b, off.data(), lines.size(), ids.data(), caps.data(), byPath, &v1);
    CHECK((g.keys == std::vector<std::string>{"/v1/a", "/v1/"}) && (g.lines == std::vector<uint64_t>{3, 1}) && g.stats.empty() && g.totals.lines == 4);
    // whole files
    std::vector<uint64_t> counts;
    uint64_t n_lines = 0;
    Gorp::Groups t = def->textGroupLines(text, byPath, &v1, &counts, &n_lines);
    CHECK(n_lines == lines.size() && (counts == std::vector<uint64_t>{1, 4, 3, 1, 0, 0, 0, 0}));
    CHECK(t.keys == g.keys && t.lines == g.lines && t.firstLine == g.firstLine && t.lineKey == g.lineKey);
    CHECK(def->textGroupLines(text, def->groupParts(), nullptr, &counts, &n_lines).keys.empty() && n_lines == lines.size() && counts[1] == 4);
    // more keys than the first size query's table takes (1 024 keys, 2 048 slots): the table overflows, the query is asked again with
    // the number of lines, and the groups are the same as ever; the vectors are sized by lines and keys, not by the text's bytes
    std::string many;
    const size_t distinct = 3000;
    for (size_t r = 0; r < 2; ++r)
        for (size_t j = 0; j < distinct; ++j) many += "[1]: GET " + std::to_string(j % 7) + "ms /p/" + std::to_string(j * 31) + "\n";
    t = def->textGroupLines(many, byPath, nullptr, &counts, &n_lines);
    CHECK(n_lines == 2 * distinct && t.keys.size() == distinct && t.lineKey.size() == 2 * distinct && t.totals.exact == 1 && t.totals.n_keys == distinct);
    CHECK(t.keys[0] == "/p/0" && t.keys[distinct - 1] == "/p/" + std::to_string((distinct - 1) * 31) && t.lines[17] == 2 && t.firstLine[distinct - 1] == distinct - 1);
    CHECK(t.lineKey[distinct + 5] == 5 && t.lineKey[2 * distinct - 1] == distinct - 1);
    std::vector<uint32_t> moff(1, 0);
    std::string mbytes;
    for (size_t at = 0; at < many.size();) {
        const size_t nl = many.find('\n', at);
        mbytes += many.substr(at, nl - at);
        moff.push_back(static_cast<uint32_t>(mbytes.size()));
        at = nl + 1;
    }
    std::vector<int32_t> mids(moff.size() - 1, -1), mcaps((moff.size() - 1) * 2 * static_cast<size_t>(def->maxGroups()), -1);
    def->extractBatch(reinterpret_cast<const uint8_t*>(mbytes.data()), moff.data(), mids.size(), mids.data(), mcaps.data());
    g = def->groupLines(reinterpret_cast<const uint8_t*>(mbytes.data()), moff.data(), mids.size(), mids.data(), mcaps.data(), byPath);
    CHECK(g.keys == t.keys && g.lines == t.lines && g.lineKey == t.lineKey && g.firstLine == t.firstLine);
    printf("GPU checks ok\n");
    return 0;
}
