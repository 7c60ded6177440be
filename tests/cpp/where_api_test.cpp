// Exercises selectLinesWhere() and the Where builder of include/gorp.hpp.
//   where_api_test          : host-only checks (names resolve, refusals, no device is an error, never a CPU path) -- no GPU needed
//   where_api_test --gpu    : also runs the call on the device
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
    typedef Gorp::Want Want;

    // names resolve to (extraction, group); the default mask marks the extractions that have terms
    Gorp::Where slow = def->where();
    slow.on("GetRequest", "timeTakenInMsec").ge(500).on("OtherRequest", "verb").eq("POST").ne("HEAD").on("GetRequest", "path").contains("/v1/").isSet();
    const std::vector<gx_where_term> t = slow.terms();
    CHECK(t.size() == 5);
    CHECK(t[0].extraction == 1 && t[0].group == 2 && t[0].op == GX_WHERE_INT_GE && t[0].negate == 0 && t[0].number == 500 && t[0].text == nullptr);
    CHECK(t[1].extraction == 2 && t[1].group == 1 && t[1].op == GX_WHERE_EQ && t[1].negate == 0 && t[1].text_units == 4 && memcmp(t[1].text, "POST", 4) == 0);
    CHECK(t[2].op == GX_WHERE_EQ && t[2].negate == 1 && memcmp(t[2].text, "HEAD", 4) == 0);
    CHECK(t[3].extraction == 1 && t[3].group == 3 && t[3].op == GX_WHERE_CONTAINS && t[3].text_units == 4);
    CHECK(t[4].op == GX_WHERE_SET && t[4].group == 3 && t[4].text == nullptr && t[4].text_units == 0);
    CHECK(slow.want() == (Want{0, 1, 1, 0, 0, 0, 0}));
    CHECK(def->where().want() == (Want{0, 0, 0, 0, 0, 0, 0}));
    CHECK(def->where().on(0, 3).isUnset().lt(-1).le(0).gt(1).eq(int64_t(7)).ne(int64_t(8)).startsWith("a").endsWith("").notContains("b").terms().size() == 9);
    try { def->where().on("Nobody", "path"); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->where().on("GetRequest", "nothing"); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->where().on(3, 0); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->where().on(0, 4); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->where().ge(1); CHECK(false); } catch (std::invalid_argument&) {}

    const std::vector<std::string> lines = {"[1]: GET 500ms /v1/a", "[2]: GET 499ms /v1/b", "[3]: PUT 900ms /v1/c", "nothing here", "[4]: POST 1ms /x",
                                            "[5]: GET 00501ms /v2/d", "[6]: HEAD 7ms /y", "[7]: GET 77777ms /v1/"};
    std::string bytes;
    std::vector<uint32_t> off(1, 0);
    for (const std::string& ln : lines) { bytes += ln; off.push_back(static_cast<uint32_t>(bytes.size())); }
    const uint8_t* p = reinterpret_cast<const uint8_t*>(bytes.data());
    std::vector<int32_t> ids(lines.size(), -1), caps(lines.size() * 2 * static_cast<size_t>(def->maxGroups()), -1);
    if (!gpu) {
        // refusals need no device ...
        try { def->selectLinesWhere(p, off.data(), lines.size(), ids.data(), nullptr, slow.want(), slow); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }                                   // terms on dense ids without capture rows
        try { def->selectLinesWhere(p, off.data(), lines.size(), ids.data(), caps.data(), Want{1}, slow); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }
        Gorp::Where many = def->where();
        many.on(0, 0);
        for (int q = 0; q < 65; ++q) many.isSet();
        try { def->selectLinesWhere(p, off.data(), lines.size(), ids.data(), caps.data(), many.want(), many); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_LIMIT); }
        Gorp::Where longText = def->where();
        longText.on(0, 0).eq(std::string(256, 'x'));
        try { def->selectLinesWhere(p, off.data(), lines.size(), ids.data(), caps.data(), longText.want(), longText); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_LIMIT); }
        // ... and behind them no device is an error, never a CPU path
        try { def->selectLinesWhere(p, off.data(), lines.size(), ids.data(), caps.data(), slow.want(), slow); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        printf("host-only checks ok\n");
        return 0;
    }
    def->extractBatch(p, off.data(), lines.size(), ids.data(), caps.data());
    CHECK((ids == std::vector<int32_t>{1, 1, 0, -1, 2, 1, 2, 1}));
    // GetRequest: timeTakenInMsec >= 500 and path contains "/v1/"; OtherRequest: verb == POST and != HEAD; PutRequest is not wanted
    Gorp::Selection s = def->selectLinesWhere(p, off.data(), lines.size(), ids.data(), caps.data(), slow.want(), slow);
    CHECK((s.index == std::vector<uint32_t>{0, 4, 7}));
    CHECK(std::string(s.bytes.begin(), s.bytes.end()) == lines[0] + lines[4] + lines[7]);
    CHECK((s.offsets == std::vector<uint32_t>{0, 20, 36, 57}));
    // want decides what has no terms: PutRequest's lines and the unmatched ones come along
    Want w = slow.want();
    w[0] = 1; w[3] = 1;
    s = def->selectLinesWhere(p, off.data(), lines.size(), ids.data(), caps.data(), w, slow);
    CHECK((s.index == std::vector<uint32_t>{0, 2, 3, 4, 7}));
    // no terms: selectLines
    Gorp::Selection a = def->selectLinesWhere(p, off.data(), lines.size(), ids.data(), caps.data(), w, def->where());
    Gorp::Selection b = def->selectLines(p, off.data(), lines.size(), ids.data(), w);
    CHECK(a.index == b.index && a.bytes == b.bytes && a.offsets == b.offsets && a.index.size() == 8);
    Gorp::Where fast = def->where();
    fast.on("GetRequest", "timeTakenInMsec").lt(500);
    s = def->selectLinesWhere(p, off.data(), lines.size(), ids.data(), caps.data(), fast.want(), fast);
    CHECK((s.index == std::vector<uint32_t>{1}));
    printf("GPU checks ok\n");
    return 0;
}
