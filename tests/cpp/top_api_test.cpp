// Exercises topLines(), textTopLines() and the TopParts builder of include/gorp.hpp.
//   top_api_test          : host-only checks (names resolve, refusals, no device is an error, never a CPU path) -- no GPU needed
//   top_api_test --gpu    : also runs the calls on the device
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
    CHECK(sizeof(gx_top_part) == 8 && sizeof(gx_top_totals) == 64 && GX_TOP_MAX_LINES >= 4096u);

    // names resolve to (extraction, group)
    Gorp::TopParts slow = def->topParts();
    slow.of("GetRequest", "timeTakenInMsec").of(2, 2);
    CHECK(slow.parts().size() == 2 && slow.parts()[0].extraction == 1 && slow.parts()[0].value_group == 2 && slow.parts()[1].extraction == 2);
    try { def->topParts().of("Nobody", "path"); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->topParts().of("GetRequest", "nothing"); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->topParts().of(3, 0); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->topParts().of(0, 4); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->topParts().of(1, 2).of("GetRequest", "path"); CHECK(false); } catch (std::invalid_argument&) {}

    const std::vector<std::string> lines = {"[1]: GET 500ms /v1/a", "[2]: GET 499ms /v1/b", "[3]: PUT 900ms /v1/c", "nothing here", "[4]: POST 501ms /x",
                                            "[5]: GET 00501ms /v2/d", "[6]: HEAD 7ms /y", "[7]: GET 77777ms /v1/", "[8]: GET 99999999999999999999ms /v1/big",
                                            "[9]: GET +501ms /v1/no"};
    std::string bytes, text;
    std::vector<uint32_t> off(1, 0);
    for (const std::string& ln : lines) { bytes += ln; text += ln + "\n"; off.push_back(static_cast<uint32_t>(bytes.size())); }
    const uint8_t* p = reinterpret_cast<const uint8_t*>(bytes.data());
    std::vector<int32_t> ids(lines.size(), -1), caps(lines.size() * 2 * static_cast<size_t>(def->maxGroups()), -1);
    Gorp::Where v1 = def->where();
    v1.on("GetRequest", "path").startsWith("/v1/");
    if (!gpu) {
        // refusals need no device ...
        try { def->topLines(p, off.data(), lines.size(), ids.data(), nullptr, slow, 3); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }                                   // parts on dense ids without capture rows
        try { def->topLines(p, off.data(), lines.size(), ids.data(), caps.data(), slow, GX_TOP_MAX_LINES + 1); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_LIMIT); }
        try { def->textTopLines(text, slow, GX_TOP_MAX_LINES + 1, false); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_LIMIT); }
        // ... and behind them no device is an error, never a CPU path
        try { def->topLines(p, off.data(), lines.size(), ids.data(), caps.data(), slow, 3, true, &v1); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        try { def->textTopLines(text, slow, 3); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        printf("host-only checks ok\n");
        return 0;
    }
    def->extractBatch(p, off.data(), lines.size(), ids.data(), caps.data());
    CHECK((ids == std::vector<int32_t>{1, 1, 0, -1, 2, 1, 2, 1, 1, -1}));
    // GetRequest and OtherRequest in one number space: 77777, then 501 twice (lines 4 and 5), 500, 499, 7; one value beyond int64
    Gorp::Top t = def->topLines(p, off.data(), lines.size(), ids.data(), caps.data(), slow, 3);
    CHECK((t.index == std::vector<uint32_t>{7, 4, 5}) && (t.values == std::vector<int64_t>{77777, 501, 501}));
    CHECK(t.totals.lines == 7 && t.totals.numbers == 6 && t.totals.not_numbers == 1 && t.totals.unset == 0 && t.totals.n_top == 3);
    CHECK(t.totals.last_value == 501 && t.totals.ties_left == 0);
    CHECK(std::string(t.bytes.begin(), t.bytes.end()) == lines[7] + lines[4] + lines[5]);
    CHECK((t.offsets == std::vector<uint32_t>{0, static_cast<uint32_t>(lines[7].size()), static_cast<uint32_t>(lines[7].size() + lines[4].size()),
                                              static_cast<uint32_t>(t.bytes.size())}));
    t = def->topLines(p, off.data(), lines.size(), ids.data(), caps.data(), slow, 2);
    CHECK((t.index == std::vector<uint32_t>{7, 4}) && t.totals.ties_left == 1);           // the tie at the cut goes to the earlier line
    t = def->topLines(p, off.data(), lines.size(), ids.data(), caps.data(), slow, 2, false);
    CHECK((t.index == std::vector<uint32_t>{6, 1}) && (t.values == std::vector<int64_t>{7, 499}));
    t = def->topLines(p, off.data(), lines.size(), ids.data(), caps.data(), slow, 100, true, &v1);   // GetRequest's lines under /v1/, and OtherRequest's
    CHECK((t.index == std::vector<uint32_t>{7, 4, 0, 1, 6}) && t.totals.n_top == 5 && t.totals.not_numbers == 1);
    CHECK(def->topLines(p, off.data(), lines.size(), ids.data(), caps.data(), def->topParts(), 5).index.empty());
    // whole files
    std::vector<uint64_t> counts;
    uint64_t n_lines = 0;
    Gorp::Top w = def->textTopLines(text, slow, 3, true, nullptr, &counts, &n_lines);
    CHECK(n_lines == lines.size() && (counts == std::vector<uint64_t>{1, 5, 2, 2, 0, 0, 0, 0}));
    CHECK((w.index == std::vector<uint32_t>{7, 4, 5}) && (w.values == std::vector<int64_t>{77777, 501, 501}) && w.totals.n_top == 3);
    CHECK(std::string(w.bytes.begin(), w.bytes.end()) == lines[7] + "\n" + lines[4] + "\n" + lines[5] + "\n");
    printf("GPU checks ok\n");
    return 0;
}
