// Exercises sortLines() and textSortLines() of include/gorp.hpp, with the TopParts builder reused.
//   sort_api_test          : host-only checks (refusals, no device is an error, never a CPU path) -- no GPU needed
//   sort_api_test --gpu    : also runs the calls on the device
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

    Gorp::TopParts byTime = def->topParts();
    byTime.of("GetRequest", "timeTakenInMsec").of("PutRequest", "timeTakenInMsec").of("OtherRequest", "timeTakenInMsec");
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
        try { def->sortLines(b, off.data(), lines.size(), ids.data(), nullptr, byTime); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }                                   // parts on dense ids without capture rows
        gx_top_part twice[2] = {{0, 0}, {0, 1}};
        gx_sort_totals totals{};
        CHECK(gx_sort_lines(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), twice, 2, nullptr, 0, 0, nullptr, &totals, nullptr) == GX_E_ARG);
        CHECK(gx_sort_lines(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), twice, 1, nullptr, 0, 16u, nullptr, &totals, nullptr) == GX_E_ARG);
        CHECK(gx_sort_lines(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), twice, 1, nullptr, 0, 0, nullptr, nullptr, nullptr) == GX_E_ARG);
        CHECK(gx_text_sort_lines(def->handle(), reinterpret_cast<const uint8_t*>(text.data()), text.size(), twice, 2, nullptr, 0, 0, nullptr, 0, nullptr, nullptr, nullptr,
                                 nullptr, &totals, nullptr, nullptr, nullptr) == GX_E_ARG);
        gx_sort_out into{};
        into.out_ids = ids.data();                                                             // an output that is an input
        into.cap_lines = lines.size();
        CHECK(gx_sort_lines(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), twice, 1, nullptr, 0, 0, &into, &totals, nullptr) == GX_E_ARG);
        CHECK(gx_sort_lines(def->handle(), b, off.data(), (1ull << 30) + 1, ids.data(), caps.data(), twice, 1, nullptr, 0, 0, nullptr, &totals, nullptr) == GX_E_LIMIT);
        // ... and behind them no device is an error, never a CPU path
        try { def->sortLines(b, off.data(), lines.size(), ids.data(), caps.data(), byTime, true, true, true, &v1); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        try { def->textSortLines(text, byTime, false, true); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        CHECK(gx_sort_lines(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), twice, 1, nullptr, 0,
                            GX_SORT_DESCENDING | GX_SORT_CARRY | GX_SORT_REST_LAST | GX_SORT_ALL_DIGITS, nullptr, &totals, nullptr) == GX_E_DEVICE);
        CHECK(Gorp::sortFlags(true, false, true) == (GX_SORT_DESCENDING | GX_SORT_REST_LAST));
        printf("host-only checks ok\n");
        return 0;
    }
    def->extractBatch(b, off.data(), lines.size(), ids.data(), caps.data());
    CHECK((ids == std::vector<int32_t>{1, 2, 0, -1, 2, 1, 2, 1, 1, 1, 2}));
    const size_t slots = 2 * static_cast<size_t>(def->maxGroups());
    // by time taken, ascending: 1 7 499 499 500 500 501 900 77777; line 3 matches nothing and line 8's value is no number: dropped
    Gorp::Sorted s = def->sortLines(b, off.data(), lines.size(), ids.data(), caps.data(), byTime);
    CHECK((s.index == std::vector<uint32_t>{4, 6, 1, 10, 0, 9, 5, 2, 7}) && (s.values == std::vector<int64_t>{1, 7, 499, 499, 500, 500, 501, 900, 77777}));
    CHECK(s.totals.lines == 10 && s.totals.numbers == 9 && s.totals.not_numbers == 1 && s.totals.unset == 0 && s.totals.carried == 0 && s.totals.rest == 2);
    CHECK(s.totals.lines_out == 9 && s.totals.first_value == 1 && s.totals.last_value == 77777 && s.totals.already_ordered == 0 && s.totals.n_passes == 3);
    CHECK((s.lineClass == std::vector<uint8_t>(9, 0)) && s.offsets.size() == 10 && s.offsets[9] == s.bytes.size() && s.totals.units_out == s.bytes.size());
    for (size_t j = 0; j < s.index.size(); ++j) {
        CHECK(std::string(s.bytes.begin() + s.offsets[j], s.bytes.begin() + s.offsets[j + 1]) == lines[s.index[j]]);
        CHECK(s.ids[j] == ids[s.index[j]] && std::equal(s.caps.begin() + j * slots, s.caps.begin() + (j + 1) * slots, caps.begin() + s.index[j] * slots));
    }
    // carried: line 3 travels with line 2 (900), line 8 with line 7 (77777)
    s = def->sortLines(b, off.data(), lines.size(), ids.data(), caps.data(), byTime, false, true);
    CHECK((s.index == std::vector<uint32_t>{4, 6, 1, 10, 0, 9, 5, 2, 3, 7, 8}) && (s.lineClass == std::vector<uint8_t>{0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1}));
    CHECK(s.values[8] == 900 && s.values[10] == 77777 && s.totals.carried == 2 && s.totals.rest == 0 && s.totals.units_out == bytes.size());
    // descending keeps a record in order; ties still go by input line
    s = def->sortLines(b, off.data(), lines.size(), ids.data(), caps.data(), byTime, true, true, true);
    CHECK((s.index == std::vector<uint32_t>{7, 8, 2, 3, 5, 0, 9, 1, 10, 6, 4}) && s.totals.first_value == 77777 && s.totals.last_value == 1);
    // under a term GetRequest's lines outside /v1/ are not stamped: line 5 is a rest line, delivered last with value 0
    s = def->sortLines(b, off.data(), lines.size(), ids.data(), caps.data(), byTime, false, false, true, &v1);
    CHECK((s.index == std::vector<uint32_t>{4, 6, 1, 10, 0, 9, 2, 7, 3, 5, 8}) && s.totals.rest == 3 && s.values[9] == 0 && s.lineClass[9] == 2 && s.totals.lines == 9);
    // whole files
    std::vector<uint64_t> counts;
    uint64_t n_lines = 0;
    Gorp::Sorted t = def->textSortLines(text, byTime, false, true, false, nullptr, &counts, &n_lines);
    CHECK(n_lines == lines.size() && (counts == std::vector<uint64_t>{1, 5, 4, 1, 0, 0, 0, 0}));
    CHECK((t.index == std::vector<uint32_t>{4, 6, 1, 10, 0, 9, 5, 2, 3, 7, 8}) && t.ids.empty() && t.totals.carried == 2);
    for (size_t j = 0; j < t.index.size(); ++j) CHECK(std::string(t.bytes.begin() + t.offsets[j], t.bytes.begin() + t.offsets[j + 1]) == lines[t.index[j]] + "\n");
    printf("GPU checks ok\n");
    return 0;
}
