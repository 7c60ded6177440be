// Exercises captureStats(), textCaptureStats() and the Measures builder of include/gorp.hpp.
//   stats_api_test          : host-only checks (names resolve, refusals, no device is an error, never a CPU path) -- no GPU needed
//   stats_api_test --gpu    : also runs the calls on the device
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
    CHECK(sizeof(gx_measure_stats) == 64);

    // names resolve to (extraction, group); the edges stay with the builder
    Gorp::Measures took = def->measures();
    took.of("GetRequest", "timeTakenInMsec", {10, 100, 500, 1000}).of("PutRequest", "timeTakenInMsec").of(1, 1).of("GetRequest", "timeTakenInMsec", {500});
    const std::vector<gx_measure> m = took.measures();
    CHECK(m.size() == 4 && took.bins() == 5 + 1 + 1 + 2);
    CHECK(m[0].extraction == 1 && m[0].group == 2 && m[0].n_edges == 4 && m[0].edges[0] == 10 && m[0].edges[3] == 1000);
    CHECK(m[1].extraction == 0 && m[1].group == 2 && m[1].n_edges == 0 && m[1].edges == nullptr);
    CHECK(m[2].extraction == 1 && m[2].group == 1 && m[3].n_edges == 1 && m[3].edges[0] == 500);
    try { def->measures().of("Nobody", "path"); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->measures().of("GetRequest", "nothing"); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->measures().of(3, 0); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->measures().of(0, 4); CHECK(false); } catch (std::invalid_argument&) {}

    const std::vector<std::string> lines = {"[1]: GET 500ms /v1/a", "[2]: GET 499ms /v1/b", "[3]: PUT 900ms /v1/c", "nothing here", "[4]: POST 1ms /x",
                                            "[5]: GET 00501ms /v2/d", "[6]: HEAD 7ms /y", "[7]: GET 77777ms /v1/", "[8]: GET 99999999999999999999ms /v1/big"};
    std::string bytes, text;
    std::vector<uint32_t> off(1, 0);
    for (const std::string& ln : lines) { bytes += ln; text += ln + "\n"; off.push_back(static_cast<uint32_t>(bytes.size())); }
    const uint8_t* p = reinterpret_cast<const uint8_t*>(bytes.data());
    std::vector<int32_t> ids(lines.size(), -1), caps(lines.size() * 2 * static_cast<size_t>(def->maxGroups()), -1);
    Gorp::Where v1 = def->where();
    v1.on("GetRequest", "path").startsWith("/v1/");
    if (!gpu) {
        // refusals need no device ...
        try { def->captureStats(p, off.data(), lines.size(), ids.data(), nullptr, took); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }                                   // measures on dense ids without capture rows
        Gorp::Measures descending = def->measures();
        descending.of(0, 0, {5, 5});
        try { def->captureStats(p, off.data(), lines.size(), ids.data(), caps.data(), descending); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }
        Gorp::Measures many = def->measures();
        for (int q = 0; q < 65; ++q) many.of(0, 0);
        try { def->captureStats(p, off.data(), lines.size(), ids.data(), caps.data(), many); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_LIMIT); }
        Gorp::Measures wide = def->measures();
        wide.of(0, 0, std::vector<int64_t>(65, 0));
        try { def->textCaptureStats(text, wide); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_LIMIT); }
        // ... and behind them no device is an error, never a CPU path
        try { def->captureStats(p, off.data(), lines.size(), ids.data(), caps.data(), took, &v1); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        try { def->textCaptureStats(text, took); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        printf("host-only checks ok\n");
        return 0;
    }
    def->extractBatch(p, off.data(), lines.size(), ids.data(), caps.data());
    CHECK((ids == std::vector<int32_t>{1, 1, 0, -1, 2, 1, 2, 1, 1}));
    std::vector<Gorp::MeasureStats> s = def->captureStats(p, off.data(), lines.size(), ids.data(), caps.data(), took);
    CHECK(s.size() == 4);
    // GetRequest.timeTakenInMsec: 500, 499, 501, 77777 and a value beyond int64
    CHECK(s[0].stats.lines == 5 && s[0].stats.numbers == 4 && s[0].stats.unset == 0 && s[0].stats.not_numbers == 1);
    CHECK(s[0].stats.min == 499 && s[0].stats.max == 77777 && s[0].stats.sum_lo == 500 + 499 + 501 + 77777 && s[0].stats.sum_hi == 0);
    CHECK((s[0].hist == std::vector<uint64_t>{0, 0, 1, 2, 1}));
    CHECK(s[1].stats.lines == 1 && s[1].stats.min == 900 && s[1].stats.max == 900 && (s[1].hist == std::vector<uint64_t>{1}));
    CHECK(s[2].stats.lines == 5 && s[2].stats.numbers == 0 && s[2].stats.not_numbers == 5 && s[2].stats.min == INT64_MAX && s[2].stats.max == INT64_MIN);   // verb
    CHECK((s[3].hist == std::vector<uint64_t>{1, 3}) && s[3].stats.sum_lo == s[0].stats.sum_lo);
    // with terms: GetRequest's lines whose path starts with /v1/
    s = def->captureStats(p, off.data(), lines.size(), ids.data(), caps.data(), took, &v1);
    CHECK(s[0].stats.lines == 4 && s[0].stats.numbers == 3 && s[0].stats.sum_lo == 500 + 499 + 77777 && s[1].stats.lines == 1);
    // whole files
    std::vector<uint64_t> counts;
    uint64_t n_lines = 0;
    std::vector<Gorp::MeasureStats> t = def->textCaptureStats(text, took, &v1, &counts, &n_lines);
    CHECK(n_lines == lines.size() && (counts == std::vector<uint64_t>{1, 5, 2, 1, 0, 0, 0, 0}));
    CHECK(t.size() == 4 && memcmp(&t[0].stats, &s[0].stats, sizeof(gx_measure_stats)) == 0 && t[0].hist == s[0].hist && t[3].hist == s[3].hist);
    CHECK(def->textCaptureStats(text, def->measures(), nullptr, &counts, &n_lines).empty() && n_lines == lines.size() && counts[1] == 5);
    printf("GPU checks ok\n");
    return 0;
}
