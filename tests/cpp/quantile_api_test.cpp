// Exercises captureQuantiles() and textCaptureQuantiles() of include/gorp.hpp, with the TopParts builder reused.
//   quantile_api_test          : host-only checks (refusals, no device is an error, never a CPU path) -- no GPU needed
//   quantile_api_test --gpu    : also runs the calls on the device
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
    CHECK(sizeof(gx_quantile) == 8 && sizeof(gx_quantile_out) == 32 && sizeof(gx_quantile_totals) == 32 && GX_QUANTILE_MAX == 16u);

    Gorp::TopParts slow = def->topParts();
    slow.of("GetRequest", "timeTakenInMsec").of(2, 2);
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
    const std::vector<gx_quantile> ends_and_median = {{0, 1}, {1, 2}, {1, 1}, {1, 2}};
    if (!gpu) {
        // refusals need no device ...
        try { def->captureQuantiles(p, off.data(), lines.size(), ids.data(), nullptr, slow, ends_and_median); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }                                   // parts on dense ids without capture rows
        try { def->captureQuantiles(p, off.data(), lines.size(), ids.data(), caps.data(), slow, {{1, 0}}); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }                                   // den == 0
        try { def->textCaptureQuantiles(text, slow, {{3, 2}}); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }                                   // num > den
        try { def->captureQuantiles(p, off.data(), lines.size(), ids.data(), caps.data(), slow, std::vector<gx_quantile>(GX_QUANTILE_MAX + 1, gx_quantile{1, 2})); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_LIMIT); }
        try { def->textCaptureQuantiles(text, slow, std::vector<gx_quantile>(GX_QUANTILE_MAX + 1, gx_quantile{1, 2})); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_LIMIT); }
        // ... and behind them no device is an error, never a CPU path
        try { def->captureQuantiles(p, off.data(), lines.size(), ids.data(), caps.data(), slow, ends_and_median, &v1); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        try { def->textCaptureQuantiles(text, slow, {}); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        printf("host-only checks ok\n");
        return 0;
    }
    def->extractBatch(p, off.data(), lines.size(), ids.data(), caps.data());
    CHECK((ids == std::vector<int32_t>{1, 1, 0, -1, 2, 1, 2, 1, 1, -1}));
    // GetRequest and OtherRequest in one number space: 7, 499, 500, 501, 501, 77777; one value beyond int64
    Gorp::Quantiles q = def->captureQuantiles(p, off.data(), lines.size(), ids.data(), caps.data(), slow, ends_and_median);
    CHECK(q.totals.lines == 7 && q.totals.numbers == 6 && q.totals.not_numbers == 1 && q.totals.unset == 0 && q.out.size() == 4);
    CHECK(row(q.out[0], 7, 1, 0, 1) && row(q.out[1], 500, 3, 2, 1) && row(q.out[2], 77777, 6, 5, 1) && row(q.out[3], 500, 3, 2, 1));
    q = def->captureQuantiles(p, off.data(), lines.size(), ids.data(), caps.data(), slow, {{2, 3}, {5, 6}});   // ranks 4 and 5: the two 501s
    CHECK(row(q.out[0], 501, 4, 3, 2) && row(q.out[1], 501, 5, 3, 2));
    q = def->captureQuantiles(p, off.data(), lines.size(), ids.data(), caps.data(), slow, ends_and_median, &v1);   // GetRequest's lines under /v1/, and OtherRequest's
    CHECK(q.totals.numbers == 5 && q.totals.not_numbers == 1 && row(q.out[1], 500, 3, 2, 1) && row(q.out[2], 77777, 5, 4, 1));
    q = def->captureQuantiles(p, off.data(), lines.size(), ids.data(), caps.data(), def->topParts(), ends_and_median);
    CHECK(q.totals.lines == 0 && row(q.out[0], 0, 0, 0, 0) && row(q.out[3], 0, 0, 0, 0));
    q = def->captureQuantiles(p, off.data(), lines.size(), ids.data(), caps.data(), slow, {});
    CHECK(q.out.empty() && q.totals.numbers == 6);
    // whole files
    std::vector<uint64_t> counts;
    uint64_t n_lines = 0;
    Gorp::Quantiles w = def->textCaptureQuantiles(text, slow, ends_and_median, nullptr, &counts, &n_lines);
    CHECK(n_lines == lines.size() && (counts == std::vector<uint64_t>{1, 5, 2, 2, 0, 0, 0, 0}));
    CHECK(w.totals.numbers == 6 && row(w.out[0], 7, 1, 0, 1) && row(w.out[1], 500, 3, 2, 1) && row(w.out[2], 77777, 6, 5, 1));
    printf("GPU checks ok\n");
    return 0;
}
