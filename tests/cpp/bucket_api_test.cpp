// Exercises bucketLines() and textBucketLines() of include/gorp.hpp, with the BucketParts builder, and the C ABI's refusals.
//   bucket_api_test          : host-only checks (refusals, no device is an error, never a CPU path) -- no GPU needed
//   bucket_api_test --gpu    : also runs the calls on the device
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

    Gorp::BucketParts perMinute = def->bucketParts();
    perMinute.of("GetRequest", "timestamp", "timeTakenInMsec").of("PutRequest", "timestamp").of(2, 0, 2);
    const std::vector<gx_bucket_part> pp = perMinute.parts();
    CHECK(pp.size() == 3 && perMinute.hasValues() && pp[0].extraction == 1 && pp[0].number_group == 0 && pp[0].value_group == 2 && pp[1].value_group == -1 &&
          pp[2].extraction == 2 && pp[2].reserved == 0);
    try { def->bucketParts().of("GetRequest", "nothing"); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->bucketParts().of(0, 4); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->bucketParts().of(0, 0, -2); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->bucketParts().of("GetRequest", "timestamp").of("GetRequest", "timeTakenInMsec"); CHECK(false); } catch (std::invalid_argument&) {}
    const std::vector<std::string> lines = {"[130]: GET 500ms /v1/a", "[119]: POST 499ms /v1/b", "[60]: PUT 900ms /v1/a", "nothing here", "[59]: POST 1ms /x",
                                            "[121]: GET 00501ms /v2/d", "[0]: HEAD 7ms /v1/a", "[179]: GET 77777ms /v1/", "[120]: GET 99999999999999999999ms /v1/a",
                                            "[99999999999999999999]: GET 500ms /v1/z", "[61]: POST 499ms /v1/b"};
    std::string bytes, text;
    std::vector<uint32_t> off(1, 0);
    for (const std::string& ln : lines) { bytes += ln; text += ln + "\n"; off.push_back(static_cast<uint32_t>(bytes.size())); }
    const uint8_t* b = reinterpret_cast<const uint8_t*>(bytes.data());
    std::vector<int32_t> ids(lines.size(), -1), caps(lines.size() * 2 * static_cast<size_t>(def->maxGroups()), -1);
    Gorp::Where v1 = def->where();
    v1.on("GetRequest", "path").startsWith("/v1/");
    if (!gpu) {
        // refusals need no device ...
        try { def->bucketLines(b, off.data(), lines.size(), ids.data(), nullptr, perMinute, 60); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }                                   // parts on dense ids without capture rows
        try { def->bucketLines(b, off.data(), lines.size(), ids.data(), caps.data(), perMinute, 0); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG && std::string(e.what()).find("width") != std::string::npos); }
        gx_bucket_part one[2] = {{0, 0, -1, 0}, {1, 0, -1, 0}}, twice[2] = {{0, 0, -1, 0}, {0, 0, -1, 0}}, reserved[1] = {{0, 0, -1, 1}}, group[1] = {{0, 4, -1, 0}};
        gx_bucket_totals totals{};
        gx_bucket_out into{};
        std::vector<uint32_t> line_bucket(lines.size());
        std::vector<gx_measure_stats> stats(lines.size());
        into.line_bucket = line_bucket.data();
        into.max_buckets = lines.size();
        const uint8_t* t8 = reinterpret_cast<const uint8_t*>(text.data());
        gx_handle* h = def->handle();
        const uint64_t n = lines.size();
        CHECK(gx_bucket_lines(h, b, off.data(), n, ids.data(), caps.data(), one, 2, 0, 0, nullptr, 0, 0, &into, &totals, nullptr) == GX_E_ARG);            // width < 1
        CHECK(gx_bucket_lines(h, b, off.data(), n, ids.data(), caps.data(), one, 2, 0, -60, nullptr, 0, 0, &into, &totals, nullptr) == GX_E_ARG);
        CHECK(gx_bucket_lines(h, b, off.data(), n, ids.data(), caps.data(), one, 2, 0, 60, nullptr, 0, 4, &into, &totals, nullptr) == GX_E_ARG);           // unknown flag bits
        CHECK(gx_bucket_lines(h, b, off.data(), n, ids.data(), caps.data(), one, 2, 0, 60, nullptr, 0, 0, &into, nullptr, nullptr) == GX_E_ARG);           // totals == NULL
        CHECK(gx_bucket_lines(h, b, off.data(), n, ids.data(), caps.data(), nullptr, 2, 0, 60, nullptr, 0, 0, &into, &totals, nullptr) == GX_E_ARG);
        CHECK(gx_bucket_lines(h, b, off.data(), n, ids.data(), caps.data(), twice, 2, 0, 60, nullptr, 0, 0, &into, &totals, nullptr) == GX_E_ARG);
        CHECK(gx_bucket_lines(h, b, off.data(), n, ids.data(), caps.data(), reserved, 1, 0, 60, nullptr, 0, 0, &into, &totals, nullptr) == GX_E_ARG);
        CHECK(gx_bucket_lines(h, b, off.data(), n, ids.data(), caps.data(), group, 1, 0, 60, nullptr, 0, 0, &into, &totals, nullptr) == GX_E_ARG);
        into.bucket_stats = stats.data();
        CHECK(gx_bucket_lines(h, b, off.data(), n, ids.data(), caps.data(), one, 2, 0, 60, nullptr, 0, 0, &into, &totals, nullptr) == GX_E_ARG);           // stats, no value_group
        CHECK(gx_text_bucket_lines(h, t8, text.size(), one, 2, 0, 60, nullptr, 0, 0, &into, &totals, nullptr, nullptr, nullptr) == GX_E_ARG);
        into.bucket_stats = nullptr;
        gx_batch_opts o{};
        o.struct_size = sizeof(o);
        o.no_sync = 1;
        CHECK(gx_bucket_lines(h, b, off.data(), n, ids.data(), caps.data(), one, 2, 0, 60, nullptr, 0, 0, &into, &totals, &o) == GX_E_ARG);
        o.no_sync = 0;
        o.utf8 = 2;
        CHECK(gx_bucket_lines(h, b, off.data(), n, ids.data(), caps.data(), one, 2, 0, 60, nullptr, 0, 0, &into, &totals, &o) == GX_E_ARG);
        into.max_buckets = (1ull << 30) + 1;
        CHECK(gx_bucket_lines(h, b, off.data(), n, ids.data(), caps.data(), one, 2, 0, 60, nullptr, 0, 0, &into, &totals, nullptr) == GX_E_LIMIT);
        CHECK(gx_text_bucket_lines(h, t8, text.size(), one, 2, 0, 60, nullptr, 0, 0, &into, &totals, nullptr, nullptr, nullptr) == GX_E_LIMIT);
        into.max_buckets = n;
        CHECK(gx_bucket_lines(h, b, off.data(), 0xFFFFFFFFull, ids.data(), caps.data(), one, 2, 0, 60, nullptr, 0, 0, &into, &totals, nullptr) == GX_E_LIMIT);
        CHECK(gx_text_bucket_lines(h, t8, text.size(), one, 2, 0, 0, nullptr, 0, 0, nullptr, &totals, nullptr, nullptr, nullptr) == GX_E_ARG);
        // ... and behind them no device is an error, never a CPU path
        CHECK(gx_bucket_lines(h, b, off.data(), n, ids.data(), caps.data(), one, 2, -5, 60, nullptr, 0, GX_GROUP_WEAK_HASH | GX_BUCKET_ALL_DIGITS, &into, &totals,
                              nullptr) == GX_E_DEVICE);
        CHECK(gx_bucket_lines(h, b, off.data(), n, ids.data(), caps.data(), one, 2, 0, 1, nullptr, 0, 0, nullptr, &totals, nullptr) == GX_E_DEVICE);
        CHECK(gx_text_bucket_lines(h, t8, text.size(), one, 2, 0, 60, nullptr, 0, 0, nullptr, &totals, nullptr, nullptr, nullptr) == GX_E_DEVICE);
        try { def->bucketLines(b, off.data(), lines.size(), ids.data(), caps.data(), perMinute, 60, 0, &v1); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        try { def->textBucketLines(text, perMinute, 60); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        printf("host-only checks ok\n");
        return 0;
    }
    def->extractBatch(b, off.data(), lines.size(), ids.data(), caps.data());
    CHECK((ids == std::vector<int32_t>{1, 2, 0, -1, 2, 1, 2, 1, 1, 1, 2}));
    // per 60 from origin 60: 130 -> 1, 119 -> 0, 60 -> 0, 59 -> -1, 121 -> 1, 0 -> -1, 179 -> 1, 120 -> 1, 10^20 -> no number, 61 -> 0
    Gorp::Buckets g = def->bucketLines(b, off.data(), lines.size(), ids.data(), caps.data(), perMinute, 60, 60);
    CHECK((g.bucketNumber == std::vector<int64_t>{-1, 0, 1}) && (g.lines == std::vector<uint64_t>{2, 3, 4}) && (g.firstLine == std::vector<uint32_t>{4, 1, 0}));
    CHECK((g.lineBucket == std::vector<uint32_t>{2, 1, 1, 0xFFFFFFFFu, 0, 2, 0, 2, 2, 0xFFFFFFFFu, 1}));
    CHECK(g.totals.n_buckets == 3 && g.totals.lines == 10 && g.totals.bucketed == 9 && g.totals.not_numbers == 1 && g.totals.unset == 0 && g.totals.out_of_range == 0 &&
          g.totals.exact == 1 && g.totals.first_bucket == -1 && g.totals.last_bucket == 1);
    // PutRequest's part has no value: its line adds nothing to the stats; 10^20 ms is no number
    CHECK(g.stats.size() == 3 && g.stats[0].numbers == 2 && g.stats[0].sum_lo == 8 && g.stats[1].lines == 2 && g.stats[1].sum_lo == 998 && g.stats[2].numbers == 3 &&
          g.stats[2].not_numbers == 1 && g.stats[2].max == 77777 && g.stats[2].min == 500);
    // GetRequest's lines under a term: /v2/d leaves
    g = def->bucketLines(b, off.data(), lines.size(), ids.data(), caps.data(), perMinute, 60, 60, &v1);
    CHECK(g.totals.lines == 9 && (g.lines == std::vector<uint64_t>{2, 3, 3}) && g.lineBucket[5] == 0xFFFFFFFFu);
    // whole files
    std::vector<uint64_t> counts;
    uint64_t n_lines = 0;
    Gorp::Buckets t = def->textBucketLines(text, perMinute, 60, 60, nullptr, &counts, &n_lines);
    CHECK(n_lines == lines.size() && (counts == std::vector<uint64_t>{1, 5, 4, 1, 0, 0, 0, 0}));
    CHECK((t.bucketNumber == std::vector<int64_t>{-1, 0, 1}) && (t.lines == std::vector<uint64_t>{2, 3, 4}) && t.lineBucket.size() == lines.size() && t.lineBucket[10] == 1);
    printf("GPU checks ok\n");
    return 0;
}
