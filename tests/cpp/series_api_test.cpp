// Exercises groupSeries() and textGroupSeries() of include/gorp.hpp, with the SeriesParts builder, and the C ABI's refusals.
//   series_api_test          : host-only checks (refusals, no device is an error, never a CPU path) -- no GPU needed
//   series_api_test --gpu    : also runs the calls on the device
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

    Gorp::SeriesParts perVerb = def->seriesParts();
    perVerb.of("GetRequest", "verb", "timestamp", "timeTakenInMsec").of("PutRequest", "verb", "timestamp").of(2, 1, 0, 2);
    const std::vector<gx_group_part>& pp = perVerb.keys().parts();
    CHECK(pp.size() == 3 && perVerb.keys().hasValues() && pp[0].extraction == 1 && pp[0].key_group == 1 && pp[0].value_group == 2 && pp[1].value_group == -1 &&
          pp[2].extraction == 2 && (perVerb.numbers() == std::vector<int32_t>{0, 0, 0}));
    CHECK((def->seriesParts().of("GetRequest", "verb", "").numbers() == std::vector<int32_t>{-1}));
    try { def->seriesParts().of("GetRequest", "verb", "nothing"); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->seriesParts().of(0, 1, 4); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->seriesParts().of(0, 1, -2); CHECK(false); } catch (std::invalid_argument&) {}
    try { def->seriesParts().of("GetRequest", "verb", "timestamp").of("GetRequest", "path", "timestamp"); CHECK(false); } catch (std::invalid_argument&) {}
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
        try { def->groupSeries(b, off.data(), lines.size(), ids.data(), nullptr, perVerb, 60); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }                                   // parts on dense ids without capture rows
        try { def->groupSeries(b, off.data(), lines.size(), ids.data(), caps.data(), perVerb, 0); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG && std::string(e.what()).find("width") != std::string::npos); }
        gx_group_part one[2] = {{0, 1, -1, 0}, {1, 1, -1, 0}}, twice[2] = {{0, 1, -1, 0}, {0, 1, -1, 0}}, reserved[1] = {{0, 1, -1, 1}};
        const int32_t numbers[2] = {0, 0}, bad[2] = {0, 4}, worse[2] = {-2, 0}, nothing[2] = {-1, -1};
        gx_series_totals totals{};
        gx_series_out into{};
        gx_group_out keys{};
        std::vector<uint32_t> line_cell(lines.size());
        std::vector<gx_measure_stats> stats(lines.size());
        into.line_cell = line_cell.data();
        into.max_cells = lines.size();
        keys.max_keys = lines.size();
        const uint8_t* t8 = reinterpret_cast<const uint8_t*>(text.data());
        gx_handle* h = def->handle();
        const uint64_t n = lines.size();
        const int32_t *i = ids.data(), *c = caps.data();
        const uint32_t* o32 = off.data();
        CHECK(gx_group_series(h, b, o32, n, i, c, one, 2, nullptr, 0, 60, nullptr, 0, 0, &keys, &into, &totals, nullptr) == GX_E_ARG);         // number_groups == NULL
        CHECK(gx_group_series(h, b, o32, n, i, c, one, 2, bad, 0, 60, nullptr, 0, 0, &keys, &into, &totals, nullptr) == GX_E_ARG);             // not one of its extraction's
        CHECK(gx_group_series(h, b, o32, n, i, c, one, 2, worse, 0, 60, nullptr, 0, 0, &keys, &into, &totals, nullptr) == GX_E_ARG);
        CHECK(gx_group_series(h, b, o32, n, i, c, one, 2, numbers, 0, 0, nullptr, 0, 0, &keys, &into, &totals, nullptr) == GX_E_ARG);          // width < 1
        CHECK(gx_group_series(h, b, o32, n, i, c, one, 2, numbers, 0, -60, nullptr, 0, 0, &keys, &into, &totals, nullptr) == GX_E_ARG);
        CHECK(gx_group_series(h, b, o32, n, i, c, one, 2, nothing, 0, 60, nullptr, 0, 0, &keys, &into, &totals, nullptr) == GX_E_ARG);         // an output, no number
        CHECK(gx_group_series(h, b, o32, n, i, c, one, 2, numbers, 0, 60, nullptr, 0, 4, &keys, &into, &totals, nullptr) == GX_E_ARG);         // unknown flag bits
        CHECK(gx_group_series(h, b, o32, n, i, c, one, 2, numbers, 0, 60, nullptr, 0, 0, &keys, &into, nullptr, nullptr) == GX_E_ARG);         // totals == NULL
        CHECK(gx_group_series(h, b, o32, n, i, c, nullptr, 2, numbers, 0, 60, nullptr, 0, 0, &keys, &into, &totals, nullptr) == GX_E_ARG);
        CHECK(gx_group_series(h, b, o32, n, i, c, twice, 2, numbers, 0, 60, nullptr, 0, 0, &keys, &into, &totals, nullptr) == GX_E_ARG);
        CHECK(gx_group_series(h, b, o32, n, i, c, reserved, 1, numbers, 0, 60, nullptr, 0, 0, &keys, &into, &totals, nullptr) == GX_E_ARG);
        into.cell_stats = stats.data();
        CHECK(gx_group_series(h, b, o32, n, i, c, one, 2, numbers, 0, 60, nullptr, 0, 0, &keys, &into, &totals, nullptr) == GX_E_ARG);         // stats, no value_group
        CHECK(gx_text_group_series(h, t8, text.size(), one, 2, numbers, 0, 60, nullptr, 0, 0, &keys, &into, &totals, nullptr, nullptr, nullptr) == GX_E_ARG);
        into.cell_stats = nullptr;
        gx_batch_opts o{};
        o.struct_size = sizeof(o);
        o.no_sync = 1;
        CHECK(gx_group_series(h, b, o32, n, i, c, one, 2, numbers, 0, 60, nullptr, 0, 0, &keys, &into, &totals, &o) == GX_E_ARG);
        o.no_sync = 0;
        o.utf8 = 2;
        CHECK(gx_group_series(h, b, o32, n, i, c, one, 2, numbers, 0, 60, nullptr, 0, 0, &keys, &into, &totals, &o) == GX_E_ARG);
        into.max_cells = (1ull << 30) + 1;
        CHECK(gx_group_series(h, b, o32, n, i, c, one, 2, numbers, 0, 60, nullptr, 0, 0, &keys, &into, &totals, nullptr) == GX_E_LIMIT);
        CHECK(gx_text_group_series(h, t8, text.size(), one, 2, numbers, 0, 60, nullptr, 0, 0, &keys, &into, &totals, nullptr, nullptr, nullptr) == GX_E_LIMIT);
        into.max_cells = n;
        CHECK(gx_group_series(h, b, o32, 0xFFFFFFFFull, i, c, one, 2, numbers, 0, 60, nullptr, 0, 0, &keys, &into, &totals, nullptr) == GX_E_LIMIT);
        // ... and behind them no device is an error, never a CPU path
        CHECK(gx_group_series(h, b, o32, n, i, c, one, 2, numbers, -5, 60, nullptr, 0, GX_GROUP_WEAK_HASH | GX_BUCKET_ALL_DIGITS, &keys, &into, &totals, nullptr) ==
              GX_E_DEVICE);
        CHECK(gx_group_series(h, b, o32, n, i, c, one, 2, nothing, 0, 1, nullptr, 0, 0, &keys, nullptr, &totals, nullptr) == GX_E_DEVICE);      // series == NULL
        CHECK(totals.cells_exact == 1 && totals.n_cells == 0);
        CHECK(gx_text_group_series(h, t8, text.size(), one, 2, numbers, 0, 60, nullptr, 0, 0, nullptr, nullptr, &totals, nullptr, nullptr, nullptr) == GX_E_DEVICE);
        try { def->groupSeries(b, off.data(), lines.size(), ids.data(), caps.data(), perVerb, 60, 0, &v1); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        try { def->textGroupSeries(text, perVerb, 60); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        printf("host-only checks ok\n");
        return 0;
    }
    def->extractBatch(b, off.data(), lines.size(), ids.data(), caps.data());
    CHECK((ids == std::vector<int32_t>{1, 2, 0, -1, 2, 1, 2, 1, 1, 1, 2}));
    // per 60 from origin 60: 130 -> 1, 119 -> 0, 60 -> 0, 59 -> -1, 121 -> 1, 0 -> -1, 179 -> 1, 120 -> 1, 10^20 -> no number, 61 -> 0
    // keys by first appearance: GET, POST, PUT, HEAD; cells: (GET, 1), (POST, -1), (POST, 0), (PUT, 0), (HEAD, -1)
    const uint32_t NONE = 0xFFFFFFFFu;
    Gorp::Series g = def->groupSeries(b, off.data(), lines.size(), ids.data(), caps.data(), perVerb, 60, 60);
    CHECK((g.keys == std::vector<std::string>{"GET", "POST", "PUT", "HEAD"}) && (g.lines == std::vector<uint64_t>{5, 3, 1, 1}));
    CHECK((g.bucketNumber == std::vector<int64_t>{-1, 0, 1}) && (g.cellKey == std::vector<uint32_t>{0, 1, 1, 2, 3}) && (g.cellBucket == std::vector<uint32_t>{2, 0, 1, 1, 0}));
    CHECK((g.cellFirstLine == std::vector<uint32_t>{0, 4, 1, 2, 6}) && (g.cellLines == std::vector<uint64_t>{4, 1, 2, 1, 1}));
    CHECK((g.keyCellBegin == std::vector<uint64_t>{0, 1, 3, 4, 5}) && (g.lineCell == std::vector<uint32_t>{0, 2, 3, NONE, 1, 0, 4, 0, 0, NONE, 2}));
    CHECK(g.series.n_cells == 5 && g.series.n_buckets == 3 && g.series.celled == 9 && g.series.not_numbers == 1 && g.series.number_unset == 0 &&
          g.series.out_of_range == 0 && g.series.cells_exact == 1 && g.series.first_bucket == -1 && g.series.last_bucket == 1 && g.series.group.keyed == 10 &&
          g.totals.n_keys == 4);
    // PutRequest's part has no value: its line adds nothing to the stats; 10^20 ms is no number
    CHECK(g.cellStats.size() == 5 && g.cellStats[0].numbers == 3 && g.cellStats[0].not_numbers == 1 && g.cellStats[0].max == 77777 && g.cellStats[0].min == 500 &&
          g.cellStats[1].sum_lo == 1 && g.cellStats[2].sum_lo == 998 && g.cellStats[3].lines == 0 && g.cellStats[4].sum_lo == 7);
    // GetRequest's lines under a term: /v2/d leaves the GET cell
    g = def->groupSeries(b, off.data(), lines.size(), ids.data(), caps.data(), perVerb, 60, 60, &v1);
    CHECK(g.totals.lines == 9 && (g.cellLines == std::vector<uint64_t>{3, 1, 2, 1, 1}) && g.lineCell[5] == NONE);
    // a part without a number: GetRequest's lines have a key and no cell
    Gorp::SeriesParts others = def->seriesParts();
    others.of("GetRequest", "verb", "").of("OtherRequest", "verb", "timestamp");
    g = def->groupSeries(b, off.data(), lines.size(), ids.data(), caps.data(), others, 60, 60);
    CHECK((g.keys == std::vector<std::string>{"GET", "POST", "HEAD"}) && (g.keyCellBegin == std::vector<uint64_t>{0, 0, 2, 3}) && g.series.number_unset == 5 &&
          g.cellStats.empty());
    // whole files
    std::vector<uint64_t> counts;
    uint64_t n_lines = 0;
    Gorp::Series t = def->textGroupSeries(text, perVerb, 60, 60, nullptr, &counts, &n_lines);
    CHECK(n_lines == lines.size() && (counts == std::vector<uint64_t>{1, 5, 4, 1, 0, 0, 0, 0}));
    CHECK((t.bucketNumber == std::vector<int64_t>{-1, 0, 1}) && (t.cellLines == std::vector<uint64_t>{4, 1, 2, 1, 1}) && t.lineCell.size() == lines.size() &&
          t.lineCell[10] == 2 && (t.keyCellBegin == std::vector<uint64_t>{0, 1, 3, 4, 5}));
    printf("GPU checks ok\n");
    return 0;
}
