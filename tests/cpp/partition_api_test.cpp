// Exercises the partition calls of include/gorp.hpp: partitionLines(), textToJsonlByExtraction().
//   partition_api_test          : host-only checks (the argument checks; no device is an error, never a CPU path) -- no GPU needed
//   partition_api_test --gpu    : also runs the two calls on the device, on the README's definition
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gorp.hpp"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static const char* DEF =
    "pattern %num \\d+\npattern %word \\w+\npattern %phrase \\S+\n\n"
    "extract PutRequest {\n   template [$timestamp(%num)]: $verb(PUT) $timeTakenInMsec(%num)ms $path(%phrase)\n}\n"
    "extract GetRequest {\n   template [$timestamp(%num)]: $verb(GET) $timeTakenInMsec(%num)ms $path(%phrase)\n}\n"
    "extract OtherRequest {\n   template [$timestamp(%num)]: $verb(%word) $timeTakenInMsec(%num)ms $path(%phrase)\n}\n";

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && strcmp(argv[1], "--gpu") == 0;
    using namespace gorp;
    auto def = DefinitionReader::reader(DEF).read(gpu ? 0 : GX_CREATE_HOST_ONLY);
    CHECK(def->getExtractions().size() == 3);
    typedef Gorp::Want Want;
    typedef std::vector<uint64_t> U64;

    // lines: Get, unmatched, Put, Other, Get, empty, Put (no terminator)
    const std::vector<std::string> lines = {"[1]: GET 1ms /a", "nothing here", "[2]: PUT 22ms /bb", "[3]: HEAD 3ms /c", "[4]: GET 4ms /d", "", "[5]: PUT 5ms /e"};
    std::string bytes, text;
    std::vector<uint32_t> off(1, 0);
    for (size_t i = 0; i < lines.size(); ++i) {
        bytes += lines[i];
        off.push_back(static_cast<uint32_t>(bytes.size()));
        text += lines[i] + (i + 1 < lines.size() ? (i % 2 ? "\r\n" : "\n") : "");
    }
    const uint8_t* p = reinterpret_cast<const uint8_t*>(bytes.data());
    if (!gpu) {
        const std::vector<int32_t> ids = {1, -1, 0, 2, 1, -1, 0};
        try { def->partitionLines(p, off.data(), ids.size(), ids.data()); CHECK(false); } catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        const Want all = def->want(true, true, {0, 1, 2});
        try { def->partitionLines(p, off.data(), ids.size(), ids.data(), &all); CHECK(false); } catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        const Want bad{1};
        try { def->partitionLines(p, off.data(), ids.size(), ids.data(), &bad); CHECK(false); } catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }
        try { def->textToJsonlByExtraction(text, "rule"); CHECK(false); } catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        uint64_t k = 0, size = 0;
        CHECK(gx_partition_lines(nullptr, p, off.data(), 7, ids.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, &k, &size,
                                 nullptr) == GX_E_ARG);
        CHECK(gx_partition_lines(def->handle(), p, nullptr, 7, ids.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, &k, &size,
                                 nullptr) == GX_E_ARG);
        CHECK(gx_text_to_jsonl_by_extraction(def->handle(), nullptr, 5, nullptr, nullptr, 0, &size, nullptr, nullptr, nullptr, nullptr) == GX_E_ARG);
        printf("host-only checks ok\n");
        return 0;
    }
    std::vector<int32_t> ids(lines.size()), caps(lines.size() * 2 * static_cast<size_t>(def->maxGroups()));
    def->extractBatch(p, off.data(), lines.size(), ids.data(), caps.data());
    CHECK((ids == std::vector<int32_t>{1, -1, 0, 2, 1, -1, 0}));
    // every outcome: Put (lines 2, 6), Get (0, 4), Other (3), unmatched (1, 5); K = 3, so 2K + 3 = 9 boundaries
    Gorp::Partition s = def->partitionLines(p, off.data(), lines.size(), ids.data());
    CHECK((s.index == std::vector<uint32_t>{2, 6, 0, 4, 3, 1, 5}));
    CHECK(std::string(s.bytes.begin(), s.bytes.end()) == lines[2] + lines[6] + lines[0] + lines[4] + lines[3] + lines[1] + lines[5]);
    CHECK((s.groupLines == U64{0, 2, 4, 5, 7, 7, 7, 7, 7}));
    CHECK(s.offsets.size() == 8 && s.offsets[0] == 0 && s.offsets[7] == bytes.size());
    for (size_t x = 0; x < s.groupLines.size(); ++x) CHECK(s.groupUnits[x] == s.offsets[s.groupLines[x]]);
    // the sinks of Get and of the unmatched lines only
    const Want some = def->want(true, false, {1});
    s = def->partitionLines(p, off.data(), lines.size(), ids.data(), &some);
    CHECK((s.index == std::vector<uint32_t>{0, 4, 1, 5}));
    CHECK(std::string(s.bytes.begin(), s.bytes.end()) == lines[0] + lines[4] + lines[1] + lines[5]);
    CHECK((s.groupLines == U64{0, 0, 2, 2, 4, 4, 4, 4, 4}));
    CHECK((s.offsets == std::vector<uint32_t>{0, 15, 30, 42, 42}));
    const Want none = def->want(false, false);
    s = def->partitionLines(p, off.data(), lines.size(), ids.data(), &none);
    CHECK(s.index.empty() && s.bytes.empty() && s.offsets == std::vector<uint32_t>{0} && s.groupLines == U64(9, 0));

    // whole file: textToJsonl's lines, regrouped by extraction
    const std::string flat = def->textToJsonl(text, "rule");
    std::vector<std::string> objs;
    for (size_t at = 0; at < flat.size();) { const size_t e = flat.find('\n', at) + 1; objs.push_back(flat.substr(at, e - at)); at = e; }
    CHECK(objs.size() == 5);   // Get, Put, Other, Get, Put
    U64 group_out, counts;
    uint64_t n_lines = 0;
    const std::string grouped = def->textToJsonlByExtraction(text, "rule", &group_out, &counts, &n_lines);
    CHECK(grouped == objs[1] + objs[4] + objs[0] + objs[3] + objs[2]);
    CHECK((group_out == U64{0, objs[1].size() + objs[4].size(), grouped.size() - objs[2].size(), grouped.size()}));
    CHECK(n_lines == 7 && (counts == U64{2, 2, 1, 2, 0, 0, 0, 0}));
    CHECK(objs[1].find("\"rule\":\"PutRequest\"") != std::string::npos && objs[1].find("\"path\":\"/bb\"") != std::string::npos);
    CHECK(def->textToJsonlByExtraction("", "rule", &group_out).empty() && group_out == U64(4, 0));
    printf("GPU checks ok\n");
    return 0;
}
