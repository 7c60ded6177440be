// Exercises the outcome calls of include/gorp.hpp: want(), countOutcomes(), selectLines(), textSelect().
//   select_api_test          : host-only checks (want masks; no device is an error, never a CPU path) -- no GPU needed
//   select_api_test --gpu    : also runs the three calls on the device
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gorp.hpp"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static const char* DEF =
    "pattern %word ([a-zA-Z]+)\n"
    "pattern %any .*\n"
    "extract single {  \n"
    "  template value=$value(%word)\n"
    "}\n"
    "extract ab {  \n"
    "  template a$x(%any)b\n"
    "}\n";

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && strcmp(argv[1], "--gpu") == 0;
    using namespace gorp;
    auto def = DefinitionReader::reader(DEF).read(gpu ? 0 : GX_CREATE_HOST_ONLY);
    CHECK(def->getExtractions().size() == 2);
    typedef Gorp::Want Want;
    CHECK(def->want(true, false) == (Want{0, 0, 1, 0, 0}));
    CHECK(def->want(false, true) == (Want{0, 0, 0, 1, 1}));
    CHECK(def->want(true, true, {1}) == (Want{0, 1, 1, 1, 1}));
    CHECK(def->want(false, false, {0, 1}) == (Want{1, 1, 0, 0, 0}));
    try { def->want(false, false, {2}); CHECK(false); } catch (std::out_of_range&) {}

    // lines: single, unmatched, ab, exception of ab ("." does not match "\r"), empty, single (no terminator)
    const std::string text = "value=foo\nnothing here\r\na--b\na\rb\n\nvalue=bar";
    const std::vector<uint32_t> offsets = {0, 10, 24, 29, 31, 33, 34, 43};   // "a\rb\n" is the lines "a" and "b": see below
    if (!gpu) {
        const std::vector<int32_t> ids = {0, -1, 1};
        try { def->countOutcomes(ids.data(), ids.size()); CHECK(false); } catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        try { def->selectLines(reinterpret_cast<const uint8_t*>(text.data()), offsets.data(), 2, ids.data(), def->want(true, true)); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        try { def->textSelect(text, def->want(true, true)); CHECK(false); } catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        try { def->textSelect(text, Want{1}); CHECK(false); } catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }
        printf("host-only checks ok\n");
        return 0;
    }
    // whole file: readLine() ends a line at the lone "\r" too, so "a\rb\n" is the two unmatched lines "a\r" and "b\n"
    std::vector<uint64_t> counts;
    uint64_t n_lines = 0;
    const std::string dropped = def->textSelect(text, def->want(true, true), &counts, &n_lines);
    CHECK(n_lines == 7);
    CHECK(dropped == "nothing here\r\na\rb\n\n");
    CHECK((counts == std::vector<uint64_t>{2, 1, 4, 0, 0, 0}));
    CHECK(def->textSelect(text, def->want(false, false, {0})) == "value=foo\nvalue=bar");
    CHECK(def->textSelect("", def->want(true, true)).empty());

    // a batch whose lines carry no terminators: "a\rb" is ONE line there, and an exception of extraction 1
    const std::vector<std::string> lines = {"value=foo", "zzz", "a--b", "a\rb", "", "value=bar"};
    std::string bytes;
    std::vector<uint32_t> off(1, 0);
    for (const std::string& ln : lines) { bytes += ln; off.push_back(static_cast<uint32_t>(bytes.size())); }
    std::vector<int32_t> ids(lines.size()), caps(lines.size() * 2 * static_cast<size_t>(def->maxGroups()));
    const uint8_t* p = reinterpret_cast<const uint8_t*>(bytes.data());
    def->extractBatch(p, off.data(), lines.size(), ids.data(), caps.data());
    CHECK((ids == std::vector<int32_t>{0, -1, 1, -3, -1, 0}));
    CHECK((def->countOutcomes(ids.data(), ids.size()) == std::vector<uint64_t>{2, 1, 2, 0, 1, 0}));
    Gorp::Selection s = def->selectLines(p, off.data(), lines.size(), ids.data(), def->want(true, true));
    CHECK((s.index == std::vector<uint32_t>{1, 3, 4}));
    CHECK(std::string(s.bytes.begin(), s.bytes.end()) == "zzza\rb");
    CHECK((s.offsets == std::vector<uint32_t>{0, 3, 6, 6}));
    s = def->selectLines(p, off.data(), lines.size(), ids.data(), def->want(false, false));
    CHECK(s.index.empty() && s.bytes.empty() && s.offsets == std::vector<uint32_t>{0});
    printf("GPU checks ok\n");
    return 0;
}
