// Exercises groupSessions() and textGroupSessions() of include/gorp.hpp, with the SeriesParts builder reused.
//   sessions_api_test          : host-only checks (refusals, no device is an error, never a CPU path) -- no GPU needed
//   sessions_api_test --gpu    : also runs the calls on the device
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

    // sessions per path, in the order of the timestamps, measured by the time taken
    Gorp::SeriesParts byPath = def->seriesParts();
    byPath.of("GetRequest", "path", "timestamp", "timeTakenInMsec").of("PutRequest", "path", "timestamp", "timeTakenInMsec").of("OtherRequest", "path", "timestamp");
    const std::vector<std::string> lines = {"[100]: GET 5ms /a", "[105]: POST 4ms /b", "[130]: PUT 9ms /a", "nothing here", "[131]: GET 1ms /a",
                                            "[104]: HEAD 7ms /b", "[162]: GET 50ms /a", "[99999999999999999999]: GET 5ms /a", "[300]: GET 2ms /c"};
    std::string bytes, text;
    std::vector<uint32_t> off(1, 0);
    for (const std::string& ln : lines) { bytes += ln; text += ln + "\n"; off.push_back(static_cast<uint32_t>(bytes.size())); }
    const uint8_t* b = reinterpret_cast<const uint8_t*>(bytes.data());
    std::vector<int32_t> ids(lines.size(), -1), caps(lines.size() * 2 * static_cast<size_t>(def->maxGroups()), -1);
    Gorp::Where fast = def->where();
    fast.on("GetRequest", "timeTakenInMsec").lt(static_cast<int64_t>(10));
    if (!gpu) {
        // refusals need no device ...
        try { def->groupSessions(b, off.data(), lines.size(), ids.data(), nullptr, byPath, 30); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }                                   // parts on dense ids without capture rows
        try { def->groupSessions(b, off.data(), lines.size(), ids.data(), caps.data(), byPath, -1); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG && std::string(e.what()).find("max_gap") != std::string::npos); }
        gx_group_part one[1] = {{0, 0, -1, 0}};
        int32_t number[1] = {9};
        gx_sessions_totals totals{};
        gx_group_out keys{};
        gx_sessions_out so{};
        CHECK(gx_group_sessions(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), one, 1, nullptr, 0, nullptr, 0, 0, &keys, &so, &totals, nullptr) == GX_E_ARG);
        CHECK(gx_group_sessions(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), one, 1, number, 0, nullptr, 0, 0, &keys, &so, &totals, nullptr) == GX_E_ARG);
        number[0] = 0;
        CHECK(gx_group_sessions(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), one, 1, number, 0, nullptr, 0, 4u, &keys, &so, &totals, nullptr) == GX_E_ARG);
        CHECK(gx_group_sessions(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), one, 1, number, 0, nullptr, 0, 0, &keys, &so, nullptr, nullptr) == GX_E_ARG);
        CHECK(gx_group_sessions(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), one, 1, number, -5, nullptr, 0, 0, &keys, nullptr, &totals, nullptr) == GX_E_ARG);
        so.max_sessions = (1ull << 30) + 1;
        CHECK(gx_group_sessions(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), one, 1, number, 0, nullptr, 0, 0, &keys, &so, &totals, nullptr) == GX_E_LIMIT);
        so.max_sessions = 0;
        uint64_t room[4] = {0, 0, 0, 0};
        so.session_stats = reinterpret_cast<gx_measure_stats*>(room);                          // session_stats where no part has a value group
        CHECK(gx_text_group_sessions(def->handle(), reinterpret_cast<const uint8_t*>(text.data()), text.size(), one, 1, number, 0, nullptr, 0, 0, &keys, &so, &totals, nullptr,
                                     nullptr, nullptr) == GX_E_ARG);
        // ... and behind them no device is an error, never a CPU path
        try { def->groupSessions(b, off.data(), lines.size(), ids.data(), caps.data(), byPath, 30, &fast); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        try { def->textGroupSessions(text, byPath, 30); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        so.session_stats = nullptr;
        CHECK(gx_group_sessions(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), one, 1, number, INT64_MAX, nullptr, 0,
                                GX_GROUP_WEAK_HASH | GX_BUCKET_ALL_DIGITS, &keys, &so, &totals, nullptr) == GX_E_DEVICE);
        printf("host-only checks ok\n");
        return 0;
    }
    def->extractBatch(b, off.data(), lines.size(), ids.data(), caps.data());
    CHECK((ids == std::vector<int32_t>{1, 2, 0, -1, 1, 2, 1, 1, 1}));
    // /a: 100, 130, 131 | 162 (31 after 131); /b: 104, 105; /c: 300; line 7's timestamp is no number
    Gorp::Sessions s = def->groupSessions(b, off.data(), lines.size(), ids.data(), caps.data(), byPath, 30);
    CHECK((s.keys == std::vector<std::string>{"/a", "/b", "/c"}) && (s.sessionKey == std::vector<uint32_t>{0, 0, 1, 2}));
    CHECK((s.sessionBegin == std::vector<int64_t>{100, 162, 104, 300}) && (s.sessionEnd == std::vector<int64_t>{131, 162, 105, 300}));
    CHECK((s.sessionFirstLine == std::vector<uint32_t>{0, 6, 5, 8}) && (s.sessionLines == std::vector<uint64_t>{3, 1, 2, 1}));
    CHECK((s.sessionEntryBegin == std::vector<uint64_t>{0, 3, 4, 6, 7}) && (s.keySessionBegin == std::vector<uint64_t>{0, 2, 3, 4}));
    CHECK((s.entryLine == std::vector<uint32_t>{0, 2, 4, 6, 5, 1, 8}));
    CHECK((s.lineSession == std::vector<uint32_t>{0, 2, 0, 0xFFFFFFFFu, 0, 2, 1, 0xFFFFFFFFu, 3}));
    CHECK(s.sessions.n_sessions == 4 && s.sessions.entries == 7 && s.sessions.not_numbers == 1 && s.sessions.number_unset == 0 && s.sessions.longest_lines == 3);
    CHECK(s.sessions.longest_duration == 31 && s.sessions.first_time == 100 && s.sessions.last_time == 300 && s.totals.keyed == 8 && s.totals.n_keys == 3);
    CHECK(s.sessionStats.size() == 4 && s.sessionStats[0].numbers == 3 && s.sessionStats[0].sum_lo == 15 && s.sessionStats[0].min == 1 && s.sessionStats[0].max == 9);
    CHECK(s.sessionStats[2].lines == 0 && s.sessionStats[1].sum_lo == 50 && (s.lines == std::vector<uint64_t>{5, 2, 1}));
    // a gap of 31 joins /a's two sessions; a gap of 0 parts everything but nothing else
    s = def->groupSessions(b, off.data(), lines.size(), ids.data(), caps.data(), byPath, 31);
    CHECK((s.sessionLines == std::vector<uint64_t>{4, 2, 1}) && s.sessions.longest_duration == 62);
    s = def->groupSessions(b, off.data(), lines.size(), ids.data(), caps.data(), byPath, 0);
    CHECK(s.sessions.n_sessions == 7 && s.sessions.longest_lines == 1);
    // under a term the slow GET (line 6) does not count
    s = def->groupSessions(b, off.data(), lines.size(), ids.data(), caps.data(), byPath, 30, &fast);
    CHECK((s.sessionLines == std::vector<uint64_t>{3, 2, 1}) && s.lineSession[6] == 0xFFFFFFFFu && s.totals.lines == 7);
    // no part has a time: the keys alone
    Gorp::SeriesParts untimed = def->seriesParts();
    untimed.of("GetRequest", "path", "");
    s = def->groupSessions(b, off.data(), lines.size(), ids.data(), caps.data(), untimed, 30);
    CHECK(s.sessions.n_sessions == 0 && s.sessions.number_unset == 5 && (s.keySessionBegin == std::vector<uint64_t>{0, 0, 0}) && s.lineSession.size() == lines.size());
    // whole files
    std::vector<uint64_t> counts;
    uint64_t n_lines = 0;
    Gorp::Sessions t = def->textGroupSessions(text, byPath, 30, nullptr, &counts, &n_lines);
    CHECK(n_lines == lines.size() && (counts == std::vector<uint64_t>{1, 5, 2, 1, 0, 0, 0, 0}));
    CHECK((t.sessionKey == std::vector<uint32_t>{0, 0, 1, 2}) && (t.entryLine == std::vector<uint32_t>{0, 2, 4, 6, 5, 1, 8}) && t.sessions.n_sessions == 4);
    CHECK((t.sessionBegin == std::vector<int64_t>{100, 162, 104, 300}) && t.sessionStats[0].sum_lo == 15 && (t.keys == std::vector<std::string>{"/a", "/b", "/c"}));
    printf("GPU checks ok\n");
    return 0;
}
