// Exercises groupWindows() and textGroupWindows() of include/gorp.hpp.
//   windows_api_test          : host-only checks (refusals, no device is an error, never a CPU path) -- no GPU needed
//   windows_api_test --gpu    : also runs the calls on the device
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gorp.hpp"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

// a failed login: a time, a user, the bytes sent
static const char* DEF =
    "pattern %num \\d+\n"
    "pattern %word \\w+\n"
    "extract LoginFailed {\n  template [$ts(%num)] failed $user(%word) $size(%num)\n}\n"
    "extract LoginOk {\n  template [$ts(%num)] ok $user(%word)\n}\n";

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && strcmp(argv[1], "--gpu") == 0;
    using namespace gorp;
    auto def = DefinitionReader::reader(DEF).read(gpu ? 0 : GX_CREATE_HOST_ONLY);
    CHECK(def->getExtractions().size() == 2);

    Gorp::SeriesParts byUser = def->seriesParts();
    byUser.of("LoginFailed", "user", "ts", "size");
    // ann: 58 59 61 -- three within 10 --, then 200; bob: 10 70 130; an ok line that is no part's
    const std::vector<std::string> lines = {"[58] failed ann 1", "[10] failed bob 2", "[59] failed ann 3", "nothing here", "[61] failed ann 4", "[70] failed bob 5",
                                            "[60] ok ann", "[200] failed ann 6", "[130] failed bob 7"};
    std::string bytes, text;
    std::vector<uint32_t> off(1, 0);
    for (const std::string& ln : lines) { bytes += ln; text += ln + "\n"; off.push_back(static_cast<uint32_t>(bytes.size())); }
    const uint8_t* b = reinterpret_cast<const uint8_t*>(bytes.data());
    std::vector<int32_t> ids(lines.size(), -1), caps(lines.size() * 2 * static_cast<size_t>(def->maxGroups()), -1);
    Gorp::Where small = def->where();
    small.on("LoginFailed", "size").lt(static_cast<int64_t>(4));
    if (!gpu) {
        // refusals need no device ...
        try { def->groupWindows(b, off.data(), lines.size(), ids.data(), nullptr, byUser, 10, 3); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }                                   // parts on dense ids without capture rows
        gx_group_part one[1] = {{0, 0, -1, 0}};
        int32_t number[1] = {9};
        gx_windows_totals totals{};
        gx_group_out keys{};
        gx_windows_out wo{};
        uint64_t room[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        auto call = [&](const int32_t* numbers, int64_t window, uint32_t threshold, uint32_t flags, const gx_windows_out* windows, gx_windows_totals* t) {
            return gx_group_windows(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), one, 1, numbers, window, threshold, nullptr, 0, flags, &keys,
                                    windows, t, nullptr);
        };
        auto said = [](const char* words) { return std::string(gx_last_error()).find(words) != std::string::npos; };
        CHECK(call(nullptr, 10, 3, 0, &wo, &totals) == GX_E_ARG && said("number_groups is NULL"));
        CHECK(call(number, 10, 3, 0, &wo, &totals) == GX_E_ARG && said("number group"));
        number[0] = 0;
        CHECK(call(number, -1, 3, 0, &wo, &totals) == GX_E_ARG && said("window below 0"));
        CHECK(call(number, -1, 3, 0, nullptr, &totals) == GX_E_ARG);                          // windows == NULL still checks the window
        wo.entry_window_sum = reinterpret_cast<gx_window_sum*>(room);
        CHECK(call(number, 10, 3, 0, &wo, &totals) == GX_E_ARG && said("entry_window_sum without a value_group"));
        wo.entry_window_sum = nullptr;
        wo.trip_line = reinterpret_cast<uint32_t*>(room);
        CHECK(call(number, 10, 0, 0, &wo, &totals) == GX_E_ARG && said("trip outputs with threshold 0"));
        number[0] = -1;
        CHECK(call(number, 10, 3, 0, &wo, &totals) == GX_E_ARG && said("every part's number group is -1"));
        number[0] = 0;
        CHECK(call(number, 10, 3, 4u, &wo, &totals) == GX_E_ARG);
        CHECK(call(number, 10, 3, 0, &wo, nullptr) == GX_E_ARG);
        wo.max_trips = (1ull << 30) + 1;
        CHECK(call(number, 10, 3, 0, &wo, &totals) == GX_E_LIMIT);
        wo.max_trips = 8;
        wo.max_entries = (1ull << 30) + 1;
        CHECK(call(number, 10, 3, 0, &wo, &totals) == GX_E_LIMIT);
        wo.max_entries = 8;
        CHECK(gx_text_group_windows(def->handle(), reinterpret_cast<const uint8_t*>(text.data()), text.size(), one, 1, nullptr, 10, 3, nullptr, 0, 0, &keys, &wo, &totals,
                                    nullptr, nullptr, nullptr) == GX_E_ARG);
        // ... and behind them no device is an error, never a CPU path
        CHECK(call(number, 10, 3, GX_GROUP_WEAK_HASH | GX_BUCKET_ALL_DIGITS, &wo, &totals) == GX_E_DEVICE);
        CHECK(totals.entries == 0 && totals.peak_lines == 0 && totals.peak_line == 0xFFFFFFFFu && totals.peak_key == 0xFFFFFFFFu);
        try { def->groupWindows(b, off.data(), lines.size(), ids.data(), caps.data(), byUser, 10, 3, &small); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        try { def->textGroupWindows(text, byUser, 10, 3); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        printf("host-only checks ok\n");
        return 0;
    }
    def->extractBatch(b, off.data(), lines.size(), ids.data(), caps.data());
    CHECK((ids == std::vector<int32_t>{0, 0, 0, -1, 0, 0, 1, 0, 0}));
    Gorp::Windows w = def->groupWindows(b, off.data(), lines.size(), ids.data(), caps.data(), byUser, 10, 3);
    CHECK((w.keys == std::vector<std::string>{"ann", "bob"}) && (w.entryLine == std::vector<uint32_t>{0, 2, 4, 7, 1, 5, 8}));
    CHECK((w.entryKey == std::vector<uint32_t>{0, 0, 0, 0, 1, 1, 1}) && (w.entryTime == std::vector<int64_t>{58, 59, 61, 200, 10, 70, 130}));
    CHECK((w.entryWindowLines == std::vector<uint32_t>{1, 2, 3, 1, 1, 1, 1}) && (w.keyEntryBegin == std::vector<uint64_t>{0, 4, 7}));
    CHECK((w.lineWindowLines == std::vector<uint32_t>{1, 1, 2, 0, 3, 1, 0, 1, 1}));
    CHECK((w.tripKey == std::vector<uint32_t>{0}) && (w.tripLine == std::vector<uint32_t>{4}) && (w.tripTime == std::vector<int64_t>{61}) &&
          (w.tripEntry == std::vector<uint32_t>{2}) && (w.keyTripBegin == std::vector<uint64_t>{0, 1, 1}));
    CHECK((w.keyPeakLines == std::vector<uint32_t>{3, 1}) && (w.keyPeakLine == std::vector<uint32_t>{4, 1}));
    CHECK(w.entryWindowSum.size() == 7 && w.entryWindowSum[2].numbers == 3 && w.entryWindowSum[2].sum_lo == 8 && w.entryWindowSum[2].sum_hi == 0 &&
          w.entryWindowSum[3].sum_lo == 6 && w.entryWindowSum[3].reserved == 0);
    CHECK(w.windows.entries == 7 && w.windows.n_trips == 1 && w.windows.tripped_keys == 1 && w.windows.peak_lines == 3 && w.windows.peak_line == 4 &&
          w.windows.peak_key == 0 && w.windows.first_time == 10 && w.windows.last_time == 200 && w.totals.keyed == 7 && w.totals.n_keys == 2);
    // under a term ann's line of size 4 does not count: two within 10, no trip
    w = def->groupWindows(b, off.data(), lines.size(), ids.data(), caps.data(), byUser, 10, 3, &small);
    CHECK(w.windows.n_trips == 0 && w.tripKey.empty() && w.windows.peak_lines == 2 && w.lineWindowLines[4] == 0 && (w.keyTripBegin == std::vector<uint64_t>{0, 0, 0}));
    // threshold 0: the counts alone
    w = def->groupWindows(b, off.data(), lines.size(), ids.data(), caps.data(), byUser, 1000);
    CHECK(w.windows.n_trips == 0 && (w.entryWindowLines == std::vector<uint32_t>{1, 2, 3, 4, 1, 2, 3}) && (w.keyTripBegin == std::vector<uint64_t>{0, 0, 0}));
    // no part has a time: the keys alone
    Gorp::SeriesParts untimed = def->seriesParts();
    untimed.of("LoginFailed", "user", "");
    w = def->groupWindows(b, off.data(), lines.size(), ids.data(), caps.data(), untimed, 10, 3);
    CHECK(w.windows.entries == 0 && w.windows.number_unset == 7 && w.entryLine.empty() && (w.keyEntryBegin == std::vector<uint64_t>{0, 0, 0}) &&
          (w.keyPeakLine == std::vector<uint32_t>{0xFFFFFFFFu, 0xFFFFFFFFu}) && w.lineWindowLines.size() == lines.size());
    // whole files
    std::vector<uint64_t> counts;
    uint64_t n_lines = 0;
    Gorp::Windows t = def->textGroupWindows(text, byUser, 10, 3, nullptr, &counts, &n_lines);
    CHECK(n_lines == lines.size() && (counts == std::vector<uint64_t>{7, 1, 1, 0, 0, 0}));
    CHECK((t.tripLine == std::vector<uint32_t>{4}) && (t.entryWindowLines == std::vector<uint32_t>{1, 2, 3, 1, 1, 1, 1}) && (t.keys == std::vector<std::string>{"ann", "bob"}));
    CHECK(t.windows.peak_line == 4 && (t.lineWindowLines == std::vector<uint32_t>{1, 1, 2, 0, 3, 1, 0, 1, 1}));
    printf("GPU checks ok\n");
    return 0;
}
