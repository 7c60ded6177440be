// Exercises groupSpans() and textGroupSpans() of include/gorp.hpp, with the SpanParts builder.
//   spans_api_test          : host-only checks (refusals, no device is an error, never a CPU path) -- no GPU needed
//   spans_api_test --gpu    : also runs the calls on the device
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gorp.hpp"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

// a start line and an end line that capture the same id
static const char* DEF =
    "pattern %num \\d+\n"
    "pattern %word \\w+\n"
    "extract RequestStart {\n  template [$ts(%num)] start $id(%word) $size(%num)\n}\n"
    "extract RequestEnd {\n  template [$ts(%num)] end $id(%word)\n}\n";

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && strcmp(argv[1], "--gpu") == 0;
    using namespace gorp;
    auto def = DefinitionReader::reader(DEF).read(gpu ? 0 : GX_CREATE_HOST_ONLY);
    CHECK(def->getExtractions().size() == 2);

    Gorp::SpanParts byId = def->spanParts();
    byId.begin("RequestStart", "id", "ts").end("RequestEnd", "id", "ts");
    CHECK((byId.roles() == std::vector<uint32_t>{GX_SPAN_BEGIN, GX_SPAN_END}) && byId.timed().numbers().size() == 2);
    try { def->spanParts().of(0, 0, -1, 3u); CHECK(false); }
    catch (std::invalid_argument&) {}
    // a: B B E E -- one span, one superseded begin, one orphan end; b: a span stamped backwards; c: left open; d: an orphan end
    const std::vector<std::string> lines = {"[100] start a 1", "[105] start b 2", "[110] start a 3", "nothing here", "[140] end a", "[90] end b",
                                            "[150] end a", "[160] start c 4", "[170] end d"};
    std::string bytes, text;
    std::vector<uint32_t> off(1, 0);
    for (const std::string& ln : lines) { bytes += ln; text += ln + "\n"; off.push_back(static_cast<uint32_t>(bytes.size())); }
    const uint8_t* b = reinterpret_cast<const uint8_t*>(bytes.data());
    std::vector<int32_t> ids(lines.size(), -1), caps(lines.size() * 2 * static_cast<size_t>(def->maxGroups()), -1);
    Gorp::Where small = def->where();
    small.on("RequestStart", "size").lt(static_cast<int64_t>(3));
    if (!gpu) {
        // refusals need no device ...
        try { def->groupSpans(b, off.data(), lines.size(), ids.data(), nullptr, byId); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_ARG); }                                   // parts on dense ids without capture rows
        gx_group_part one[1] = {{0, 0, -1, 0}};
        int32_t number[1] = {9};
        uint32_t role[1] = {GX_SPAN_BEGIN};
        gx_spans_totals totals{};
        gx_group_out keys{};
        gx_spans_out so{};
        auto call = [&](const int32_t* numbers, const uint32_t* roles, uint32_t flags, const gx_spans_out* spans, gx_spans_totals* t) {
            return gx_group_spans(def->handle(), b, off.data(), lines.size(), ids.data(), caps.data(), one, 1, numbers, roles, nullptr, 0, flags, &keys, spans, t, nullptr);
        };
        CHECK(call(nullptr, role, 0, &so, &totals) == GX_E_ARG && std::string(gx_last_error()).find("number_groups is NULL") != std::string::npos);
        CHECK(call(number, role, 0, &so, &totals) == GX_E_ARG && std::string(gx_last_error()).find("number group") != std::string::npos);
        number[0] = 0;
        CHECK(call(number, nullptr, 0, &so, &totals) == GX_E_ARG && std::string(gx_last_error()).find("roles is NULL") != std::string::npos);
        role[0] = 0;
        CHECK(call(number, role, 0, &so, &totals) == GX_E_ARG && std::string(gx_last_error()).find("role is neither") != std::string::npos);
        CHECK(call(number, role, 0, nullptr, &totals) == GX_E_ARG);                           // spans == NULL still checks the roles
        role[0] = GX_SPAN_END;
        CHECK(call(number, role, 4u, &so, &totals) == GX_E_ARG);
        CHECK(call(number, role, 0, &so, nullptr) == GX_E_ARG);
        so.max_spans = (1ull << 30) + 1;
        CHECK(call(number, role, 0, &so, &totals) == GX_E_LIMIT);
        so.max_spans = 0;
        CHECK(gx_text_group_spans(def->handle(), reinterpret_cast<const uint8_t*>(text.data()), text.size(), one, 1, number, nullptr, nullptr, 0, 0, &keys, &so, &totals,
                                  nullptr, nullptr, nullptr) == GX_E_ARG);
        // ... and behind them no device is an error, never a CPU path
        try { def->groupSpans(b, off.data(), lines.size(), ids.data(), caps.data(), byId, &small); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        try { def->textGroupSpans(text, byId); CHECK(false); }
        catch (GorpError& e) { CHECK(e.code == GX_E_DEVICE); }
        number[0] = -1;
        uint64_t room[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        so.span_duration = reinterpret_cast<int64_t*>(room);                                  // durations without a time are legal
        so.max_spans = 8;
        CHECK(call(number, role, GX_GROUP_WEAK_HASH | GX_BY_KEY_ALL_DIGITS, &so, &totals) == GX_E_DEVICE);
        printf("host-only checks ok\n");
        return 0;
    }
    def->extractBatch(b, off.data(), lines.size(), ids.data(), caps.data());
    CHECK((ids == std::vector<int32_t>{0, 0, 0, -1, 1, 1, 1, 0, 1}));
    Gorp::Spans s = def->groupSpans(b, off.data(), lines.size(), ids.data(), caps.data(), byId);
    CHECK((s.keys == std::vector<std::string>{"a", "b", "c", "d"}) && (s.spanKey == std::vector<uint32_t>{0, 1}));
    CHECK((s.spanBeginLine == std::vector<uint32_t>{2, 1}) && (s.spanEndLine == std::vector<uint32_t>{4, 5}));
    CHECK((s.spanBegin == std::vector<int64_t>{110, 105}) && (s.spanEnd == std::vector<int64_t>{140, 90}) && (s.spanDuration == std::vector<int64_t>{30, -15}));
    CHECK((s.spanClass == std::vector<uint8_t>{0, 0}) && (s.keySpanBegin == std::vector<uint64_t>{0, 1, 2, 2, 2}));
    CHECK((s.keyOpenLine == std::vector<uint32_t>{0xFFFFFFFFu, 0xFFFFFFFFu, 7, 0xFFFFFFFFu}));
    CHECK((s.lineSpan == std::vector<uint32_t>{0xFFFFFFFFu, 1, 0, 0xFFFFFFFFu, 0, 1, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}));
    CHECK((s.lineState == std::vector<uint8_t>{3, 1, 1, 0, 2, 2, 5, 4, 5}));
    CHECK(s.spans.n_spans == 2 && s.spans.begins == 4 && s.spans.ends == 4 && s.spans.superseded == 1 && s.spans.left_open == 1 && s.spans.orphan_ends == 2);
    CHECK(s.spans.out_of_range == 0 && s.spans.durations.lines == 2 && s.spans.durations.numbers == 2 && s.spans.durations.min == -15 && s.spans.durations.max == 30);
    CHECK(s.spans.durations.sum_lo == 15 && s.spans.durations.sum_hi == 0 && s.totals.keyed == 8 && s.totals.n_keys == 4);
    CHECK(s.keySpanStats.size() == 4 && s.keySpanStats[0].numbers == 1 && s.keySpanStats[0].sum_lo == 30 && s.keySpanStats[1].min == -15 && s.keySpanStats[2].lines == 0);
    // under a term a's second begin (size 3) does not count: its first begin pairs with the first end
    s = def->groupSpans(b, off.data(), lines.size(), ids.data(), caps.data(), byId, &small);
    CHECK((s.spanBeginLine == std::vector<uint32_t>{0, 1}) && (s.spanDuration == std::vector<int64_t>{40, -15}) && s.lineState[2] == 0 && s.spans.superseded == 0);
    // no part has a time: the spans pair all the same, and every one is class 1
    Gorp::SpanParts untimed = def->spanParts();
    untimed.begin("RequestStart", "id").end("RequestEnd", "id");
    s = def->groupSpans(b, off.data(), lines.size(), ids.data(), caps.data(), untimed);
    CHECK((s.spanEndLine == std::vector<uint32_t>{4, 5}) && (s.spanClass == std::vector<uint8_t>{1, 1}) && (s.spanDuration == std::vector<int64_t>{0, 0}));
    CHECK(s.spans.durations.unset == 2 && s.spans.durations.numbers == 0 && s.spans.n_spans == 2);
    // whole files
    std::vector<uint64_t> counts;
    uint64_t n_lines = 0;
    Gorp::Spans t = def->textGroupSpans(text, byId, nullptr, &counts, &n_lines);
    CHECK(n_lines == lines.size() && (counts == std::vector<uint64_t>{4, 4, 1, 0, 0, 0}));
    CHECK((t.spanKey == std::vector<uint32_t>{0, 1}) && (t.spanDuration == std::vector<int64_t>{30, -15}) && (t.lineState == std::vector<uint8_t>{3, 1, 1, 0, 2, 2, 5, 4, 5}));
    CHECK((t.keys == std::vector<std::string>{"a", "b", "c", "d"}) && t.spans.left_open == 1 && (t.keyOpenLine == std::vector<uint32_t>{0xFFFFFFFFu, 0xFFFFFFFFu, 7, 0xFFFFFFFFu}));
    printf("GPU checks ok\n");
    return 0;
}
