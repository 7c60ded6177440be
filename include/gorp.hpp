// gorp.hpp -- C++ host-side mirror of the reference's API for the match-and-extract path, header-only over the
// C ABI of libgorp_hip.so (include/gorp_hip.h).  Same names, argument meaning and error behaviour as
// salesforce/gorp (core/ = gorp-core/src/main/java/com/salesforce/gorp/):
//
//   gorp::DefinitionReader::reader(text).read()  core/DefinitionReader.java:58-84
//   gorp::Gorp::extract / extractSafe            core/Gorp.java:145-186
//   gorp::ExtractionResult::getId / asMap        core/ExtractionResult.java:39-88
//   gorp::ExtractionException                    core/ExtractionException.java:15-34
//   gorp::DefinitionParseException               core/DefinitionParseException.java
//   gorp::RegexHelper                            core/util/RegexHelper.java
//
// plus the batch entry points the GPU needs (Gorp::extractBatch over a CSR byte buffer, splitLines before it,
// Gorp::resultsToJsonl after it).  All matching runs in the
// HIP kernels; nothing here computes a match on the CPU.  Link: -lgorp_hip -lamdhip64.
#pragma once
#include <cstdint>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "gorp_hip.h"

namespace gorp {

struct DefinitionParseException : std::runtime_error {
    int code;
    DefinitionParseException(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

struct ExtractionException : std::runtime_error {
    std::string input;
    ExtractionException(std::string in, const std::string& m) : std::runtime_error(m), input(std::move(in)) {}
    const std::string& getInput() const { return input; }
};

struct GorpError : std::runtime_error {
    int code;
    GorpError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

// core/model/CookedExtraction.java (data only)
struct CookedExtraction {
    std::string name;
    std::vector<std::string> extractorNames;
    std::string appendJson;  // getExtra() as JSON object text; empty when there is none
    std::vector<std::pair<std::string, std::string>> extra;  // getExtra() entry by entry: key, value as JSON text
    const std::string& getName() const { return name; }
};

// A value of ExtractionResult.asMap(): the captured text, null (Matcher.group() == null), or -- for `append`
// entries, whose values are typed -- JSON text.
struct MapValue {
    enum Kind { Null, String, Json } kind;
    std::string text;
    bool operator==(const char* s) const { return kind == String && text == s; }
};

// core/ExtractionResult.java.  Values are (present, text) because Matcher.group may return null.
class ExtractionResult {
public:
    ExtractionResult(const CookedExtraction* x, std::string input, std::vector<std::pair<bool, std::string>> values)
        : x_(x), input_(std::move(input)), values_(std::move(values)) {}
    const std::string& getId() const { return x_->name; }
    const std::string& getInput() const { return input_; }
    const CookedExtraction& getMatchedExtraction() const { return *x_; }
    // core/ExtractionResult.java:65-88 on a LinkedHashMap: the id (optional) first, every extractor name -> its text
    // or null in group order, then the `append` entries; a key put again keeps its position and takes the new value
    std::vector<std::pair<std::string, MapValue>> asMap(const char* idAs = nullptr) const {
        std::vector<std::pair<std::string, MapValue>> m;
        auto put = [&m](const std::string& key, MapValue v) {
            for (auto& e : m) if (e.first == key) { e.second = std::move(v); return; }
            m.emplace_back(key, std::move(v));
        };
        if (idAs) put(idAs, MapValue{MapValue::String, x_->name});
        for (size_t i = 0; i < values_.size(); ++i)
            put(x_->extractorNames[i], values_[i].first ? MapValue{MapValue::String, values_[i].second} : MapValue{MapValue::Null, ""});
        for (auto& kv : x_->extra) put(kv.first, MapValue{MapValue::Json, kv.second});
        return m;
    }
    bool has(size_t group) const { return group < values_.size() && values_[group].first; }
    const std::string& value(size_t group) const { return values_[group].second; }

private:
    const CookedExtraction* x_;
    std::string input_;
    std::vector<std::pair<bool, std::string>> values_;
};

struct RegexHelper {
    static std::string quoteLiteralAsRegexp(const std::string& t) { return call(gx_quote_literal_as_regexp, t); }
    static std::string massageRegexpForAutomaton(const std::string& p) { return call(gx_massage_regexp_for_automaton, p); }
    static std::string massageRegexpForJDK(const std::string& p) { return call(gx_massage_regexp_for_jdk, p); }

private:
    typedef int (*Fn)(const char*, char*, size_t, size_t*);
    static std::string call(Fn fn, const std::string& in) {
        size_t n = 0;
        std::string out(8 * in.size() + 64, '\0');
        int rc = fn(in.c_str(), &out[0], out.size(), &n);
        if (rc == GX_E_ARG && n + 1 > out.size()) { out.assign(n + 1, '\0'); rc = fn(in.c_str(), &out[0], out.size(), &n); }
        if (rc == GX_E_REGEX_SYNTAX) throw std::invalid_argument(gx_last_error());  // IllegalArgumentException
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        out.resize(n);
        return out;
    }
};

// core/Gorp.java
class Gorp {
public:
    ~Gorp() { gx_destroy(h_); }
    Gorp(const Gorp&) = delete;
    Gorp& operator=(const Gorp&) = delete;

    const std::vector<CookedExtraction>& getExtractions() const { return extractions_; }

    // Gorp.extract(String): the line as UTF-8 (converted to UTF-16 code units, which is what the reference walks).
    // Returns nullptr for "no match"; throws ExtractionException when the matcher and the capture regexp disagree.
    std::unique_ptr<ExtractionResult> extract(const std::string& input, bool allowFallbacks = false) const {
        std::u16string u = to_utf16(input);
        int32_t id = 0;
        std::vector<int32_t> caps(2 * static_cast<size_t>(gx_max_groups(h_)) + 2, -1);
        int rc = gx_extract_one_utf16(h_, reinterpret_cast<const uint16_t*>(u.data()), static_cast<int32_t>(u.size()), &id, caps.data());
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        return materialise(input, u, id, caps.data(), allowFallbacks);
    }
    std::unique_ptr<ExtractionResult> extractSafe(const std::string& input) const { return extract(input, true); }

    // CookedExtraction.match(String) (core/model/CookedExtraction.java:61) for extraction k: its capture regexp alone,
    // no matcher stage; nullptr when the regexp does not match the whole line.
    std::unique_ptr<ExtractionResult> matchExtraction(size_t k, const std::string& input) const {
        std::u16string u = to_utf16(input);
        int32_t matched = 0;
        std::vector<int32_t> caps(2 * static_cast<size_t>(gx_max_groups(h_)) + 2, -1);
        int rc = gx_capture_one_utf16(h_, static_cast<int32_t>(k), reinterpret_cast<const uint16_t*>(u.data()), static_cast<int32_t>(u.size()),
                                      &matched, caps.data());
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        return matched ? materialise(input, u, static_cast<int32_t>(k), caps.data(), false) : nullptr;
    }

    // The batch path: lines as one Latin-1 byte buffer + offsets[n+1]; match_id[n], caps[n * 2*maxGroups()].
    void extractBatch(const uint8_t* bytes, const uint32_t* offsets, uint64_t n, int32_t* match_id, int32_t* caps,
                      const gx_batch_opts* opts = nullptr) const {
        int rc = gx_extract_batch(h_, bytes, offsets, n, match_id, caps, opts);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
    }
    // Result materialisation for a finished batch: asMap(idAs) of every matched line as JSON Lines (gx_results_to_jsonl)
    std::string resultsToJsonl(const uint8_t* bytes, const uint32_t* offsets, uint64_t n, const int32_t* match_id, const int32_t* caps,
                               const char* idAs = nullptr, const gx_batch_opts* opts = nullptr) const {
        uint64_t size = 0;
        int rc = gx_results_to_jsonl(h_, bytes, offsets, n, match_id, caps, idAs, nullptr, 0, &size, nullptr, opts);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        std::string out(static_cast<size_t>(size), '\0');
        rc = gx_results_to_jsonl(h_, bytes, offsets, n, match_id, caps, idAs, reinterpret_cast<uint8_t*>(&out[0]), size, &size, nullptr, opts);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        return out;
    }
    // Whole files: raw text in, JSON Lines of the matched lines out (gx_text_to_jsonl); counts are optional
    std::string textToJsonl(const std::string& text, const char* idAs = nullptr, uint64_t* nLines = nullptr, uint64_t* nMatched = nullptr,
                            uint64_t* nExceptions = nullptr) const {
        uint64_t size = 0;
        const uint8_t* p = reinterpret_cast<const uint8_t*>(text.data());
        int rc = gx_text_to_jsonl(h_, p, text.size(), idAs, nullptr, 0, &size, nLines, nMatched, nExceptions, nullptr);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        std::string out(static_cast<size_t>(size), '\0');
        rc = gx_text_to_jsonl(h_, p, text.size(), idAs, reinterpret_cast<uint8_t*>(&out[0]), size, &size, nLines, nMatched, nExceptions, nullptr);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        return out;
    }
    // Outcomes of a finished batch (gx_count_outcomes / gx_select_lines / gx_text_select).  The outcome index over
    // K = getExtractions().size(): extraction k -> k; no match -> K; exception of extraction k -> K + 1 + k; any other id -> 2K + 1.
    // A want mask has 2K + 1 entries; want(unmatched, exceptions of every extraction, matched lines of these extractions) builds one.
    using Want = std::vector<uint8_t>;
    Want want(bool unmatched, bool exceptions, const std::vector<size_t>& extractions = {}) const {
        const size_t K = extractions_.size();
        Want w(2 * K + 1, 0);
        w[K] = unmatched ? 1 : 0;
        for (size_t k = 0; k < K; ++k) w[K + 1 + k] = exceptions ? 1 : 0;
        for (size_t k : extractions) w.at(k < K ? k : w.size()) = 1;   // (std::out_of_range for an extraction that does not exist)
        return w;
    }
    // lines per outcome index, 2K + 2 entries; ids in the format opts->compact_results names
    std::vector<uint64_t> countOutcomes(const void* ids, uint64_t n, const gx_batch_opts* opts = nullptr) const {
        std::vector<uint64_t> counts(2 * extractions_.size() + 2, 0);
        int rc = gx_count_outcomes(h_, ids, n, counts.data(), opts);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        return counts;
    }
    // The lines `want` names, in input order, as a new batch: their line numbers, bytes and offsets (host buffers, Latin-1, 32-bit
    // offsets, int32 match ids; the C call takes every other layout)
    struct Selection { std::vector<uint32_t> index; std::vector<uint8_t> bytes; std::vector<uint32_t> offsets; };
    Selection selectLines(const uint8_t* bytes, const uint32_t* offsets, uint64_t n, const int32_t* match_id, const Want& want) const {
        if (want.size() != 2 * extractions_.size() + 1) throw GorpError(GX_E_ARG, "selectLines: the want mask has 2K + 1 entries");
        // one pass: no selection is larger than its input
        const uint64_t total = offsets[n] - offsets[0];
        uint64_t k = 0, size = 0;
        Selection s{std::vector<uint32_t>(static_cast<size_t>(n) + 1), std::vector<uint8_t>(static_cast<size_t>(total) + 1), std::vector<uint32_t>(static_cast<size_t>(n) + 1)};
        int rc = gx_select_lines(h_, bytes, offsets, n, match_id, nullptr, want.data(), s.index.data(), s.bytes.data(), s.offsets.data(), nullptr, nullptr, n, total,
                                 &k, &size, nullptr);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        s.index.resize(static_cast<size_t>(k));
        s.bytes.resize(static_cast<size_t>(size));
        s.offsets.resize(static_cast<size_t>(k) + 1);
        return s;
    }
    // Lines by the values they captured (gx_select_lines_where): the terms of a call, built by name.  where().on("GetRequest",
    // "timeTakenInMsec").ge(500) is the caller's Long.parseLong(r.asMap().get("timeTakenInMsec")) >= 500 (README.md:26,63-79).  An
    // extraction or extractor that does not exist, or an extractor name that two groups of the extraction share, is
    // std::invalid_argument (name such a group by its index).  Text is Latin-1 code units, as selectLines' bytes are.
    class Where {
    public:
        explicit Where(const Gorp* g) : g_(g) {}
        Where& on(const std::string& extraction, const std::string& extractor) {
            const size_t k = g_->extractionIndex(extraction);
            const std::vector<std::string>& names = g_->extractions_[k].extractorNames;
            size_t found = names.size(), count = 0;
            for (size_t g = 0; g < names.size(); ++g)
                if (names[g] == extractor) { found = g; ++count; }
            if (count != 1) throw std::invalid_argument("extraction " + extraction + (count ? " has several extractors " : " has no extractor ") + extractor);
            return on(k, found);
        }
        Where& on(size_t extraction, size_t group) {
            if (extraction >= g_->extractions_.size() || group >= g_->extractions_[extraction].extractorNames.size())
                throw std::invalid_argument("no such extraction or group");
            k_ = static_cast<int32_t>(extraction);
            g_at_ = static_cast<int32_t>(group);
            return *this;
        }
        Where& isSet() { return add(GX_WHERE_SET, 0, nullptr, 0); }
        Where& isUnset() { return add(GX_WHERE_SET, 1, nullptr, 0); }
        Where& eq(const std::string& text) { return add(GX_WHERE_EQ, 0, &text, 0); }
        Where& ne(const std::string& text) { return add(GX_WHERE_EQ, 1, &text, 0); }
        Where& startsWith(const std::string& text) { return add(GX_WHERE_PREFIX, 0, &text, 0); }
        Where& endsWith(const std::string& text) { return add(GX_WHERE_SUFFIX, 0, &text, 0); }
        Where& contains(const std::string& text) { return add(GX_WHERE_CONTAINS, 0, &text, 0); }
        Where& notContains(const std::string& text) { return add(GX_WHERE_CONTAINS, 1, &text, 0); }
        Where& eq(int64_t number) { return add(GX_WHERE_INT_EQ, 0, nullptr, number); }
        Where& ne(int64_t number) { return add(GX_WHERE_INT_EQ, 1, nullptr, number); }
        Where& lt(int64_t number) { return add(GX_WHERE_INT_LT, 0, nullptr, number); }
        Where& le(int64_t number) { return add(GX_WHERE_INT_LE, 0, nullptr, number); }
        Where& gt(int64_t number) { return add(GX_WHERE_INT_GT, 0, nullptr, number); }
        Where& ge(int64_t number) { return add(GX_WHERE_INT_GE, 0, nullptr, number); }
        // the terms as the C call takes them (the pointers live as long as this object is not changed)
        std::vector<gx_where_term> terms() const {
            std::vector<gx_where_term> out = terms_;
            for (size_t t = 0; t < out.size(); ++t) {
                out[t].text = texts_[t].empty() ? nullptr : texts_[t].data();
                out[t].text_units = static_cast<uint32_t>(texts_[t].size());
            }
            return out;
        }
        // the mask that marks exactly the extractions that have terms
        Want want() const {
            Want w(2 * g_->extractions_.size() + 1, 0);
            for (const gx_where_term& t : terms_) w[static_cast<size_t>(t.extraction)] = 1;
            return w;
        }

    private:
        Where& add(uint32_t op, uint32_t negate, const std::string* text, int64_t number) {
            if (k_ < 0) throw std::invalid_argument("Where: on(extraction, extractor) first");
            gx_where_term t{};
            t.extraction = k_; t.group = g_at_; t.op = op; t.negate = negate; t.number = number;
            terms_.push_back(t);
            texts_.push_back(text ? *text : std::string());
            return *this;
        }
        const Gorp* g_;
        int32_t k_ = -1, g_at_ = 0;
        std::vector<gx_where_term> terms_;
        std::vector<std::string> texts_;
    };
    Where where() const { return Where(this); }
    size_t extractionIndex(const std::string& name) const {
        for (size_t k = 0; k < extractions_.size(); ++k)
            if (extractions_[k].name == name) return k;
        throw std::invalid_argument("no extraction " + name);
    }
    // selectLines with terms: of the lines of an extraction that has terms only those on which every term holds; caps: the dense capture
    // rows of the batch (extractBatch's)
    Selection selectLinesWhere(const uint8_t* bytes, const uint32_t* offsets, uint64_t n, const int32_t* match_id, const int32_t* caps, const Want& want,
                               const Where& where) const {
        if (want.size() != 2 * extractions_.size() + 1) throw GorpError(GX_E_ARG, "selectLinesWhere: the want mask has 2K + 1 entries");
        const std::vector<gx_where_term> terms = where.terms();
        const uint64_t total = offsets[n] - offsets[0];
        uint64_t k = 0, size = 0;
        Selection s{std::vector<uint32_t>(static_cast<size_t>(n) + 1), std::vector<uint8_t>(static_cast<size_t>(total) + 1), std::vector<uint32_t>(static_cast<size_t>(n) + 1)};
        int rc = gx_select_lines_where(h_, bytes, offsets, n, match_id, caps, want.data(), terms.data(), static_cast<uint32_t>(terms.size()), s.index.data(),
                                       s.bytes.data(), s.offsets.data(), nullptr, nullptr, n, total, &k, &size, nullptr);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        s.index.resize(static_cast<size_t>(k));
        s.bytes.resize(static_cast<size_t>(size));
        s.offsets.resize(static_cast<size_t>(k) + 1);
        return s;
    }
    // How a group is read as a number (gx_set_number_format): setNumberFormat("Syslog", "ts", {GX_NUMBER_ISO8601, 3}) makes every
    // integer term, measure and value group on it the caller's Instant.parse(r.asMap().get("ts")).toEpochMilli().  Names resolve as
    // Where's do.  Not thread-safe against calls on the same Gorp.
    void setNumberFormat(const std::string& extraction, const std::string& extractor, gx_number_format format) {
        Where at(this);
        at.on(extraction, extractor).isSet();
        const gx_where_term t = at.terms()[0];
        if (gx_set_number_format(h_, t.extraction, t.group, &format) != GX_OK) throw GorpError(GX_E_ARG, gx_last_error());
    }
    gx_number_format numberFormat(const std::string& extraction, const std::string& extractor) const {
        Where at(this);
        at.on(extraction, extractor).isSet();
        const gx_where_term t = at.terms()[0];
        gx_number_format f{};
        if (gx_get_number_format(h_, t.extraction, t.group, &f) != GX_OK) throw GorpError(GX_E_ARG, gx_last_error());
        return f;
    }
    // Captured numbers, summarised (gx_capture_stats): the measures of a call, built by name.  measures().of("GetRequest",
    // "timeTakenInMsec", {10, 100, 500, 1000}) is the caller's metrics.record(Long.parseLong(r.asMap().get("timeTakenInMsec")))
    // (README.md:26,63-79) with a latency histogram.  Names resolve as Where's do; edges are strictly ascending, at most 64.
    class Measures {
    public:
        explicit Measures(const Gorp* g) : g_(g) {}
        Measures& of(const std::string& extraction, const std::string& extractor, const std::vector<int64_t>& edges = {}) {
            Where at(g_);
            at.on(extraction, extractor).isSet();
            const gx_where_term t = at.terms()[0];
            return of(static_cast<size_t>(t.extraction), static_cast<size_t>(t.group), edges);
        }
        Measures& of(size_t extraction, size_t group, const std::vector<int64_t>& edges = {}) {
            if (extraction >= g_->extractions_.size() || group >= g_->extractions_[extraction].extractorNames.size())
                throw std::invalid_argument("no such extraction or group");
            gx_measure m{};
            m.extraction = static_cast<int32_t>(extraction);
            m.group = static_cast<int32_t>(group);
            measures_.push_back(m);
            edges_.push_back(edges);
            return *this;
        }
        // the measures as the C call takes them (the pointers live as long as this object is not changed)
        std::vector<gx_measure> measures() const {
            std::vector<gx_measure> out = measures_;
            for (size_t t = 0; t < out.size(); ++t) {
                out[t].edges = edges_[t].empty() ? nullptr : edges_[t].data();
                out[t].n_edges = static_cast<uint32_t>(edges_[t].size());
            }
            return out;
        }
        size_t bins() const {
            size_t b = 0;
            for (const std::vector<int64_t>& e : edges_) b += e.size() + 1;
            return b;
        }

    private:
        const Gorp* g_;
        std::vector<gx_measure> measures_;
        std::vector<std::vector<int64_t>> edges_;
    };
    Measures measures() const { return Measures(this); }
    // One measure's summary: gx_measure_stats (lines, numbers, unset, not_numbers, min, max, and the exact sum as the 128-bit
    // two's-complement integer sum_hi : sum_lo) and its n_edges + 1 histogram buckets.
    struct MeasureStats { gx_measure_stats stats; std::vector<uint64_t> hist; };
    // of the batch's lines (host buffers, Latin-1, 32-bit offsets, int32 match ids and dense capture rows; the C call takes every other
    // layout), per measure: those of its extraction on which every term of `where` holds, classed by what the group captured
    std::vector<MeasureStats> captureStats(const uint8_t* bytes, const uint32_t* offsets, uint64_t n, const int32_t* match_id, const int32_t* caps,
                                           const Measures& measures, const Where* where = nullptr) const {
        const std::vector<gx_measure> m = measures.measures();
        const std::vector<gx_where_term> terms = where ? where->terms() : std::vector<gx_where_term>();
        std::vector<gx_measure_stats> stats(m.size() + 1);
        std::vector<uint64_t> hist(measures.bins() + 1, 0);
        int rc = gx_capture_stats(h_, bytes, offsets, n, match_id, caps, m.data(), static_cast<uint32_t>(m.size()), terms.data(), static_cast<uint32_t>(terms.size()),
                                  stats.data(), hist.data(), nullptr);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        return statsOf(m, stats, hist);
    }
    // Whole files: raw text in, the same summary out (gx_text_capture_stats).  counts (optional): lines per outcome index.
    std::vector<MeasureStats> textCaptureStats(const std::string& text, const Measures& measures, const Where* where = nullptr,
                                               std::vector<uint64_t>* counts = nullptr, uint64_t* nLines = nullptr, bool utf8 = false) const {
        const std::vector<gx_measure> m = measures.measures();
        const std::vector<gx_where_term> terms = where ? where->terms() : std::vector<gx_where_term>();
        std::vector<gx_measure_stats> stats(m.size() + 1);
        std::vector<uint64_t> hist(measures.bins() + 1, 0);
        if (counts) counts->assign(2 * extractions_.size() + 2, 0);
        gx_batch_opts o{};
        o.struct_size = sizeof(o);
        o.utf8 = utf8 ? 1u : 0u;
        int rc = gx_text_capture_stats(h_, reinterpret_cast<const uint8_t*>(text.data()), text.size(), m.data(), static_cast<uint32_t>(m.size()), terms.data(),
                                       static_cast<uint32_t>(terms.size()), stats.data(), hist.data(), counts ? counts->data() : nullptr, nLines, utf8 ? &o : nullptr);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        return statsOf(m, stats, hist);
    }
    // Lines grouped by the text they captured (gx_group_lines): the parts of a call, built by name.  groupParts().of("GetRequest",
    // "verb").of("OtherRequest", "verb") is the caller's byVerb.merge(r.asMap().get("verb"), 1L, Long::sum) (README.md:26,63-79);
    // of("GetRequest", "path", "timeTakenInMsec") also measures a number per key.  Names resolve as Where's do; one part per extraction.
    class GroupParts {
    public:
        explicit GroupParts(const Gorp* g) : g_(g) {}
        GroupParts& of(const std::string& extraction, const std::string& key, const std::string& value = std::string()) {
            Where at(g_);
            at.on(extraction, key).isSet();
            const gx_where_term k = at.terms()[0];
            int32_t v = -1;
            if (!value.empty()) {
                at.on(extraction, value).isSet();
                v = at.terms()[1].group;
            }
            return of(static_cast<size_t>(k.extraction), static_cast<size_t>(k.group), v);
        }
        GroupParts& of(size_t extraction, size_t keyGroup, int32_t valueGroup = -1) {
            if (extraction >= g_->extractions_.size() || keyGroup >= g_->extractions_[extraction].extractorNames.size() || valueGroup < -1 ||
                (valueGroup >= 0 && static_cast<size_t>(valueGroup) >= g_->extractions_[extraction].extractorNames.size()))
                throw std::invalid_argument("no such extraction or group");
            for (const gx_group_part& p : parts_)
                if (p.extraction == static_cast<int32_t>(extraction)) throw std::invalid_argument("two parts for one extraction");
            gx_group_part p{};
            p.extraction = static_cast<int32_t>(extraction);
            p.key_group = static_cast<int32_t>(keyGroup);
            p.value_group = valueGroup;
            parts_.push_back(p);
            return *this;
        }
        const std::vector<gx_group_part>& parts() const { return parts_; }
        bool hasValues() const {
            for (const gx_group_part& p : parts_)
                if (p.value_group >= 0) return true;
            return false;
        }

    private:
        const Gorp* g_;
        std::vector<gx_group_part> parts_;
    };
    GroupParts groupParts() const { return GroupParts(this); }
    // The groups of a call: the distinct keys in the order of their first line (a LinkedHashMap's insertion order), per key its first
    // line, its lines and -- when a part has a value -- its gx_measure_stats; per input line its key's number (0xFFFFFFFF: none).
    struct Groups {
        std::vector<std::string> keys;
        std::vector<uint32_t> firstLine;
        std::vector<uint64_t> lines;
        std::vector<gx_measure_stats> stats;   // empty when no part has a value
        std::vector<uint32_t> lineKey;
        gx_group_totals totals{};
    };
    // of the batch's lines (host buffers, Latin-1, 32-bit offsets, int32 match ids and dense capture rows; the C call takes every other
    // layout): those whose extraction has a part and on which every term of `where` holds, grouped by the part's key
    Groups groupLines(const uint8_t* bytes, const uint32_t* offsets, uint64_t n, const int32_t* match_id, const int32_t* caps, const GroupParts& parts,
                      const Where* where = nullptr) const {
        return groupsOf(parts, where, &n, [&](const gx_group_part* p, uint32_t np, const gx_where_term* t, uint32_t nt, const gx_group_out* out, gx_group_totals* totals) {
            return gx_group_lines(h_, bytes, offsets, n, match_id, caps, p, np, t, nt, 0, out, totals, nullptr);
        });
    }
    // Whole files: raw text in, the same groups out (gx_text_group_lines).  counts (optional): lines per outcome index.
    Groups textGroupLines(const std::string& text, const GroupParts& parts, const Where* where = nullptr, std::vector<uint64_t>* counts = nullptr,
                          uint64_t* nLines = nullptr, bool utf8 = false) const {
        if (counts) counts->assign(2 * extractions_.size() + 2, 0);
        gx_batch_opts o{};
        o.struct_size = sizeof(o);
        o.utf8 = utf8 ? 1u : 0u;
        uint64_t lines = 0;
        Groups g = groupsOf(parts, where, &lines, [&](const gx_group_part* p, uint32_t np, const gx_where_term* t, uint32_t nt, const gx_group_out* out,
                                                      gx_group_totals* totals) {
            return gx_text_group_lines(h_, reinterpret_cast<const uint8_t*>(text.data()), text.size(), p, np, t, nt, 0, out, totals, counts ? counts->data() : nullptr,
                                       &lines, utf8 ? &o : nullptr);
        });
        if (nLines) *nLines = lines;
        return g;
    }
    // Every key's lines together (gx_lines_by_key): the caller's byRequest.computeIfAbsent(r.asMap().get("requestId"), k -> new
    // ArrayList<>()).add(line) (README.md:26,63-79).  groupLines' result for every key, kept or not, plus the lines of the keys that have
    // minLines .. maxLines lines (maxLines 0: no upper bound; 1, 1: the keys with a single line) as a new batch ordered by (key number,
    // input line): key j's lines are the output lines keyOutLines[j] .. keyOutLines[j + 1], its bytes bytes[keyOutUnits[j] ..
    // keyOutUnits[j + 1]).  ids / caps: the kept lines' match ids and capture rows (textLinesByKey: empty; index holds lines of the text).
    struct LinesByKey : Groups {
        std::vector<uint32_t> index;
        std::vector<uint8_t> bytes;
        std::vector<uint32_t> offsets;
        std::vector<int32_t> ids, caps;
        std::vector<uint64_t> keyOutLines, keyOutUnits;
        gx_by_key_totals byKey{};
    };
    LinesByKey linesByKey(const uint8_t* bytes, const uint32_t* offsets, uint64_t n, const int32_t* match_id, const int32_t* caps, const GroupParts& parts,
                          uint64_t minLines = 1, uint64_t maxLines = 0, const Where* where = nullptr) const {
        LinesByKey r;
        const size_t slots = 2 * static_cast<size_t>(gx_max_groups(h_));
        Groups g = groupsOf(parts, where, &n, [&](const gx_group_part* p, uint32_t np, const gx_where_term* t, uint32_t nt, const gx_group_out* out, gx_group_totals* totals) {
            gx_by_key_out b{};
            const bool deliver = out->key_offsets != nullptr;   // (the size query before it left the sizes in r.byKey)
            if (deliver) {
                const size_t m = static_cast<size_t>(r.byKey.lines_out);
                r.index.assign(m, 0);
                r.bytes.assign(static_cast<size_t>(r.byKey.units_out) + 1, 0);
                r.offsets.assign(m + 1, 0);
                r.ids.assign(m, 0);
                r.caps.assign(m * slots + 1, 0);
                r.keyOutLines.assign(static_cast<size_t>(out->max_keys) + 1, 0);
                r.keyOutUnits.assign(static_cast<size_t>(out->max_keys) + 1, 0);
                b.out_index = r.index.data(); b.out_bytes = r.bytes.data(); b.out_offsets = r.offsets.data(); b.out_ids = r.ids.data();
                b.out_caps = caps && slots ? r.caps.data() : nullptr;
                b.cap_lines = m; b.out_bytes_cap = r.byKey.units_out;
                b.key_out_lines = r.keyOutLines.data(); b.key_out_units = r.keyOutUnits.data();
            }
            const int rc = gx_lines_by_key(h_, bytes, offsets, n, match_id, caps, p, np, t, nt, minLines, maxLines, 0, out, deliver ? &b : nullptr, &r.byKey, nullptr);
            *totals = r.byKey.group;
            return rc;
        });
        static_cast<Groups&>(r) = std::move(g);
        r.bytes.resize(static_cast<size_t>(r.byKey.units_out));
        r.caps.resize(caps ? r.index.size() * slots : 0);
        return r;
    }
    // Whole files: raw text in, the same regrouping out (gx_text_lines_by_key); bytes holds the kept lines' original bytes, cut at offsets.
    LinesByKey textLinesByKey(const std::string& text, const GroupParts& parts, uint64_t minLines = 1, uint64_t maxLines = 0, const Where* where = nullptr,
                              std::vector<uint64_t>* counts = nullptr, uint64_t* nLines = nullptr, bool utf8 = false) const {
        if (counts) counts->assign(2 * extractions_.size() + 2, 0);
        gx_batch_opts o{};
        o.struct_size = sizeof(o);
        o.utf8 = utf8 ? 1u : 0u;
        uint64_t lines = 0;
        LinesByKey r;
        Groups g = groupsOf(parts, where, &lines, [&](const gx_group_part* p, uint32_t np, const gx_where_term* t, uint32_t nt, const gx_group_out* out,
                                                      gx_group_totals* totals) {
            const bool deliver = out->key_offsets != nullptr;
            if (deliver) {
                r.index.assign(static_cast<size_t>(r.byKey.lines_out), 0);
                r.bytes.assign(static_cast<size_t>(r.byKey.units_out) + 1, 0);
                r.offsets.assign(static_cast<size_t>(r.byKey.lines_out) + 1, 0);
                r.keyOutLines.assign(static_cast<size_t>(out->max_keys) + 1, 0);
                r.keyOutUnits.assign(static_cast<size_t>(out->max_keys) + 1, 0);
            }
            const uint64_t cap = r.byKey.units_out;
            const int rc = gx_text_lines_by_key(h_, reinterpret_cast<const uint8_t*>(text.data()), text.size(), p, np, t, nt, minLines, maxLines, 0, out,
                                                deliver ? r.bytes.data() : nullptr, cap, deliver ? r.offsets.data() : nullptr, deliver ? r.index.data() : nullptr,
                                                deliver ? r.keyOutLines.data() : nullptr, deliver ? r.keyOutUnits.data() : nullptr, &r.byKey,
                                                counts ? counts->data() : nullptr, &lines, utf8 ? &o : nullptr);
            *totals = r.byKey.group;
            return rc;
        });
        static_cast<Groups&>(r) = std::move(g);
        r.bytes.resize(static_cast<size_t>(r.byKey.units_out));
        if (nLines) *nLines = lines;
        return r;
    }
    // Captured texts looked up in a dictionary of the caller's (gx_lookup_lines): the caller's wanted.contains(r.asMap().get("user")) and
    // meta = byHost.get(r.asMap().get("host")) (README.md:26,63-79).  Parts are groupParts'; entries are the dictionary's texts, and the
    // lowest of several equal entries stands for them all (entrySame).  lineEntry: per input line the entry its key equals,
    // GX_LOOKUP_MISS or GX_LOOKUP_NONE; entryLines, entryFirstLine and -- when a part has a value -- entryStats per entry.  With keep the
    // kept lines leave in input order as a new batch (index, bytes, offsets, ids, caps; textLookupLines: ids and caps stay empty and index
    // holds lines of the text).
    struct Lookup {
        std::vector<uint32_t> lineEntry, entrySame;
        std::vector<uint64_t> entryLines;
        std::vector<uint32_t> entryFirstLine;
        std::vector<gx_measure_stats> entryStats;   // empty when no part has a value
        std::vector<uint32_t> index;
        std::vector<uint8_t> bytes;
        std::vector<uint32_t> offsets;
        std::vector<int32_t> ids, caps;
        gx_lookup_totals totals{};
    };
    Lookup lookupLines(const uint8_t* bytes, const uint32_t* offsets, uint64_t n, const int32_t* match_id, const int32_t* caps, const GroupParts& parts,
                       const std::vector<std::string>& entries, uint32_t keep = GX_LOOKUP_KEEP_NOTHING, const Where* where = nullptr) const {
        const size_t slots = 2 * static_cast<size_t>(gx_max_groups(h_));
        return lookupOf(parts, entries, keep, where, n, [&](const gx_group_part* p, uint32_t np, const gx_where_term* t, uint32_t nt, const void* eu, const void* eo,
                                                             Lookup& r, bool deliver) {
            gx_lookup_out out = lookupOut(r, deliver);
            if (deliver && keep != GX_LOOKUP_KEEP_NOTHING) {
                const size_t m = static_cast<size_t>(r.totals.lines_out);
                r.ids.assign(m + 1, 0);
                r.caps.assign(m * slots + 1, 0);
                out.out_index = r.index.data(); out.out_bytes = r.bytes.data(); out.out_offsets = r.offsets.data(); out.out_ids = r.ids.data();
                out.out_caps = caps && slots ? r.caps.data() : nullptr;
                out.cap_lines = m; out.out_bytes_cap = r.totals.units_out;
            }
            const int rc = gx_lookup_lines(h_, bytes, offsets, n, match_id, caps, p, np, t, nt, eu, eo, entries.size(), keep, 0, deliver ? &out : nullptr, &r.totals, nullptr);
            if (deliver) {
                r.ids.resize(static_cast<size_t>(r.totals.lines_out));
                r.caps.resize(caps ? r.ids.size() * slots : 0);
            }
            return rc;
        });
    }
    // Whole files: raw text in, the same lookup out (gx_text_lookup_lines); bytes holds the kept lines' original bytes, cut at offsets.
    Lookup textLookupLines(const std::string& text, const GroupParts& parts, const std::vector<std::string>& entries, uint32_t keep = GX_LOOKUP_KEEP_NOTHING,
                           const Where* where = nullptr, std::vector<uint64_t>* counts = nullptr, uint64_t* nLines = nullptr, bool utf8 = false) const {
        if (counts) counts->assign(2 * extractions_.size() + 2, 0);
        gx_batch_opts o{};
        o.struct_size = sizeof(o);
        o.utf8 = utf8 ? 1u : 0u;
        uint64_t lines = 0;
        for (char c : text) lines += (c == '\n' || c == '\r') ? 1u : 0u;   // (no more lines than line ends, plus the last)
        Lookup r = lookupOf(parts, entries, keep, where, lines + 1, [&](const gx_group_part* p, uint32_t np, const gx_where_term* t, uint32_t nt, const void* eu,
                                                                         const void* eo, Lookup& l, bool deliver) {
            const gx_lookup_out out = lookupOut(l, deliver);
            const bool kept = deliver && keep != GX_LOOKUP_KEEP_NOTHING;
            return gx_text_lookup_lines(h_, reinterpret_cast<const uint8_t*>(text.data()), text.size(), p, np, t, nt, eu, eo, entries.size(), keep, 0,
                                        deliver ? &out : nullptr, kept ? l.bytes.data() : nullptr, l.totals.units_out, kept ? l.offsets.data() : nullptr,
                                        kept ? l.index.data() : nullptr, &l.totals, counts ? counts->data() : nullptr, &lines, utf8 ? &o : nullptr);
        });
        r.lineEntry.resize(static_cast<size_t>(lines));
        if (nLines) *nLines = lines;
        return r;
    }
    // Lines grouped by TWO captured texts (gx_group_pairs): the caller's seen.computeIfAbsent(r.asMap().get("verb"), v -> new
    // HashSet<>()).add(r.asMap().get("path")) and byBoth.merge(List.of(verb, path), 1L, Long::sum) (README.md:26,63-79).  The parts of a
    // call are groupParts' plus a SECOND extractor per part (an empty name, or -1: the part's lines have a key and no second):
    // pairParts().of("GetRequest", "verb", "path").of("OtherRequest", "verb", "path").
    class PairParts {
    public:
        explicit PairParts(const Gorp* g) : g_(g), keys_(g) {}
        PairParts& of(const std::string& extraction, const std::string& key, const std::string& second, const std::string& value = std::string()) {
            int32_t s = -1;
            if (!second.empty()) {
                Where at(g_);
                at.on(extraction, second).isSet();
                s = at.terms()[0].group;
            }
            keys_.of(extraction, key, value);
            seconds_.push_back(s);
            return *this;
        }
        PairParts& of(size_t extraction, size_t keyGroup, int32_t secondGroup, int32_t valueGroup = -1) {
            if (secondGroup < -1 || (extraction < g_->extractions_.size() && secondGroup >= 0 &&
                                     static_cast<size_t>(secondGroup) >= g_->extractions_[extraction].extractorNames.size()))
                throw std::invalid_argument("no such extraction or group");
            keys_.of(extraction, keyGroup, valueGroup);
            seconds_.push_back(secondGroup);
            return *this;
        }
        const GroupParts& keys() const { return keys_; }
        const std::vector<int32_t>& seconds() const { return seconds_; }

    private:
        const Gorp* g_;
        GroupParts keys_;
        std::vector<int32_t> seconds_;
    };
    PairParts pairParts() const { return PairParts(this); }
    // groupLines' result, plus the distinct pairs (key, second) in the order of their first line: per pair its key's number, its second,
    // its first line and its lines; per key its pairs (its distinct seconds); per input line its pair's number (0xFFFFFFFF: none).
    struct Pairs : Groups {
        std::vector<uint32_t> pairKey;
        std::vector<std::string> seconds;
        std::vector<uint32_t> pairFirstLine;
        std::vector<uint64_t> pairLines, keyPairs;
        std::vector<uint32_t> linePair;
        gx_pairs_totals pairs{};
    };
    Pairs groupPairs(const uint8_t* bytes, const uint32_t* offsets, uint64_t n, const int32_t* match_id, const int32_t* caps, const PairParts& parts,
                     const Where* where = nullptr) const {
        return pairsOf(parts, where, &n, n, [&](const gx_group_part* p, uint32_t np, const int32_t* s, const gx_where_term* t, uint32_t nt, const gx_group_out* out,
                                                const gx_pairs_out* po, gx_pairs_totals* totals) {
            return gx_group_pairs(h_, bytes, offsets, n, match_id, caps, p, np, s, t, nt, 0, out, po, totals, nullptr);
        });
    }
    // Whole files: raw text in, the same pairs out (gx_text_group_pairs).  counts (optional): lines per outcome index.
    Pairs textGroupPairs(const std::string& text, const PairParts& parts, const Where* where = nullptr, std::vector<uint64_t>* counts = nullptr,
                         uint64_t* nLines = nullptr, bool utf8 = false) const {
        if (counts) counts->assign(2 * extractions_.size() + 2, 0);
        gx_batch_opts o{};
        o.struct_size = sizeof(o);
        o.utf8 = utf8 ? 1u : 0u;
        uint64_t lines = 0, ends = 1;   // (no more lines than line ends, plus the last)
        for (const char c : text) ends += (c == '\n' || c == '\r') ? 1u : 0u;
        Pairs r = pairsOf(parts, where, &lines, ends, [&](const gx_group_part* p, uint32_t np, const int32_t* s, const gx_where_term* t, uint32_t nt,
                                                         const gx_group_out* out, const gx_pairs_out* po, gx_pairs_totals* totals) {
            return gx_text_group_pairs(h_, reinterpret_cast<const uint8_t*>(text.data()), text.size(), p, np, s, t, nt, 0, out, po, totals,
                                       counts ? counts->data() : nullptr, &lines, utf8 ? &o : nullptr);
        });
        if (nLines) *nLines = lines;
        return r;
    }
    // Lines counted and measured per interval of a captured number (gx_bucket_lines): the caller's
    //     long b = Math.floorDiv(Instant.parse(r.asMap().get("ts")).toEpochMilli() - origin, 60_000L);
    //     perMinute.merge(b, 1L, Long::sum); latency.computeIfAbsent(b, x -> new Stats()).record(Long.parseLong(...));
    // (README.md:26,63-79, with a timestamp field).  The parts of a call, built by name: bucketParts().of("Syslog", "ts") or
    // .of("GetRequest", "ts", "timeTakenInMsec"), which also measures a number per bucket.  The number is read under its group's number
    // format (gx_set_number_format).  Names resolve as Where's do; one part per extraction; all parts share one bucket space.
    class BucketParts {
    public:
        explicit BucketParts(const Gorp* g) : groups_(g) {}
        BucketParts& of(const std::string& extraction, const std::string& number, const std::string& value = std::string()) {
            groups_.of(extraction, number, value);
            return *this;
        }
        BucketParts& of(size_t extraction, size_t numberGroup, int32_t valueGroup = -1) {
            groups_.of(extraction, numberGroup, valueGroup);
            return *this;
        }
        std::vector<gx_bucket_part> parts() const {
            std::vector<gx_bucket_part> out;
            for (const gx_group_part& p : groups_.parts()) out.push_back(gx_bucket_part{p.extraction, p.key_group, p.value_group, 0});
            return out;
        }
        bool hasValues() const { return groups_.hasValues(); }

    private:
        GroupParts groups_;
    };
    BucketParts bucketParts() const { return BucketParts(this); }
    // The occupied buckets b = floor((number - origin) / width) in ascending order: per bucket its number, its first line, its lines and --
    // when a part has a value -- its gx_measure_stats; per input line the index of its bucket (0xFFFFFFFF: none).
    struct Buckets {
        std::vector<int64_t> bucketNumber;
        std::vector<uint32_t> firstLine;
        std::vector<uint64_t> lines;
        std::vector<gx_measure_stats> stats;   // empty when no part has a value
        std::vector<uint32_t> lineBucket;
        gx_bucket_totals totals{};
    };
    Buckets bucketLines(const uint8_t* bytes, const uint32_t* offsets, uint64_t n, const int32_t* match_id, const int32_t* caps, const BucketParts& parts,
                        int64_t width, int64_t origin = 0, const Where* where = nullptr) const {
        return bucketsOf(parts, where, &n, [&](const gx_bucket_part* p, uint32_t np, const gx_where_term* t, uint32_t nt, const gx_bucket_out* out,
                                               gx_bucket_totals* totals) {
            return gx_bucket_lines(h_, bytes, offsets, n, match_id, caps, p, np, origin, width, t, nt, 0, out, totals, nullptr);
        });
    }
    // Whole files: raw text in, the same buckets out (gx_text_bucket_lines).  counts (optional): lines per outcome index.
    Buckets textBucketLines(const std::string& text, const BucketParts& parts, int64_t width, int64_t origin = 0, const Where* where = nullptr,
                            std::vector<uint64_t>* counts = nullptr, uint64_t* nLines = nullptr, bool utf8 = false) const {
        if (counts) counts->assign(2 * extractions_.size() + 2, 0);
        gx_batch_opts o{};
        o.struct_size = sizeof(o);
        o.utf8 = utf8 ? 1u : 0u;
        uint64_t lines = 0;
        Buckets b = bucketsOf(parts, where, &lines, [&](const gx_bucket_part* p, uint32_t np, const gx_where_term* t, uint32_t nt, const gx_bucket_out* out,
                                                        gx_bucket_totals* totals) {
            return gx_text_bucket_lines(h_, reinterpret_cast<const uint8_t*>(text.data()), text.size(), p, np, origin, width, t, nt, 0, out, totals,
                                        counts ? counts->data() : nullptr, &lines, utf8 ? &o : nullptr);
        });
        if (nLines) *nLines = lines;
        return b;
    }
    // Lines ranked by a number they captured (gx_top_lines): the parts of a call, built by name.  topParts().of("GetRequest",
    // "timeTakenInMsec").of("OtherRequest", "timeTakenInMsec") with topLines(..., 10) is the caller's "which requests were the slowest?",
    // sorted(results, by timeTakenInMsec).take(10) (README.md:26,63-79).  Names resolve as Where's do; one part per extraction; all
    // parts share one number space.
    class TopParts {
    public:
        explicit TopParts(const Gorp* g) : g_(g) {}
        TopParts& of(const std::string& extraction, const std::string& value) {
            Where at(g_);
            at.on(extraction, value).isSet();
            const gx_where_term t = at.terms()[0];
            return of(static_cast<size_t>(t.extraction), static_cast<size_t>(t.group));
        }
        TopParts& of(size_t extraction, size_t valueGroup) {
            if (extraction >= g_->extractions_.size() || valueGroup >= g_->extractions_[extraction].extractorNames.size())
                throw std::invalid_argument("no such extraction or group");
            for (const gx_top_part& p : parts_)
                if (p.extraction == static_cast<int32_t>(extraction)) throw std::invalid_argument("two parts for one extraction");
            parts_.push_back(gx_top_part{static_cast<int32_t>(extraction), static_cast<int32_t>(valueGroup)});
            return *this;
        }
        const std::vector<gx_top_part>& parts() const { return parts_; }

    private:
        const Gorp* g_;
        std::vector<gx_top_part> parts_;
    };
    TopParts topParts() const { return TopParts(this); }
    // The ranked lines of a call, ordered by (value descending -- ascending for the smallest --, input line ascending): their input line
    // numbers, their numbers, and the lines themselves as a batch (topLines: bytes + offsets) or as text (textTopLines: bytes alone,
    // each line with its terminator).
    struct Top {
        std::vector<uint32_t> index;
        std::vector<int64_t> values;
        std::vector<uint8_t> bytes;
        std::vector<uint32_t> offsets;
        gx_top_totals totals{};
    };
    // of the batch's lines (host buffers, Latin-1, 32-bit offsets, int32 match ids and dense capture rows; the C call takes every other
    // layout): the n whose extraction has a part, on which every term of `where` holds and whose value is a number, largest first
    Top topLines(const uint8_t* bytes, const uint32_t* offsets, uint64_t n, const int32_t* match_id, const int32_t* caps, const TopParts& parts, uint32_t wanted,
                 bool largest = true, const Where* where = nullptr) const {
        return topOf(parts, where, [&](const gx_top_part* p, uint32_t np, const gx_where_term* t, uint32_t nt, Top& out, bool deliver) {
            out.offsets.resize(out.index.size() + 1);
            return gx_top_lines(h_, bytes, offsets, n, match_id, caps, p, np, t, nt, wanted, largest ? 0u : GX_TOP_SMALLEST, deliver ? out.index.data() : nullptr,
                                deliver ? out.values.data() : nullptr, deliver ? out.bytes.data() : nullptr, deliver ? out.offsets.data() : nullptr, nullptr, nullptr,
                                out.index.size(), out.bytes.size(), &out.totals, nullptr);
        });
    }
    // Whole files: raw text in, the same ranking out (gx_text_top_lines).  counts (optional): lines per outcome index.
    Top textTopLines(const std::string& text, const TopParts& parts, uint32_t wanted, bool largest = true, const Where* where = nullptr,
                     std::vector<uint64_t>* counts = nullptr, uint64_t* nLines = nullptr, bool utf8 = false) const {
        if (counts) counts->assign(2 * extractions_.size() + 2, 0);
        gx_batch_opts o{};
        o.struct_size = sizeof(o);
        o.utf8 = utf8 ? 1u : 0u;
        return topOf(parts, where, [&](const gx_top_part* p, uint32_t np, const gx_where_term* t, uint32_t nt, Top& out, bool deliver) {
            uint64_t size = 0;
            out.index.resize(wanted);    // (the whole-file call's per-line outputs have room for `wanted` entries)
            out.values.resize(wanted);
            return gx_text_top_lines(h_, reinterpret_cast<const uint8_t*>(text.data()), text.size(), p, np, t, nt, wanted, largest ? 0u : GX_TOP_SMALLEST,
                                     deliver ? out.index.data() : nullptr, deliver ? out.values.data() : nullptr, deliver ? out.bytes.data() : nullptr,
                                     out.bytes.size(), &size, &out.totals, counts ? counts->data() : nullptr, nLines, utf8 ? &o : nullptr);
        });
    }
    // A whole batch ordered by a number its lines captured (gx_sort_lines): the caller's results.sort(Comparator.comparingLong(r ->
    // Instant.parse(r.asMap().get("ts")).toEpochMilli())) (README.md:26,63-79) -- two hosts' logs as one timeline.  The lines leave by
    // (value, input line), descending by (value descending, input line); with carry a line without a number of its own travels with the
    // nearest earlier line that has one (stack traces kept with their line); with restLast the remaining lines follow in input order,
    // else they are dropped.  index: the input line of every output line; values: their numbers (a carried line's is its header's, a rest
    // line's 0); lineClass: 0 own number, 1 carried, 2 rest; bytes / offsets: the lines as a batch; ids / caps: their match ids and
    // capture rows (textSortLines: empty; index holds lines of the text, bytes the lines' original bytes cut at offsets).
    struct Sorted {
        std::vector<uint32_t> index;
        std::vector<int64_t> values;
        std::vector<uint8_t> lineClass;
        std::vector<uint8_t> bytes;
        std::vector<uint32_t> offsets;
        std::vector<int32_t> ids, caps;
        gx_sort_totals totals{};
    };
    static uint32_t sortFlags(bool descending, bool carry, bool restLast) {
        return (descending ? GX_SORT_DESCENDING : 0u) | (carry ? GX_SORT_CARRY : 0u) | (restLast ? GX_SORT_REST_LAST : 0u);
    }
    // of the batch's lines (host buffers, Latin-1, 32-bit offsets, int32 match ids and dense capture rows; the C call takes every other layout)
    Sorted sortLines(const uint8_t* bytes, const uint32_t* offsets, uint64_t n, const int32_t* match_id, const int32_t* caps, const TopParts& parts,
                     bool descending = false, bool carry = false, bool restLast = false, const Where* where = nullptr) const {
        const std::vector<gx_top_part>& p = parts.parts();
        const std::vector<gx_where_term> terms = where ? where->terms() : std::vector<gx_where_term>();
        const uint32_t np = static_cast<uint32_t>(p.size()), nt = static_cast<uint32_t>(terms.size()), flags = sortFlags(descending, carry, restLast);
        const size_t slots = 2 * static_cast<size_t>(gx_max_groups(h_));
        Sorted r;
        int rc = gx_sort_lines(h_, bytes, offsets, n, match_id, caps, p.data(), np, terms.data(), nt, flags, nullptr, &r.totals, nullptr);   // the size query
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        const size_t m = static_cast<size_t>(r.totals.lines_out), units = static_cast<size_t>(r.totals.units_out);
        r.index.assign(m, 0);
        r.values.assign(m, 0);
        r.lineClass.assign(m, 0);
        r.bytes.assign(units + 1, 0);
        r.offsets.assign(m + 1, 0);
        r.ids.assign(m, 0);
        r.caps.assign(m * slots + 1, 0);
        gx_sort_out out{};
        out.out_index = r.index.data(); out.out_values = r.values.data(); out.out_class = r.lineClass.data(); out.out_bytes = r.bytes.data();
        out.out_offsets = r.offsets.data(); out.out_ids = r.ids.data(); out.out_caps = caps && slots ? r.caps.data() : nullptr;
        out.cap_lines = m; out.out_bytes_cap = units;
        rc = gx_sort_lines(h_, bytes, offsets, n, match_id, caps, p.data(), np, terms.data(), nt, flags, &out, &r.totals, nullptr);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        r.bytes.resize(units);
        r.caps.resize(caps ? m * slots : 0);
        return r;
    }
    // Whole files: raw text in, the same ordering out (gx_text_sort_lines).  counts (optional): lines per outcome index.
    Sorted textSortLines(const std::string& text, const TopParts& parts, bool descending = false, bool carry = false, bool restLast = false,
                         const Where* where = nullptr, std::vector<uint64_t>* counts = nullptr, uint64_t* nLines = nullptr, bool utf8 = false) const {
        if (counts) counts->assign(2 * extractions_.size() + 2, 0);
        gx_batch_opts o{};
        o.struct_size = sizeof(o);
        o.utf8 = utf8 ? 1u : 0u;
        const std::vector<gx_top_part>& p = parts.parts();
        const std::vector<gx_where_term> terms = where ? where->terms() : std::vector<gx_where_term>();
        const uint32_t np = static_cast<uint32_t>(p.size()), nt = static_cast<uint32_t>(terms.size()), flags = sortFlags(descending, carry, restLast);
        const uint8_t* t = reinterpret_cast<const uint8_t*>(text.data());
        Sorted r;
        int rc = gx_text_sort_lines(h_, t, text.size(), p.data(), np, terms.data(), nt, flags, nullptr, 0, nullptr, nullptr, nullptr, nullptr, &r.totals, nullptr, nullptr,
                                    utf8 ? &o : nullptr);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        const size_t m = static_cast<size_t>(r.totals.lines_out), units = static_cast<size_t>(r.totals.units_out);
        r.index.assign(m, 0);
        r.values.assign(m, 0);
        r.lineClass.assign(m, 0);
        r.bytes.assign(units + 1, 0);
        r.offsets.assign(m + 1, 0);
        rc = gx_text_sort_lines(h_, t, text.size(), p.data(), np, terms.data(), nt, flags, r.bytes.data(), units, r.offsets.data(), r.index.data(), r.values.data(),
                                r.lineClass.data(), &r.totals, counts ? counts->data() : nullptr, nLines, utf8 ? &o : nullptr);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        r.bytes.resize(units);
        return r;
    }
    // Percentiles of a number the lines captured (gx_capture_quantiles): nearest-rank quantiles num / den of the numbers that the parts
    // name -- sorted(values)[ceil(q * numbers) - 1], in integers alone -- each with its rank and the counts of the numbers below and
    // equal to it.  captureQuantiles(..., topParts().of("GetRequest", "timeTakenInMsec"), {{50, 100}, {95, 100}, {99, 100}}) is the
    // caller's median, p95 and p99 of its results' timeTakenInMsec (README.md:26,63-79).  With no numbers every row is all zeros.
    struct Quantiles {
        std::vector<gx_quantile_out> out;   // one per quantile, in input order
        gx_quantile_totals totals{};
    };
    // of the batch's lines (host buffers, Latin-1, 32-bit offsets, int32 match ids and dense capture rows; the C call takes every other layout)
    Quantiles captureQuantiles(const uint8_t* bytes, const uint32_t* offsets, uint64_t n, const int32_t* match_id, const int32_t* caps, const TopParts& parts,
                               const std::vector<gx_quantile>& quantiles, const Where* where = nullptr) const {
        const std::vector<gx_where_term> terms = where ? where->terms() : std::vector<gx_where_term>();
        Quantiles q;
        q.out.assign(quantiles.size(), gx_quantile_out{});
        const int rc = gx_capture_quantiles(h_, bytes, offsets, n, match_id, caps, parts.parts().data(), static_cast<uint32_t>(parts.parts().size()), terms.data(),
                                            static_cast<uint32_t>(terms.size()), quantiles.data(), static_cast<uint32_t>(quantiles.size()), q.out.data(), &q.totals,
                                            nullptr);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        return q;
    }
    // Whole files: raw text in, the same result out (gx_text_capture_quantiles).  counts (optional): lines per outcome index.
    Quantiles textCaptureQuantiles(const std::string& text, const TopParts& parts, const std::vector<gx_quantile>& quantiles, const Where* where = nullptr,
                                   std::vector<uint64_t>* counts = nullptr, uint64_t* nLines = nullptr, bool utf8 = false) const {
        if (counts) counts->assign(2 * extractions_.size() + 2, 0);
        gx_batch_opts o{};
        o.struct_size = sizeof(o);
        o.utf8 = utf8 ? 1u : 0u;
        const std::vector<gx_where_term> terms = where ? where->terms() : std::vector<gx_where_term>();
        Quantiles q;
        q.out.assign(quantiles.size(), gx_quantile_out{});
        const int rc = gx_text_capture_quantiles(h_, reinterpret_cast<const uint8_t*>(text.data()), text.size(), parts.parts().data(),
                                                 static_cast<uint32_t>(parts.parts().size()), terms.data(), static_cast<uint32_t>(terms.size()), quantiles.data(),
                                                 static_cast<uint32_t>(quantiles.size()), q.out.data(), &q.totals, counts ? counts->data() : nullptr, nLines,
                                                 utf8 ? &o : nullptr);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        return q;
    }
    // Percentiles of a captured number per captured text (gx_group_quantiles): groupLines plus, per key, the nearest-rank quantiles of
    // the numbers its lines captured.  groupQuantiles(..., groupParts().of("GetRequest", "path", "timeTakenInMsec"), {{50, 100}, {95, 100},
    // {99, 100}}) is the caller's byPath.computeIfAbsent(path, ...).add(timeTakenInMsec) and sorted(list)[ceil(q * size) - 1] per key
    // (README.md:26,63-79).  A key without numbers has all-zero rows.
    struct GroupQuantiles : Groups {
        size_t nQuantiles = 0;
        std::vector<gx_quantile_out> quantiles;   // keys.size() x nQuantiles rows, key-major
        const gx_quantile_out& at(size_t key, size_t quantile) const { return quantiles[key * nQuantiles + quantile]; }
    };
    // of the batch's lines (host buffers, Latin-1, 32-bit offsets, int32 match ids and dense capture rows; the C call takes every other layout)
    GroupQuantiles groupQuantiles(const uint8_t* bytes, const uint32_t* offsets, uint64_t n, const int32_t* match_id, const int32_t* caps, const GroupParts& parts,
                                  const std::vector<gx_quantile>& quantiles, const Where* where = nullptr) const {
        GroupQuantiles g;
        g.nQuantiles = quantiles.size();
        static_cast<Groups&>(g) = groupsOf(parts, where, &n, [&](const gx_group_part* p, uint32_t np, const gx_where_term* t, uint32_t nt, const gx_group_out* out,
                                                                  gx_group_totals* totals) {
            return gx_group_quantiles(h_, bytes, offsets, n, match_id, caps, p, np, t, nt, quantiles.data(), static_cast<uint32_t>(quantiles.size()), 0, out,
                                      g.quantiles.empty() ? nullptr : g.quantiles.data(), totals, nullptr);
        }, &g.quantiles, quantiles.size());
        return g;
    }
    // Whole files: raw text in, the same result out (gx_text_group_quantiles).  counts (optional): lines per outcome index.
    GroupQuantiles textGroupQuantiles(const std::string& text, const GroupParts& parts, const std::vector<gx_quantile>& quantiles, const Where* where = nullptr,
                                      std::vector<uint64_t>* counts = nullptr, uint64_t* nLines = nullptr, bool utf8 = false) const {
        if (counts) counts->assign(2 * extractions_.size() + 2, 0);
        gx_batch_opts o{};
        o.struct_size = sizeof(o);
        o.utf8 = utf8 ? 1u : 0u;
        uint64_t lines = 0;
        GroupQuantiles g;
        g.nQuantiles = quantiles.size();
        static_cast<Groups&>(g) = groupsOf(parts, where, &lines, [&](const gx_group_part* p, uint32_t np, const gx_where_term* t, uint32_t nt, const gx_group_out* out,
                                                                      gx_group_totals* totals) {
            return gx_text_group_quantiles(h_, reinterpret_cast<const uint8_t*>(text.data()), text.size(), p, np, t, nt, quantiles.data(),
                                           static_cast<uint32_t>(quantiles.size()), 0, out, g.quantiles.empty() ? nullptr : g.quantiles.data(), totals,
                                           counts ? counts->data() : nullptr, &lines, utf8 ? &o : nullptr);
        }, &g.quantiles, quantiles.size());
        if (nLines) *nLines = lines;
        return g;
    }
    // Keys ranked by their lines or by the numbers their lines captured (gx_top_groups): "the ten most requested paths" is
    // topGroups(..., groupParts().of("GetRequest", "path"), 10), "the ten clients that sent the most bytes" ranks with GX_RANK_SUM -- the
    // caller's byPath.entrySet().stream().sorted(comparingByValue().reversed()).limit(10) (README.md:26,63-79).  Groups' fields in RANK
    // order (ties: the key that appeared first), plus the keys' numbers in groupLines' order; lineKey stays empty, lineRank holds, when
    // asked for, every input line's rank (0xFFFFFFFF: no key, or its key not delivered).
    struct TopGroups : Groups {
        std::vector<uint32_t> keyNumber;
        std::vector<uint32_t> lineRank;
        gx_top_groups_totals top{};   // top.group is Groups::totals
    };
    // of the batch's lines (host buffers, Latin-1, 32-bit offsets, int32 match ids and dense capture rows; the C call takes every other layout)
    TopGroups topGroups(const uint8_t* bytes, const uint32_t* offsets, uint64_t n, const int32_t* match_id, const int32_t* caps, const GroupParts& parts,
                        uint32_t nWanted, uint32_t rankBy = GX_RANK_LINES, bool largest = true, const Where* where = nullptr, bool lineRank = false) const {
        const uint32_t flags = largest ? 0u : GX_TOP_GROUPS_SMALLEST;
        return topGroupsOf(parts, where, nWanted, lineRank, &n, [&](const gx_group_part* p, uint32_t np, const gx_where_term* t, uint32_t nt, uint64_t maxKeys,
                                                                    const gx_top_groups_out* out, gx_top_groups_totals* totals) {
            return gx_top_groups(h_, bytes, offsets, n, match_id, caps, p, np, t, nt, rankBy, nWanted, maxKeys, flags, out, totals, nullptr);
        });
    }
    // Whole files: raw text in, the same result out (gx_text_top_groups).  counts (optional): lines per outcome index.
    TopGroups textTopGroups(const std::string& text, const GroupParts& parts, uint32_t nWanted, uint32_t rankBy = GX_RANK_LINES, bool largest = true,
                            const Where* where = nullptr, bool lineRank = false, std::vector<uint64_t>* counts = nullptr, uint64_t* nLines = nullptr,
                            bool utf8 = false) const {
        if (counts) counts->assign(2 * extractions_.size() + 2, 0);
        gx_batch_opts o{};
        o.struct_size = sizeof(o);
        o.utf8 = utf8 ? 1u : 0u;
        const uint32_t flags = largest ? 0u : GX_TOP_GROUPS_SMALLEST;
        uint64_t lines = 0;
        TopGroups g = topGroupsOf(parts, where, nWanted, lineRank, &lines, [&](const gx_group_part* p, uint32_t np, const gx_where_term* t, uint32_t nt,
                                                                               uint64_t maxKeys, const gx_top_groups_out* out, gx_top_groups_totals* totals) {
            return gx_text_top_groups(h_, reinterpret_cast<const uint8_t*>(text.data()), text.size(), p, np, t, nt, rankBy, nWanted, maxKeys, flags, out, totals,
                                      counts ? counts->data() : nullptr, &lines, utf8 ? &o : nullptr);
        });
        if (nLines) *nLines = lines;
        return g;
    }
    // Whole files: raw text in, the text of the lines `want` names out (gx_text_select) -- with want(true, true) the
    // lines textToJsonl writes nothing for.  counts (optional): lines per outcome index.
    // utf8: the text is UTF-8 and outcomes are those of the decoded Strings (gx_batch_opts.utf8 = 1); the selected lines are their bytes
    std::string textSelect(const std::string& text, const Want& want, std::vector<uint64_t>* counts = nullptr, uint64_t* nLines = nullptr,
                           bool utf8 = false) const {
        if (want.size() != 2 * extractions_.size() + 1) throw GorpError(GX_E_ARG, "textSelect: the want mask has 2K + 1 entries");
        if (counts) counts->assign(2 * extractions_.size() + 2, 0);
        uint64_t size = 0;
        std::string out(text.size() + 1, '\0');   // (one pass: the selected text is no larger than the text)
        gx_batch_opts o{};
        o.struct_size = sizeof(o);
        o.utf8 = utf8 ? 1u : 0u;
        int rc = gx_text_select(h_, reinterpret_cast<const uint8_t*>(text.data()), text.size(), want.data(), reinterpret_cast<uint8_t*>(&out[0]), text.size(), &size,
                                counts ? counts->data() : nullptr, nLines, utf8 ? &o : nullptr);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        out.resize(static_cast<size_t>(size));
        return out;
    }
    // Every sink's lines at once (gx_partition_lines): the kept lines ordered by (outcome index, input line number) as a new batch,
    // and where every outcome's group begins -- outcome x's lines are offsets[groupLines[x] .. groupLines[x + 1]], its bytes
    // bytes[groupUnits[x] .. groupUnits[x + 1]) (2K + 3 entries each).  want == nullptr keeps every outcome 0 .. 2K.
    struct Partition { std::vector<uint32_t> index; std::vector<uint8_t> bytes; std::vector<uint32_t> offsets; std::vector<uint64_t> groupLines, groupUnits; };
    Partition partitionLines(const uint8_t* bytes, const uint32_t* offsets, uint64_t n, const int32_t* match_id, const Want* want = nullptr) const {
        if (want && want->size() != 2 * extractions_.size() + 1) throw GorpError(GX_E_ARG, "partitionLines: the want mask has 2K + 1 entries");
        // one pass: no partition is larger than its input
        const uint64_t total = offsets[n] - offsets[0];
        uint64_t k = 0, size = 0;
        const size_t groups = 2 * extractions_.size() + 3;
        Partition s{std::vector<uint32_t>(static_cast<size_t>(n) + 1), std::vector<uint8_t>(static_cast<size_t>(total) + 1), std::vector<uint32_t>(static_cast<size_t>(n) + 1),
                    std::vector<uint64_t>(groups), std::vector<uint64_t>(groups)};
        int rc = gx_partition_lines(h_, bytes, offsets, n, match_id, nullptr, want ? want->data() : nullptr, s.index.data(), s.bytes.data(), s.offsets.data(), nullptr,
                                    nullptr, n, total, s.groupLines.data(), s.groupUnits.data(), &k, &size, nullptr);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        s.index.resize(static_cast<size_t>(k));
        s.bytes.resize(static_cast<size_t>(size));
        s.offsets.resize(static_cast<size_t>(k) + 1);
        return s;
    }
    // Whole files: raw text in, one homogeneous JSON Lines stream per extraction out (gx_text_to_jsonl_by_extraction): textToJsonl's
    // lines regrouped stably by extraction; extraction k's objects are the returned text's [groupOut[k], groupOut[k + 1]).
    std::string textToJsonlByExtraction(const std::string& text, const char* idAs = nullptr, std::vector<uint64_t>* groupOut = nullptr,
                                        std::vector<uint64_t>* counts = nullptr, uint64_t* nLines = nullptr, bool utf8 = false) const {
        if (groupOut) groupOut->assign(extractions_.size() + 1, 0);
        if (counts) counts->assign(2 * extractions_.size() + 2, 0);
        gx_batch_opts o{};
        o.struct_size = sizeof(o);
        o.utf8 = utf8 ? 1u : 0u;
        uint64_t size = 0;
        const uint8_t* p = reinterpret_cast<const uint8_t*>(text.data());
        int rc = gx_text_to_jsonl_by_extraction(h_, p, text.size(), idAs, nullptr, 0, &size, nullptr, nullptr, nullptr, &o);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        std::string out(static_cast<size_t>(size) + 1, '\0');
        rc = gx_text_to_jsonl_by_extraction(h_, p, text.size(), idAs, reinterpret_cast<uint8_t*>(&out[0]), size, &size, groupOut ? groupOut->data() : nullptr,
                                            counts ? counts->data() : nullptr, nLines, &o);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        out.resize(static_cast<size_t>(size));
        return out;
    }
    // A series per captured text (gx_group_series): the caller's
    //     long b = Math.floorDiv(Instant.parse(r.asMap().get("ts")).toEpochMilli() - origin, 60_000L);
    //     perVerb.computeIfAbsent(r.asMap().get("verb"), v -> new TreeMap<Long, Stats>()).computeIfAbsent(b, x -> new Stats()).record(...);
    // (README.md:26,63-79, with a timestamp field) -- GROUP BY verb, floor((ts - origin) / width).  The parts of a call are groupParts' plus
    // a NUMBER extractor per part (an empty name, or -1: the part's lines have a key and no number), read under its group's number format:
    // seriesParts().of("GetRequest", "verb", "ts", "timeTakenInMsec").
    class SeriesParts {
    public:
        explicit SeriesParts(const Gorp* g) : g_(g), keys_(g) {}
        SeriesParts& of(const std::string& extraction, const std::string& key, const std::string& number, const std::string& value = std::string()) {
            int32_t n = -1;
            if (!number.empty()) {
                Where at(g_);
                at.on(extraction, number).isSet();
                n = at.terms()[0].group;
            }
            keys_.of(extraction, key, value);
            numbers_.push_back(n);
            return *this;
        }
        SeriesParts& of(size_t extraction, size_t keyGroup, int32_t numberGroup, int32_t valueGroup = -1) {
            if (numberGroup < -1 || (extraction < g_->extractions_.size() && numberGroup >= 0 &&
                                     static_cast<size_t>(numberGroup) >= g_->extractions_[extraction].extractorNames.size()))
                throw std::invalid_argument("no such extraction or group");
            keys_.of(extraction, keyGroup, valueGroup);
            numbers_.push_back(numberGroup);
            return *this;
        }
        const GroupParts& keys() const { return keys_; }
        const std::vector<int32_t>& numbers() const { return numbers_; }

    private:
        const Gorp* g_;
        GroupParts keys_;
        std::vector<int32_t> numbers_;
    };
    SeriesParts seriesParts() const { return SeriesParts(this); }
    // groupLines' result, plus the axis (the distinct buckets that hold a cell, ascending) and the cells ordered by (key number, bucket):
    // per cell its key's number, the index of its bucket on the axis, its first line, its lines and -- when a part has a value -- its
    // gx_measure_stats; per key where its cells begin (keys.size() + 1 entries); per input line its cell's number (0xFFFFFFFF: none).
    struct Series : Groups {
        std::vector<int64_t> bucketNumber;
        std::vector<uint32_t> cellKey, cellBucket, cellFirstLine;
        std::vector<uint64_t> cellLines;
        std::vector<gx_measure_stats> cellStats;   // empty when no part has a value
        std::vector<uint64_t> keyCellBegin;
        std::vector<uint32_t> lineCell;
        gx_series_totals series{};
    };
    Series groupSeries(const uint8_t* bytes, const uint32_t* offsets, uint64_t n, const int32_t* match_id, const int32_t* caps, const SeriesParts& parts,
                       int64_t width, int64_t origin = 0, const Where* where = nullptr) const {
        return seriesOf(parts, where, &n, n, [&](const gx_group_part* p, uint32_t np, const int32_t* s, const gx_where_term* t, uint32_t nt, const gx_group_out* out,
                                                 const gx_series_out* so, gx_series_totals* totals) {
            return gx_group_series(h_, bytes, offsets, n, match_id, caps, p, np, s, origin, width, t, nt, 0, out, so, totals, nullptr);
        });
    }
    // Whole files: raw text in, the same series out (gx_text_group_series).  counts (optional): lines per outcome index.
    Series textGroupSeries(const std::string& text, const SeriesParts& parts, int64_t width, int64_t origin = 0, const Where* where = nullptr,
                           std::vector<uint64_t>* counts = nullptr, uint64_t* nLines = nullptr, bool utf8 = false) const {
        if (counts) counts->assign(2 * extractions_.size() + 2, 0);
        gx_batch_opts o{};
        o.struct_size = sizeof(o);
        o.utf8 = utf8 ? 1u : 0u;
        uint64_t lines = 0, ends = 1;   // (no more lines than line ends, plus the last)
        for (const char c : text) ends += (c == '\n' || c == '\r') ? 1u : 0u;
        Series r = seriesOf(parts, where, &lines, ends, [&](const gx_group_part* p, uint32_t np, const int32_t* s, const gx_where_term* t, uint32_t nt,
                                                            const gx_group_out* out, const gx_series_out* so, gx_series_totals* totals) {
            return gx_text_group_series(h_, reinterpret_cast<const uint8_t*>(text.data()), text.size(), p, np, s, origin, width, t, nt, 0, out, so, totals,
                                        counts ? counts->data() : nullptr, &lines, utf8 ? &o : nullptr);
        });
        if (nLines) *nLines = lines;
        return r;
    }
    // Sessions per captured text (gx_group_sessions): the caller's
    //     byId.computeIfAbsent(r.asMap().get("id"), k -> new ArrayList<>()).add(r);
    //     ... per id: sort by Instant.parse(ts).toEpochMilli(); a new session wherever ts - previous ts > maxGap
    // (README.md:26,63-79) -- Splunk's `transaction id maxpause=30s`.  The parts are seriesParts(): the NUMBER extractor is the line's
    // TIME.  groupLines' result, plus the sessions ordered by (key number, begin): per session its key's number, the times of its first
    // and last entry, the input line of its first entry, its entries and -- when a part has a value -- its gx_measure_stats; where its
    // entries begin in entryLine (sessions + 1 entries); per key where its sessions begin (keys.size() + 1 entries); the entries' input
    // lines ordered by (key, time, line); per input line its session's number (0xFFFFFFFF: the line is no entry).
    struct Sessions : Groups {
        std::vector<uint32_t> sessionKey, sessionFirstLine;
        std::vector<int64_t> sessionBegin, sessionEnd;
        std::vector<uint64_t> sessionLines;
        std::vector<gx_measure_stats> sessionStats;   // empty when no part has a value
        std::vector<uint64_t> sessionEntryBegin, keySessionBegin;
        std::vector<uint32_t> entryLine, lineSession;
        gx_sessions_totals sessions{};
    };
    Sessions groupSessions(const uint8_t* bytes, const uint32_t* offsets, uint64_t n, const int32_t* match_id, const int32_t* caps, const SeriesParts& parts,
                           int64_t maxGap, const Where* where = nullptr) const {
        return sessionsOf(parts, where, &n, [&](const gx_group_part* p, uint32_t np, const int32_t* s, const gx_where_term* t, uint32_t nt, const gx_group_out* out,
                                                const gx_sessions_out* so, gx_sessions_totals* totals) {
            return gx_group_sessions(h_, bytes, offsets, n, match_id, caps, p, np, s, maxGap, t, nt, 0, out, so, totals, nullptr);
        });
    }
    // Whole files: raw text in, the same sessions out (gx_text_group_sessions).  counts (optional): lines per outcome index.
    Sessions textGroupSessions(const std::string& text, const SeriesParts& parts, int64_t maxGap, const Where* where = nullptr,
                               std::vector<uint64_t>* counts = nullptr, uint64_t* nLines = nullptr, bool utf8 = false) const {
        if (counts) counts->assign(2 * extractions_.size() + 2, 0);
        gx_batch_opts o{};
        o.struct_size = sizeof(o);
        o.utf8 = utf8 ? 1u : 0u;
        uint64_t lines = 0;
        Sessions r = sessionsOf(parts, where, &lines, [&](const gx_group_part* p, uint32_t np, const int32_t* s, const gx_where_term* t, uint32_t nt,
                                                          const gx_group_out* out, const gx_sessions_out* so, gx_sessions_totals* totals) {
            return gx_text_group_sessions(h_, reinterpret_cast<const uint8_t*>(text.data()), text.size(), p, np, s, maxGap, t, nt, 0, out, so, totals,
                                          counts ? counts->data() : nullptr, &lines, utf8 ? &o : nullptr);
        });
        if (nLines) *nLines = lines;
        return r;
    }
    // Trailing time windows per captured text (gx_group_windows): the caller's deque per key,
    //     q.addLast(t);  while (t - q.peekFirst() > window) q.removeFirst();  if (q.size() >= threshold && !tripped.contains(user)) alert(...)
    // -- Splunk's `streamstats time_window=60s count by user`, fail2ban's findtime and maxretry.  The parts are seriesParts(): the NUMBER
    // extractor is the line's TIME.  groupLines' result, plus per entry -- ordered by (key, time, line) -- its input line, key number, time,
    // the number of its key's entries within `window` before it (itself included) and, when a part has a value, that window's
    // gx_window_sum; per key where its entries begin (keys.size() + 1 entries), its peak and the input line that first attains it (0 and
    // 0xFFFFFFFF: the key has no entry); per input line its window_lines (0: the line is no entry); and the TRIPS, the entries at which the
    // count reaches `threshold` from below (0: no trips), in the same order, with every key's run of them.
    struct Windows : Groups {
        std::vector<uint32_t> entryLine, entryKey, entryWindowLines;
        std::vector<int64_t> entryTime;
        std::vector<gx_window_sum> entryWindowSum;   // empty when no part has a value
        std::vector<uint64_t> keyEntryBegin, keyTripBegin;
        std::vector<uint32_t> keyPeakLines, keyPeakLine, lineWindowLines;
        std::vector<uint32_t> tripKey, tripLine, tripEntry;
        std::vector<int64_t> tripTime;
        gx_windows_totals windows{};
    };
    Windows groupWindows(const uint8_t* bytes, const uint32_t* offsets, uint64_t n, const int32_t* match_id, const int32_t* caps, const SeriesParts& parts,
                         int64_t window, uint32_t threshold = 0, const Where* where = nullptr) const {
        return windowsOf(parts, threshold, where, &n, [&](const gx_group_part* p, uint32_t np, const int32_t* s, const gx_where_term* t, uint32_t nt,
                                                          const gx_group_out* out, const gx_windows_out* wo, gx_windows_totals* totals) {
            return gx_group_windows(h_, bytes, offsets, n, match_id, caps, p, np, s, window, threshold, t, nt, 0, out, wo, totals, nullptr);
        });
    }
    // Whole files: raw text in, the same windows out (gx_text_group_windows).  counts (optional): lines per outcome index.
    Windows textGroupWindows(const std::string& text, const SeriesParts& parts, int64_t window, uint32_t threshold = 0, const Where* where = nullptr,
                             std::vector<uint64_t>* counts = nullptr, uint64_t* nLines = nullptr, bool utf8 = false) const {
        if (counts) counts->assign(2 * extractions_.size() + 2, 0);
        gx_batch_opts o{};
        o.struct_size = sizeof(o);
        o.utf8 = utf8 ? 1u : 0u;
        uint64_t lines = 0;
        Windows r = windowsOf(parts, threshold, where, &lines, [&](const gx_group_part* p, uint32_t np, const int32_t* s, const gx_where_term* t, uint32_t nt,
                                                                   const gx_group_out* out, const gx_windows_out* wo, gx_windows_totals* totals) {
            return gx_text_group_windows(h_, reinterpret_cast<const uint8_t*>(text.data()), text.size(), p, np, s, window, threshold, t, nt, 0, out, wo, totals,
                                         counts ? counts->data() : nullptr, &lines, utf8 ? &o : nullptr);
        });
        if (nLines) *nLines = lines;
        return r;
    }
    // Begin/end spans per captured text (gx_group_spans): the caller's
    //     if (r.name().equals("RequestStart")) { prev = open.put(id(r), r); if (prev != null) superseded.add(prev); }
    //     if (r.name().equals("RequestEnd"))   { b = open.remove(id(r)); if (b == null) orphanEnds.add(r); else took.record(ts(r) - ts(b)); }
    // -- Splunk's `transaction id startswith=... endswith=...`.  The parts of a call are seriesParts' (the NUMBER extractor is the line's
    // TIME; an empty name, or -1: none) plus a ROLE per part: spanParts().begin("RequestStart", "id", "ts").end("RequestEnd", "id", "ts").
    class SpanParts {
    public:
        explicit SpanParts(const Gorp* g) : timed_(g) {}
        SpanParts& begin(const std::string& extraction, const std::string& key, const std::string& time = std::string(), const std::string& value = std::string()) {
            timed_.of(extraction, key, time, value);
            roles_.push_back(GX_SPAN_BEGIN);
            return *this;
        }
        SpanParts& end(const std::string& extraction, const std::string& key, const std::string& time = std::string(), const std::string& value = std::string()) {
            timed_.of(extraction, key, time, value);
            roles_.push_back(GX_SPAN_END);
            return *this;
        }
        SpanParts& of(size_t extraction, size_t keyGroup, int32_t timeGroup, uint32_t role, int32_t valueGroup = -1) {
            if (role != GX_SPAN_BEGIN && role != GX_SPAN_END) throw std::invalid_argument("a role is GX_SPAN_BEGIN or GX_SPAN_END");
            timed_.of(extraction, keyGroup, timeGroup, valueGroup);
            roles_.push_back(role);
            return *this;
        }
        const SeriesParts& timed() const { return timed_; }
        const std::vector<uint32_t>& roles() const { return roles_; }

    private:
        SeriesParts timed_;
        std::vector<uint32_t> roles_;
    };
    SpanParts spanParts() const { return SpanParts(this); }
    // groupLines' result, plus the spans ordered by (key number, end line): per span its key's number, the input lines and the times of
    // its two sides, its duration and its class (0 duration, 1 unset, 2 not a number); per key where its spans begin (keys.size() + 1
    // entries), the gx_measure_stats of its spans' durations and the BEGIN line it leaves open (0xFFFFFFFF: none); per input line its
    // span's number (0xFFFFFFFF: none) and its state (0 no entry, 1 a span's begin, 2 a span's end, 3 a begin superseded, 4 a begin left
    // open, 5 an end without a begin).
    struct Spans : Groups {
        std::vector<uint32_t> spanKey, spanBeginLine, spanEndLine;
        std::vector<int64_t> spanBegin, spanEnd, spanDuration;
        std::vector<uint8_t> spanClass;
        std::vector<uint64_t> keySpanBegin;
        std::vector<gx_measure_stats> keySpanStats;
        std::vector<uint32_t> keyOpenLine, lineSpan;
        std::vector<uint8_t> lineState;
        gx_spans_totals spans{};
    };
    Spans groupSpans(const uint8_t* bytes, const uint32_t* offsets, uint64_t n, const int32_t* match_id, const int32_t* caps, const SpanParts& parts,
                     const Where* where = nullptr) const {
        return spansOf(parts, where, &n, [&](const gx_group_part* p, uint32_t np, const int32_t* s, const uint32_t* roles, const gx_where_term* t, uint32_t nt,
                                             const gx_group_out* out, const gx_spans_out* so, gx_spans_totals* totals) {
            return gx_group_spans(h_, bytes, offsets, n, match_id, caps, p, np, s, roles, t, nt, 0, out, so, totals, nullptr);
        });
    }
    // Whole files: raw text in, the same spans out (gx_text_group_spans).  counts (optional): lines per outcome index.
    Spans textGroupSpans(const std::string& text, const SpanParts& parts, const Where* where = nullptr, std::vector<uint64_t>* counts = nullptr,
                         uint64_t* nLines = nullptr, bool utf8 = false) const {
        if (counts) counts->assign(2 * extractions_.size() + 2, 0);
        gx_batch_opts o{};
        o.struct_size = sizeof(o);
        o.utf8 = utf8 ? 1u : 0u;
        uint64_t lines = 0;
        Spans r = spansOf(parts, where, &lines, [&](const gx_group_part* p, uint32_t np, const int32_t* s, const uint32_t* roles, const gx_where_term* t, uint32_t nt,
                                                    const gx_group_out* out, const gx_spans_out* so, gx_spans_totals* totals) {
            return gx_text_group_spans(h_, reinterpret_cast<const uint8_t*>(text.data()), text.size(), p, np, s, roles, t, nt, 0, out, so, totals,
                                       counts ? counts->data() : nullptr, &lines, utf8 ? &o : nullptr);
        });
        if (nLines) *nLines = lines;
        return r;
    }
    int maxGroups() const { return gx_max_groups(h_); }
    gx_handle* handle() const { return h_; }

private:
    friend class DefinitionReader;
    Gorp(gx_handle* h, std::vector<CookedExtraction> x) : h_(h), extractions_(std::move(x)) {}
    // The size query with a table for a modest number of keys -- if that table overflows (GX_E_LIMIT, exact == 0), once more with as many
    // keys as lines, which always suffices -- then the call with exactly the sizes it reported.  *lines: the batch's lines (for a text:
    // what the call itself reports).
    template <typename Call>
    Groups groupsOf(const GroupParts& parts, const Where* where, const uint64_t* lines, Call&& call, std::vector<gx_quantile_out>* rows = nullptr,
                    size_t rowsPerKey = 0) const {
        const std::vector<gx_group_part>& p = parts.parts();
        const std::vector<gx_where_term> terms = where ? where->terms() : std::vector<gx_where_term>();
        const uint32_t np = static_cast<uint32_t>(p.size()), nt = static_cast<uint32_t>(terms.size());
        Groups g;
        gx_group_out query{};
        query.max_keys = 1024;
        int rc = call(p.data(), np, terms.data(), nt, &query, &g.totals);
        if (rc == GX_E_LIMIT && g.totals.n_keys != 0 && g.totals.exact == 0) {
            query.max_keys = *lines;
            rc = call(p.data(), np, terms.data(), nt, &query, &g.totals);
        }
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        const size_t k = static_cast<size_t>(g.totals.n_keys);
        std::vector<uint8_t> units(static_cast<size_t>(g.totals.key_units) + 1);
        std::vector<uint32_t> offsets(k + 1, 0);
        g.firstLine.assign(k, 0);
        g.lines.assign(k, 0);
        if (parts.hasValues()) g.stats.assign(k, gx_measure_stats{});
        g.lineKey.assign(static_cast<size_t>(*lines), 0xFFFFFFFFu);
        if (rows) rows->assign(k * rowsPerKey, gx_quantile_out{});   // (groupQuantiles: its call delivers them from here on)
        gx_group_out out{};
        out.key_units = units.data();
        out.key_units_cap = g.totals.key_units;
        out.key_offsets = offsets.data();
        out.key_first_line = g.firstLine.data();
        out.key_lines = g.lines.data();
        out.key_stats = parts.hasValues() ? g.stats.data() : nullptr;
        out.line_key = g.lineKey.data();
        out.max_keys = g.totals.n_keys;   // (the arrays' capacity; a table of twice as many slots holds them all)
        rc = call(p.data(), np, terms.data(), nt, &out, &g.totals);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        for (size_t j = 0; j < k; ++j) g.keys.emplace_back(reinterpret_cast<const char*>(units.data()) + offsets[j], offsets[j + 1] - offsets[j]);
        return g;
    }
    // lookupLines and textLookupLines: the entries as a CSR; with keep the size query, then the call with exactly the sizes it reported
    // (linesCap: the lines, or no fewer).  call(parts, n, terms, n, entry units, entry offsets, result, deliver).
    static gx_lookup_out lookupOut(Lookup& r, bool deliver) {
        gx_lookup_out out{};
        if (!deliver) return out;
        out.line_entry = r.lineEntry.data();
        out.entry_same = r.entrySame.data();
        out.entry_lines = r.entryLines.data();
        out.entry_first_line = r.entryFirstLine.data();
        out.entry_stats = r.entryStats.empty() ? nullptr : r.entryStats.data();
        return out;
    }
    template <typename Call>
    Lookup lookupOf(const GroupParts& parts, const std::vector<std::string>& entries, uint32_t keep, const Where* where, uint64_t linesCap, Call&& call) const {
        const std::vector<gx_group_part>& p = parts.parts();
        const std::vector<gx_where_term> terms = where ? where->terms() : std::vector<gx_where_term>();
        const uint32_t np = static_cast<uint32_t>(p.size()), nt = static_cast<uint32_t>(terms.size());
        std::string units;
        std::vector<uint32_t> eoff(1, 0);
        for (const std::string& e : entries) {
            units += e;
            eoff.push_back(static_cast<uint32_t>(units.size()));
        }
        const size_t m = entries.size();
        Lookup r;
        int rc = GX_OK;
        if (keep != GX_LOOKUP_KEEP_NOTHING) {
            rc = call(p.data(), np, terms.data(), nt, units.data(), eoff.data(), r, false);   // the size query
            if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        }
        const size_t kept = static_cast<size_t>(r.totals.lines_out);
        r.lineEntry.assign(static_cast<size_t>(linesCap) + 1, GX_LOOKUP_NONE);
        r.entrySame.assign(m + 1, 0);
        r.entryLines.assign(m + 1, 0);
        r.entryFirstLine.assign(m + 1, 0xFFFFFFFFu);
        if (parts.hasValues()) r.entryStats.assign(m + 1, gx_measure_stats{});
        if (keep != GX_LOOKUP_KEEP_NOTHING) {
            r.index.assign(kept + 1, 0);
            r.bytes.assign(static_cast<size_t>(r.totals.units_out) + 1, 0);
            r.offsets.assign(kept + 1, 0);
        }
        rc = call(p.data(), np, terms.data(), nt, units.data(), eoff.data(), r, true);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        r.lineEntry.resize(static_cast<size_t>(linesCap));
        r.entrySame.resize(m);
        r.entryLines.resize(m);
        r.entryFirstLine.resize(m);
        if (!r.entryStats.empty()) r.entryStats.resize(m);
        if (keep != GX_LOOKUP_KEEP_NOTHING) {
            r.index.resize(kept);
            r.bytes.resize(static_cast<size_t>(r.totals.units_out));
        }
        return r;
    }
    // groupsOf's scheme for bucketLines: the size query with a table for a modest number of buckets, once more with as many buckets as
    // lines if that table overflows, then the call with exactly the size it reported.
    template <typename Call>
    Buckets bucketsOf(const BucketParts& parts, const Where* where, const uint64_t* lines, Call&& call) const {
        const std::vector<gx_bucket_part> p = parts.parts();
        const std::vector<gx_where_term> terms = where ? where->terms() : std::vector<gx_where_term>();
        const uint32_t np = static_cast<uint32_t>(p.size()), nt = static_cast<uint32_t>(terms.size());
        Buckets b;
        gx_bucket_out query{};
        query.max_buckets = 1024;
        int rc = call(p.data(), np, terms.data(), nt, &query, &b.totals);
        if (rc == GX_E_LIMIT && b.totals.n_buckets != 0 && b.totals.exact == 0) {
            query.max_buckets = *lines;
            rc = call(p.data(), np, terms.data(), nt, &query, &b.totals);
        }
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        const size_t k = static_cast<size_t>(b.totals.n_buckets);
        b.bucketNumber.assign(k, 0);
        b.firstLine.assign(k, 0);
        b.lines.assign(k, 0);
        if (parts.hasValues()) b.stats.assign(k, gx_measure_stats{});
        b.lineBucket.assign(static_cast<size_t>(*lines), 0xFFFFFFFFu);
        gx_bucket_out out{};
        out.bucket_number = b.bucketNumber.data();
        out.bucket_first_line = b.firstLine.data();
        out.bucket_lines = b.lines.data();
        out.bucket_stats = parts.hasValues() ? b.stats.data() : nullptr;
        out.line_bucket = b.lineBucket.data();
        out.max_buckets = b.totals.n_buckets;   // (the arrays' capacity; a table of twice as many slots holds them all)
        rc = call(p.data(), np, terms.data(), nt, &out, &b.totals);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        return b;
    }
    // groupsOf with the pairs beside the keys: the size queries ask with a pair table for maxLines lines, which always suffices; the call
    // with exactly the sizes they reported delivers both.  Pair outputs are asked for only where a part has a second (the C call refuses
    // them otherwise: there is nothing they could hold).
    template <typename Call>
    Pairs pairsOf(const PairParts& parts, const Where* where, const uint64_t* lines, uint64_t maxLines, Call&& call) const {
        Pairs r;
        const int32_t none = -1;
        const std::vector<int32_t>& seconds = parts.seconds();
        bool wanted = seconds.empty();
        for (const int32_t s : seconds) wanted = wanted || s >= 0;
        std::vector<uint8_t> units;
        std::vector<uint32_t> offsets;
        Groups g = groupsOf(parts.keys(), where, lines, [&](const gx_group_part* p, uint32_t np, const gx_where_term* t, uint32_t nt, const gx_group_out* out,
                                                            gx_group_totals* totals) {
            gx_pairs_out po{};
            po.max_pairs = maxLines < (1ull << 30) ? maxLines : (1ull << 30);
            if (out->key_offsets != nullptr && wanted) {   // (the size query before it left the sizes in r.pairs)
                const size_t m = static_cast<size_t>(r.pairs.n_pairs);
                units.assign(static_cast<size_t>(r.pairs.pair_units) + 1, 0);
                offsets.assign(m + 1, 0);
                r.pairKey.assign(m, 0);
                r.pairFirstLine.assign(m, 0);
                r.pairLines.assign(m, 0);
                r.keyPairs.assign(static_cast<size_t>(out->max_keys), 0);
                r.linePair.assign(static_cast<size_t>(*lines), 0xFFFFFFFFu);
                po.pair_units = units.data(); po.pair_units_cap = r.pairs.pair_units; po.pair_offsets = offsets.data(); po.pair_key = r.pairKey.data();
                po.pair_first_line = r.pairFirstLine.data(); po.pair_lines = r.pairLines.data(); po.key_pairs = r.keyPairs.data(); po.line_pair = r.linePair.data();
                po.max_pairs = r.pairs.n_pairs;   // (the arrays' capacity; a table of twice as many slots holds them all)
            }
            const int rc = call(p, np, seconds.empty() ? &none : seconds.data(), t, nt, out, &po, &r.pairs);
            *totals = r.pairs.group;
            return rc;
        });
        static_cast<Groups&>(r) = std::move(g);
        if (!wanted) {
            r.keyPairs.assign(r.keys.size(), 0);
            r.linePair.assign(static_cast<size_t>(*lines), 0xFFFFFFFFu);
        }
        for (size_t j = 0; j < r.pairKey.size(); ++j) r.seconds.emplace_back(reinterpret_cast<const char*>(units.data()) + offsets[j], offsets[j + 1] - offsets[j]);
        return r;
    }
    // groupsOf with the series beside the keys: the size queries ask with tables for maxLines cells, which always suffices; the call with
    // exactly the sizes they reported delivers both.  Series outputs are asked for only where a part has a number (the C call refuses
    // them otherwise: there is nothing they could hold).
    template <typename Call>
    Series seriesOf(const SeriesParts& parts, const Where* where, const uint64_t* lines, uint64_t maxLines, Call&& call) const {
        Series r;
        const int32_t none = -1;
        const std::vector<int32_t>& numbers = parts.numbers();
        bool wanted = numbers.empty();
        for (const int32_t s : numbers) wanted = wanted || s >= 0;
        Groups g = groupsOf(parts.keys(), where, lines, [&](const gx_group_part* p, uint32_t np, const gx_where_term* t, uint32_t nt, const gx_group_out* out,
                                                            gx_group_totals* totals) {
            gx_series_out so{};
            so.max_cells = maxLines < (1ull << 30) ? maxLines : (1ull << 30);
            if (out->key_offsets != nullptr && wanted) {   // (the size query before it left the sizes in r.series)
                const size_t m = static_cast<size_t>(r.series.n_cells);
                r.bucketNumber.assign(static_cast<size_t>(r.series.n_buckets), 0);
                r.cellKey.assign(m, 0);
                r.cellBucket.assign(m, 0);
                r.cellFirstLine.assign(m, 0);
                r.cellLines.assign(m, 0);
                if (parts.keys().hasValues()) r.cellStats.assign(m, gx_measure_stats{});
                r.keyCellBegin.assign(static_cast<size_t>(out->max_keys) + 1, 0);
                r.lineCell.assign(static_cast<size_t>(*lines), 0xFFFFFFFFu);
                so.bucket_number = r.bucketNumber.data(); so.cell_key = r.cellKey.data(); so.cell_bucket = r.cellBucket.data();
                so.cell_first_line = r.cellFirstLine.data(); so.cell_lines = r.cellLines.data();
                so.cell_stats = parts.keys().hasValues() ? r.cellStats.data() : nullptr;
                so.key_cell_begin = r.keyCellBegin.data(); so.line_cell = r.lineCell.data();
                so.max_cells = r.series.n_cells;   // (the arrays' capacity; tables of twice as many slots hold them all)
                so.max_buckets = r.series.n_buckets;
            }
            const int rc = call(p, np, numbers.empty() ? &none : numbers.data(), t, nt, out, &so, &r.series);
            *totals = r.series.group;
            return rc;
        });
        static_cast<Groups&>(r) = std::move(g);
        if (!wanted) {
            r.keyCellBegin.assign(r.keys.size() + 1, 0);
            r.lineCell.assign(static_cast<size_t>(*lines), 0xFFFFFFFFu);
        }
        return r;
    }
    // groupsOf with the sessions beside the keys: the size queries leave the sessions and the entries in r.sessions; the call with
    // exactly the sizes they reported delivers both.  Session outputs are asked for only where a part has a number (the C call refuses
    // them otherwise: there is nothing they could hold).
    template <typename Call>
    Sessions sessionsOf(const SeriesParts& parts, const Where* where, const uint64_t* lines, Call&& call) const {
        Sessions r;
        const int32_t none = -1;
        const std::vector<int32_t>& numbers = parts.numbers();
        bool wanted = numbers.empty();
        for (const int32_t s : numbers) wanted = wanted || s >= 0;
        Groups g = groupsOf(parts.keys(), where, lines, [&](const gx_group_part* p, uint32_t np, const gx_where_term* t, uint32_t nt, const gx_group_out* out,
                                                            gx_group_totals* totals) {
            gx_sessions_out so{};
            if (out->key_offsets != nullptr && wanted) {   // (the size query before it left the sizes in r.sessions)
                const size_t m = static_cast<size_t>(r.sessions.n_sessions);
                r.sessionKey.assign(m, 0);
                r.sessionBegin.assign(m, 0);
                r.sessionEnd.assign(m, 0);
                r.sessionFirstLine.assign(m, 0);
                r.sessionLines.assign(m, 0);
                if (parts.keys().hasValues()) r.sessionStats.assign(m, gx_measure_stats{});
                r.sessionEntryBegin.assign(m + 1, 0);
                r.keySessionBegin.assign(static_cast<size_t>(out->max_keys) + 1, 0);
                r.entryLine.assign(static_cast<size_t>(r.sessions.entries), 0);
                r.lineSession.assign(static_cast<size_t>(*lines), 0xFFFFFFFFu);
                so.session_key = r.sessionKey.data(); so.session_begin = r.sessionBegin.data(); so.session_end = r.sessionEnd.data();
                so.session_first_line = r.sessionFirstLine.data(); so.session_lines = r.sessionLines.data();
                so.session_stats = parts.keys().hasValues() ? r.sessionStats.data() : nullptr;
                so.session_entry_begin = r.sessionEntryBegin.data(); so.key_session_begin = r.keySessionBegin.data();
                so.entry_line = r.entryLine.data(); so.line_session = r.lineSession.data();
                so.max_sessions = r.sessions.n_sessions;
                so.max_entries = r.sessions.entries;
            }
            const int rc = call(p, np, numbers.empty() ? &none : numbers.data(), t, nt, out, &so, &r.sessions);
            *totals = r.sessions.group;
            return rc;
        });
        static_cast<Groups&>(r) = std::move(g);
        if (!wanted) {
            r.sessionEntryBegin.assign(1, 0);
            r.keySessionBegin.assign(r.keys.size() + 1, 0);
            r.lineSession.assign(static_cast<size_t>(*lines), 0xFFFFFFFFu);
        }
        return r;
    }
    // groupsOf with the windows beside the keys: the size queries leave the entries and the trips in r.windows; the call with exactly
    // the sizes they reported delivers both.  Window outputs are asked for only where a part has a number, trip outputs only with a
    // threshold (the C call refuses them otherwise: there is nothing they could hold).
    template <typename Call>
    Windows windowsOf(const SeriesParts& parts, uint32_t threshold, const Where* where, const uint64_t* lines, Call&& call) const {
        Windows r;
        const int32_t none = -1;
        const std::vector<int32_t>& numbers = parts.numbers();
        bool wanted = numbers.empty();
        for (const int32_t s : numbers) wanted = wanted || s >= 0;
        Groups g = groupsOf(parts.keys(), where, lines, [&](const gx_group_part* p, uint32_t np, const gx_where_term* t, uint32_t nt, const gx_group_out* out,
                                                            gx_group_totals* totals) {
            gx_windows_out wo{};
            if (out->key_offsets != nullptr && wanted) {   // (the size query before it left the sizes in r.windows)
                const size_t m = static_cast<size_t>(r.windows.entries), nt_ = static_cast<size_t>(r.windows.n_trips), k = static_cast<size_t>(out->max_keys);
                r.entryLine.assign(m, 0);
                r.entryKey.assign(m, 0);
                r.entryTime.assign(m, 0);
                r.entryWindowLines.assign(m, 0);
                if (parts.keys().hasValues()) r.entryWindowSum.assign(m, gx_window_sum{});
                r.keyEntryBegin.assign(k + 1, 0);
                r.keyPeakLines.assign(k, 0);
                r.keyPeakLine.assign(k, 0xFFFFFFFFu);
                r.lineWindowLines.assign(static_cast<size_t>(*lines), 0);
                r.keyTripBegin.assign(k + 1, 0);
                wo.entry_line = r.entryLine.data(); wo.entry_key = r.entryKey.data(); wo.entry_time = r.entryTime.data();
                wo.entry_window_lines = r.entryWindowLines.data(); wo.entry_window_sum = parts.keys().hasValues() ? r.entryWindowSum.data() : nullptr;
                wo.key_entry_begin = r.keyEntryBegin.data(); wo.key_peak_lines = r.keyPeakLines.data(); wo.key_peak_line = r.keyPeakLine.data();
                wo.line_window_lines = r.lineWindowLines.data();
                if (threshold != 0) {
                    r.tripKey.assign(nt_, 0);
                    r.tripLine.assign(nt_, 0);
                    r.tripTime.assign(nt_, 0);
                    r.tripEntry.assign(nt_, 0);
                    wo.trip_key = r.tripKey.data(); wo.trip_line = r.tripLine.data(); wo.trip_time = r.tripTime.data(); wo.trip_entry = r.tripEntry.data();
                    wo.key_trip_begin = r.keyTripBegin.data();
                }
                wo.max_entries = r.windows.entries;
                wo.max_trips = r.windows.n_trips;
            }
            const int rc = call(p, np, numbers.empty() ? &none : numbers.data(), t, nt, out, &wo, &r.windows);
            *totals = r.windows.group;
            return rc;
        });
        static_cast<Groups&>(r) = std::move(g);
        if (!wanted) {
            r.keyEntryBegin.assign(r.keys.size() + 1, 0);
            r.keyTripBegin.assign(r.keys.size() + 1, 0);
            r.keyPeakLines.assign(r.keys.size(), 0);
            r.keyPeakLine.assign(r.keys.size(), 0xFFFFFFFFu);
            r.lineWindowLines.assign(static_cast<size_t>(*lines), 0);
        }
        return r;
    }
    // groupsOf with the spans beside the keys: the size queries leave the spans in r.spans; the call with exactly the sizes they reported
    // delivers both.
    template <typename Call>
    Spans spansOf(const SpanParts& parts, const Where* where, const uint64_t* lines, Call&& call) const {
        Spans r;
        const int32_t none = -1;
        const uint32_t no_role = GX_SPAN_BEGIN;
        const std::vector<int32_t>& numbers = parts.timed().numbers();
        const std::vector<uint32_t>& roles = parts.roles();
        Groups g = groupsOf(parts.timed().keys(), where, lines, [&](const gx_group_part* p, uint32_t np, const gx_where_term* t, uint32_t nt, const gx_group_out* out,
                                                                    gx_group_totals* totals) {
            gx_spans_out so{};
            if (out->key_offsets != nullptr) {   // (the size query before it left the sizes in r.spans)
                const size_t m = static_cast<size_t>(r.spans.n_spans), k = static_cast<size_t>(out->max_keys);
                r.spanKey.assign(m, 0);
                r.spanBeginLine.assign(m, 0);
                r.spanEndLine.assign(m, 0);
                r.spanBegin.assign(m, 0);
                r.spanEnd.assign(m, 0);
                r.spanDuration.assign(m, 0);
                r.spanClass.assign(m, 0);
                r.keySpanBegin.assign(k + 1, 0);
                r.keySpanStats.assign(k, gx_measure_stats{});
                r.keyOpenLine.assign(k, 0xFFFFFFFFu);
                r.lineSpan.assign(static_cast<size_t>(*lines), 0xFFFFFFFFu);
                r.lineState.assign(static_cast<size_t>(*lines), 0);
                so.span_key = r.spanKey.data(); so.span_begin_line = r.spanBeginLine.data(); so.span_end_line = r.spanEndLine.data();
                so.span_begin = r.spanBegin.data(); so.span_end = r.spanEnd.data(); so.span_duration = r.spanDuration.data(); so.span_class = r.spanClass.data();
                so.key_span_begin = r.keySpanBegin.data(); so.key_span_stats = r.keySpanStats.data(); so.key_open_line = r.keyOpenLine.data();
                so.line_span = r.lineSpan.data(); so.line_state = r.lineState.data();
                so.max_spans = r.spans.n_spans;
            }
            const int rc = call(p, np, numbers.empty() ? &none : numbers.data(), roles.empty() ? &no_role : roles.data(), t, nt, out, &so, &r.spans);
            *totals = r.spans.group;
            return rc;
        });
        static_cast<Groups&>(r) = std::move(g);
        return r;
    }
    // groupsOf's scheme for topGroups: the size query with a table for a modest number of keys, once more with as many keys as lines if
    // that table overflows, then the call with exactly the sizes it reported.
    template <typename Call>
    TopGroups topGroupsOf(const GroupParts& parts, const Where* where, uint32_t nWanted, bool lineRank, const uint64_t* lines, Call&& call) const {
        const std::vector<gx_group_part>& p = parts.parts();
        const std::vector<gx_where_term> terms = where ? where->terms() : std::vector<gx_where_term>();
        const uint32_t np = static_cast<uint32_t>(p.size()), nt = static_cast<uint32_t>(terms.size());
        TopGroups g;
        uint64_t maxKeys = 1024;
        int rc = call(p.data(), np, terms.data(), nt, maxKeys, nullptr, &g.top);
        if (rc == GX_E_LIMIT && g.top.group.n_keys != 0 && g.top.group.exact == 0) {
            maxKeys = *lines;
            rc = call(p.data(), np, terms.data(), nt, maxKeys, nullptr, &g.top);
        }
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        const size_t k = static_cast<size_t>(g.top.n_top);
        std::vector<uint8_t> units(static_cast<size_t>(g.top.units_top) + 1);
        std::vector<uint32_t> offsets(k + 1, 0);
        g.keyNumber.assign(k, 0);
        g.firstLine.assign(k, 0);
        g.lines.assign(k, 0);
        if (parts.hasValues()) g.stats.assign(k, gx_measure_stats{});
        if (lineRank) g.lineRank.assign(static_cast<size_t>(*lines), 0xFFFFFFFFu);
        gx_top_groups_out out{};
        out.key_units = units.data();
        out.key_units_cap = g.top.units_top;
        out.key_offsets = offsets.data();
        out.key_number = g.keyNumber.data();
        out.key_first_line = g.firstLine.data();
        out.key_lines = g.lines.data();
        out.key_stats = parts.hasValues() ? g.stats.data() : nullptr;
        out.line_rank = lineRank && !g.lineRank.empty() ? g.lineRank.data() : nullptr;
        out.cap_keys = nWanted;
        rc = call(p.data(), np, terms.data(), nt, maxKeys, &out, &g.top);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        g.totals = g.top.group;
        for (size_t j = 0; j < k; ++j) g.keys.emplace_back(reinterpret_cast<const char*>(units.data()) + offsets[j], offsets[j + 1] - offsets[j]);
        return g;
    }
    // The size query, then the call with exactly the sizes it reported.  call(..., top, deliver): deliver == false is the size query,
    // which fills top.totals alone; with deliver the outputs' capacities are the vectors' sizes.
    template <typename Call>
    Top topOf(const TopParts& parts, const Where* where, Call&& call) const {
        const std::vector<gx_top_part>& p = parts.parts();
        const std::vector<gx_where_term> terms = where ? where->terms() : std::vector<gx_where_term>();
        const uint32_t np = static_cast<uint32_t>(p.size()), nt = static_cast<uint32_t>(terms.size());
        Top top;
        int rc = call(p.data(), np, terms.data(), nt, top, false);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        const size_t k = static_cast<size_t>(top.totals.n_top), units = static_cast<size_t>(top.totals.units_top);
        top.index.assign(k, 0);
        top.values.assign(k, 0);
        top.bytes.assign(units, 0);
        top.offsets.clear();
        rc = call(p.data(), np, terms.data(), nt, top, true);
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        top.index.resize(k);
        top.values.resize(k);
        return top;
    }
    static std::vector<MeasureStats> statsOf(const std::vector<gx_measure>& m, const std::vector<gx_measure_stats>& stats, const std::vector<uint64_t>& hist) {
        std::vector<MeasureStats> out;
        size_t at = 0;
        for (size_t t = 0; t < m.size(); ++t) {
            out.push_back(MeasureStats{stats[t], std::vector<uint64_t>(hist.begin() + at, hist.begin() + at + m[t].n_edges + 1)});
            at += m[t].n_edges + 1;
        }
        return out;
    }
    gx_handle* h_;
    std::vector<CookedExtraction> extractions_;

    std::unique_ptr<ExtractionResult> materialise(const std::string& input, const std::u16string& u, int32_t id, const int32_t* caps,
                                                  bool safe) const {
        if (id == -1) return nullptr;
        if (id <= -2) {
            const CookedExtraction& x = extractions_[static_cast<size_t>(-2 - id)];
            if (safe) return nullptr;  // core/Gorp.java:178-185
            throw ExtractionException(input, "Internal error: high-level match for extraction #" + std::to_string(-2 - id) + " (" + x.name +
                                                 ") failed to match generated regexp");
        }
        const CookedExtraction& x = extractions_[static_cast<size_t>(id)];
        std::vector<std::pair<bool, std::string>> values;
        const int ng = gx_num_groups(h_, id);
        for (int g = 0; g < ng; ++g) {
            const int32_t b = caps[2 * g], e = caps[2 * g + 1];
            if (b < 0) values.emplace_back(false, std::string());
            else values.emplace_back(true, to_utf8(u.substr(static_cast<size_t>(b), static_cast<size_t>(e - b))));
        }
        return std::unique_ptr<ExtractionResult>(new ExtractionResult(&x, input, std::move(values)));
    }

    static std::u16string to_utf16(const std::string& s) {
        std::u16string out;
        for (size_t i = 0; i < s.size();) {
            uint32_t cp = static_cast<unsigned char>(s[i]);
            int extra = cp < 0x80 ? 0 : (cp >> 5) == 6 ? 1 : (cp >> 4) == 14 ? 2 : 3;
            cp = extra == 0 ? cp : cp & (0x3F >> extra);
            ++i;
            for (int k = 0; k < extra && i < s.size(); ++k, ++i) cp = (cp << 6) | (static_cast<unsigned char>(s[i]) & 0x3F);
            if (cp > 0xFFFF) {
                cp -= 0x10000;
                out.push_back(static_cast<char16_t>(0xD800 | (cp >> 10)));
                out.push_back(static_cast<char16_t>(0xDC00 | (cp & 0x3FF)));
            } else out.push_back(static_cast<char16_t>(cp));
        }
        return out;
    }
    static std::string to_utf8(const std::u16string& s) {
        std::string out;
        for (size_t i = 0; i < s.size(); ++i) {
            uint32_t cp = s[i];
            if (cp >= 0xD800 && cp <= 0xDBFF && i + 1 < s.size()) { cp = 0x10000 + ((cp & 0x3FF) << 10) + (s[i + 1] & 0x3FF); ++i; }
            if (cp < 0x80) out += static_cast<char>(cp);
            else if (cp < 0x800) { out += static_cast<char>(0xC0 | (cp >> 6)); out += static_cast<char>(0x80 | (cp & 0x3F)); }
            else if (cp < 0x10000) {
                out += static_cast<char>(0xE0 | (cp >> 12)); out += static_cast<char>(0x80 | ((cp >> 6) & 0x3F)); out += static_cast<char>(0x80 | (cp & 0x3F));
            } else {
                out += static_cast<char>(0xF0 | (cp >> 18)); out += static_cast<char>(0x80 | ((cp >> 12) & 0x3F));
                out += static_cast<char>(0x80 | ((cp >> 6) & 0x3F)); out += static_cast<char>(0x80 | (cp & 0x3F));
            }
        }
        return out;
    }
};

// Line ingestion (gx_split_lines): BufferedReader.readLine() boundaries of a raw text buffer as CSR offsets; the lines
// keep their terminators, so pass gx_batch_opts.strip_eol = 1 to extractBatch.
inline std::vector<uint32_t> splitLines(const uint8_t* bytes, uint64_t size) {
    std::vector<uint32_t> offsets(static_cast<size_t>(size) + 2);
    uint64_t n = 0;
    int rc = gx_split_lines(bytes, size, offsets.data(), size + 1, &n, nullptr, nullptr);
    if (rc != GX_OK) throw GorpError(rc, gx_last_error());
    offsets.resize(static_cast<size_t>(n) + 1);
    return offsets;
}

// gx_utf8_to_utf16: the UTF-8 lines of a CSR batch (offsets as splitLines gives them) as the UTF-16 code units of the Strings Java
// would see -- new InputStreamReader(in, "UTF-8") -- with their offsets in units: directly a gx_batch_opts.utf16 batch.
inline std::pair<std::u16string, std::vector<uint32_t>> utf8ToUtf16(const uint8_t* bytes, const std::vector<uint32_t>& offsets) {
    if (offsets.empty()) throw GorpError(GX_E_ARG, "utf8ToUtf16: offsets has n + 1 entries");
    const uint64_t n = offsets.size() - 1;
    uint64_t units = 0;
    int rc = gx_utf8_to_utf16(bytes, offsets.data(), n, nullptr, 0, nullptr, &units, nullptr);
    if (rc != GX_OK) throw GorpError(rc, gx_last_error());
    std::u16string out(static_cast<size_t>(units), u'\0');
    std::vector<uint32_t> unitOffsets(offsets.size());
    rc = gx_utf8_to_utf16(bytes, offsets.data(), n, reinterpret_cast<uint16_t*>(&out[0]), units, unitOffsets.data(), &units, nullptr);
    if (rc != GX_OK) throw GorpError(rc, gx_last_error());
    return {std::move(out), std::move(unitOffsets)};
}

// core/DefinitionReader.java
class DefinitionReader {
public:
    static DefinitionReader reader(const std::string& contents, const std::string& sourceRef = "<input string>") {
        return DefinitionReader(contents, sourceRef);
    }
    // flags: 0, or GX_CREATE_HOST_ONLY to parse and compile without touching a GPU
    std::unique_ptr<Gorp> read(uint32_t flags = 0) const {
        gx_handle* h = nullptr;
        int rc = gx_create_from_definition(text_.c_str(), ref_.c_str(), flags, &h);
        if (rc == GX_E_DEFINITION || rc == GX_E_REGEX_SYNTAX || rc == GX_E_UNSUPPORTED_CONSTRUCT || rc == GX_E_LIMIT)
            throw DefinitionParseException(rc, gx_last_error());
        if (rc != GX_OK) throw GorpError(rc, gx_last_error());
        std::vector<CookedExtraction> xs;
        for (int32_t k = 0; k < gx_num_extractions(h); ++k) {
            CookedExtraction x;
            x.name = gx_extraction_name(h, k);
            for (int32_t g = 0; gx_extractor_name(h, k, g); ++g) x.extractorNames.push_back(gx_extractor_name(h, k, g));
            if (const char* a = gx_extraction_append_json(h, k)) x.appendJson = a;
            for (int32_t j = 0; j < gx_extraction_append_count(h, k); ++j)
                x.extra.emplace_back(gx_extraction_append_key(h, k, j), gx_extraction_append_value_json(h, k, j));
            xs.push_back(std::move(x));
        }
        return std::unique_ptr<Gorp>(new Gorp(h, std::move(xs)));
    }

private:
    DefinitionReader(std::string t, std::string r) : text_(std::move(t)), ref_(std::move(r)) {}
    std::string text_, ref_;
};

}  // namespace gorp
