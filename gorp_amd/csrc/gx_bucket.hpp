// gx_bucket.hpp -- the rule of gx_bucket_lines, once: plain C++ for the host (g++ alone: tests/cpp/bucket_test.cpp) and for the kernels
// (gx_bucket.hip).  No HIP in here.  On top of gx_group.hpp: the parts' shape, the hash's finishing mix, the order-preserving word, the
// per-slot words and group_stats_out are that header's.
//
// The reference's caller counts and measures per interval of a captured number right behind the extraction (README.md:26,63-79, with a
// timestamp field):
//     r = gorp.extract(line);
//     if (r != null) {
//         long b = Math.floorDiv(Instant.parse(r.asMap().get("ts")).toEpochMilli() - origin, 60_000L);
//         perMinute.merge(b, 1L, Long::sum);                                            // a TreeMap: buckets in time order
//         latency.computeIfAbsent(b, x -> new Stats()).record(Long.parseLong(r.asMap().get("timeTakenInMsec")));
//     }
// A PART names, for the lines of one extraction, the group whose value is the line's NUMBER (parsed under its gx_number_format and
// classed as gx_capture_stats classes a value: unset, no number, a number) and optionally a group measured per bucket as gx_group_lines
// measures one per key.  All parts share one bucket space.  A line counts by gx_capture_stats' rule.  A number v has the bucket
//     b = floor((v - origin) / width),          width >= 1
// exact for every int64 v and origin: the difference needs 65 bits, so it is taken in unsigned 64-bit arithmetic on the two sides of
// origin (bucket_of), with no 128-bit type -- the device has no 128-bit divide.  A bucket outside [INT64_MIN + 1, INT64_MAX] is OUT OF
// RANGE and the line has no bucket.  This differs from Java on purpose: Math.subtractExact would throw where v - origin overflows, while
// here the difference is exact and only the bucket number is limited.  Only the bucket number is delivered, never origin + b * width,
// which can overflow.
//
// The buckets live in a hash table of 64-bit words, word = group_max_word(b), the order-preserving unsigned form; 0 = empty, which is
// why INT64_MIN is no bucket.  The word is the WHOLE key, so a slot claimed by one 64-bit compare-and-swap is complete the moment it is
// visible -- no flag, no fence, no lane that waits for another lane (gx_group.hpp's argument, without even a batch to read back).
// Every loop is bounded: probing visits every slot at most once, then reports GROUP_NONE ("full").  Buckets leave in ascending order of
// their number: an LSD radix sort of the occupied slots' words over the digits bucket_digits plans.
//
// Not in scope: a text key beside the bucket (a series per verb), empty buckets filled in, calendar widths (months, local days),
// quantiles per bucket.
#pragma once
#include <cstdint>

#include "gx_group.hpp"

namespace gx {

constexpr uint32_t BUCKET_MAX_PARTS = GROUP_MAX_PARTS;
constexpr uint64_t BUCKET_MAX_BUCKETS = GROUP_MAX_KEYS;   // max_buckets <= 2^30: group_slots gives at most 2^31 slots
constexpr uint32_t BUCKET_ALL_DIGITS = 2u;                // GX_BUCKET_ALL_DIGITS of include/gorp_hip.h
// the lines a workgroup of the build pass covers in one step of its loop (one lane per line); below 2 048 workgroups' worth of lines a
// workgroup covers exactly these and no others
constexpr uint32_t BUCKET_WG_LINES = 256;
constexpr uint32_t BUCKET_DIGIT_BITS = 6, BUCKET_MAX_DIGITS = 11;   // 11 x 6 = 66 >= 64

// b = floor((v - origin) / width) for width >= 1.  false: the bucket is outside [INT64_MIN + 1, INT64_MAX] -- out of range, *b untouched.
GX_WHERE_HD bool bucket_of(int64_t v, int64_t origin, uint64_t width, int64_t* b) {
    if (v >= origin) {
        const uint64_t d = static_cast<uint64_t>(v) - static_cast<uint64_t>(origin);   // (exact: 0 .. 2^64 - 1)
        const uint64_t q = d / width;
        if (q > 0x7FFFFFFFFFFFFFFFull) return false;
        *b = static_cast<int64_t>(q);
        return true;
    }
    const uint64_t d = static_cast<uint64_t>(origin) - static_cast<uint64_t>(v);       // (exact: 1 .. 2^64 - 1)
    const uint64_t q = d / width + (d % width != 0 ? 1u : 0u);                          // (<= 2^64 - 1: the ceiling of d / width, d >= 1 so q >= 1)
    if (q > 0x7FFFFFFFFFFFFFFFull) return false;                                        // (-2^63 is INT64_MIN: no bucket)
    *b = -static_cast<int64_t>(q);
    return true;
}

GX_WHERE_HD uint64_t bucket_word(int64_t b) { return group_max_word(b); }     // (b > INT64_MIN: never 0)
GX_WHERE_HD int64_t bucket_number(uint64_t word) { return group_max_of(word); }

// The first slot of a word: group_hash's finishing mix over the word.  weak: GX_GROUP_WEAK_HASH's cut to the low 3 bits.
GX_WHERE_HD uint64_t bucket_hash(uint64_t word, bool weak) {
    uint64_t h = word;
    h ^= h >> 33;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    h *= 0xC4CEB9FE1A85EC53ull;
    h ^= h >> 33;
    return weak ? (h & 7ull) : h;
}

// Find-or-insert of `word` (!= 0): its slot, or GROUP_NONE when every slot holds another word.  table: group_find_or_insert's policy
// (load, claim).  A slot goes from empty to full once and never back, so a failed claim hands back the word that beat it.
template <typename Table>
GX_WHERE_HD uint32_t bucket_find_or_insert(Table& table, uint32_t n_slots, uint64_t word, bool weak) {
    uint32_t slot = group_first_slot(bucket_hash(word, weak), n_slots);
    for (uint32_t probe = 0; probe < n_slots; ++probe) {
        uint64_t cur = table.load(slot);
        if (cur == 0) {
            cur = table.claim(slot, word);
            if (cur == 0) return slot;
        }
        if (cur == word) return slot;
        slot = (slot + 1u) & (n_slots - 1u);
    }
    return GROUP_NONE;
}

typedef GroupHostTable BucketHostTable;

// The digit plan of the sort: 6-bit digits from the lowest, as many as cover the highest bit in which the smallest and the largest word
// differ -- 0 for one bucket, at most 11.  (Words between the two agree with both above that bit.)
GX_WHERE_HD uint32_t bucket_digits(uint64_t min_word, uint64_t max_word) {
    uint64_t x = min_word ^ max_word;
    uint32_t bits = 0;
    while (x) { ++bits; x >>= 1; }
    return (bits + BUCKET_DIGIT_BITS - 1u) / BUCKET_DIGIT_BITS;
}
GX_WHERE_HD uint32_t bucket_digit(uint64_t word, uint32_t d) { return static_cast<uint32_t>(word >> (d * BUCKET_DIGIT_BITS)) & 63u; }

// The parts as the kernel reads them, built by the host (gx_api.cpp: bucket_image) and copied to LDS by every workgroup: GroupHead's
// scheme (ext[] ascending, searched with where_find), part[].key_group the NUMBER group, and both groups' packed number formats.
struct BucketHead {
    uint32_t n_parts, flags, has_values;
    uint32_t formats;                 // != 0: some format is not LONG -- the build pass's instantiation that reads them
    int64_t origin;
    uint64_t width;                   // >= 1
    uint32_t ext[BUCKET_MAX_PARTS];
    GroupPart part[BUCKET_MAX_PARTS];
    uint8_t nfmt[BUCKET_MAX_PARTS];   // part[e].key_group's (the number's) packed format, 0 = LONG
    uint8_t vfmt[BUCKET_MAX_PARTS];   // part[e].value_group's
};
static_assert(sizeof(BucketHead) % 16 == 0, "the head is copied in 16-byte words");

// What the build pass leaves for the host, read in ONE wait with the number of buckets (status bit 1: a line of 4 G units, 2: the table
// is full).  min_inv is the maximum of ~word, max_word the maximum of word; both 0 without a bucket.
struct BucketDev {
    uint64_t lines, unset, status, not_numbers, out_of_range, min_inv, max_word, spare;
};
static_assert(sizeof(BucketDev) == 64, "the host reads it from device memory as it is");

}  // namespace gx
