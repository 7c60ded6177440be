// gx_device.hpp -- device-side view of the compiled tables + kernel launch entry points.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include "gx_layout.hpp"

namespace gx {

// All pointers are device pointers into ONE allocation (the uploaded table image).
struct GxDev {
    // class maps
    const uint8_t* cls256;       // [256]
    const uint16_t* hi_lo;       // [n_hi] ascending lower bounds, hi_lo[0] == 256
    const uint16_t* hi_cls;      // [n_hi]
    int32_t n_hi;
    int32_t ncls;
    // match automaton (total; m_dead absorbing)
    const uint16_t* m_next16;    // [m_states * ncls] when m_states <= 65536, else null
    const uint32_t* m_next32;    // [m_states * ncls] otherwise
    const int32_t* m_accept_first;  // [m_states]
    int32_t m_states;
    int32_t m_dead;
    // capture automata, all extractions concatenated
    const uint32_t* c_trans;     // rule k at c_trans + c_trans_off[k], [n_states_k * ncls]
    const uint32_t* c_trans_off; // [n_rules]
    const int32_t* c_fin;        // rule k at c_fin + c_fin_off[k], [n_states_k]
    const uint32_t* c_fin_off;   // [n_rules]
    const int32_t* c_ngroups;    // [n_rules]
    const uint32_t* ops_off;     // [n_oplists + 1] in (dst,src) pairs
    const uint16_t* ops;         // pairs
    const uint16_t* fin_tags;
    int32_t n_rules;
    int32_t max_groups;
    int32_t max_regs;
    int32_t has_capture;
    // extractions without a capture automaton (gx_compile.hpp: Tables::pike_*): their programs, run as they are.  pike_off null: none.
    const uint32_t* pike_off;    // [n_rules + 1]
    const uint32_t* pike_code;   // two words per instruction
    const uint32_t* pike_sets;   // eight words per set
    int32_t* pike_scratch;       // [256 pike_blocks + 1][pike_lane_ints]: the thread lists of the lanes that run one (the last: the one-line calls)
    uint32_t pike_lane_ints;
    uint32_t pike_blocks;        // the per-line kernels of a handle that has such extractions run this many workgroups of 256 lanes at most
};
constexpr uint32_t GX_PIKE_BLOCKS = 64;                     // ... 64 when the thread lists of 16 K lanes stay within GX_PIKE_SCRATCH_BYTES, else fewer
constexpr uint64_t GX_PIKE_SCRATCH_BYTES = 256ull << 20;

// GxLds, the layout of a batch kernel's table image in LDS, and the constants it is planned with: gx_layout.hpp

struct GxBatch {
    const void* data;      // uint8_t (Latin-1) or uint16_t (UTF-16) code units
    const void* offsets;   // uint32_t or uint64_t [n + 1], in code units
    uint64_t n;
    int32_t* match_id;     // [n]
    int32_t* caps;         // [n * 2 * max_groups] or null when match_only
    int32_t* state_out;    // optional [n]: final match-automaton state (for PolyMatcher.match)
    int32_t wide;          // 1: data is uint16_t
    int32_t offsets64;
    int32_t match_only;
    int32_t strip_eol;     // 1: every line carries its terminator ("\n", "\r\n" or "\r"), to be ignored
    // compact result rows (gx_batch_opts.compact_results): per line u16[1 + 2 * max_groups] = int16 match id, then the
    // capture offsets (0xFFFF = unset) -- written instead of match_id / caps when `packed` is set
    uint16_t* packed;
    unsigned long long* overflow;  // with `packed`: += number of offsets above 65534 (stored saturated)
    // narrow rows (compact_results = 2): `packed` holds u8[1 + 2 * max_groups] per line instead -- int8 match id, offsets with
    // 0xFF = unset, an offset above 254 stored as 254 and counted in *overflow
    int32_t narrow;
    // lines the tile kernel cannot stage (longer than its staging area) are left to a follow-up launch of the
    // per-line kernel: the tile kernel puts `seq` into *oversize_flag when it meets one (announce_left_line below); the word
    // GX_SLOT_WORDS behind it counts the launches that did
    uint32_t* oversize_flag;
    uint32_t seq;
    // lane kernel, length-sorted mode: the launch's chunk counter (never reset: chunk = ticket - chunk_base; a launch draws
    // one ticket per chunk and one more per workgroup)
    uint32_t* chunk_ctr;
    uint32_t chunk_base;
    // the host knows that no line of the batch is beyond what the chosen kernel stages (the one-line calls: the host has the line;
    // batches: the caller's promise, gx_batch_opts.max_line_bytes): no follow-up launch of the per-line kernel behind the batch
    // kernel.  oversize_flag then points to a word in pinned HOST memory: a kernel that meets such a line after all says so there,
    // and the host tells this launch's break from an earlier one's by the count behind the word (gx_slots.hpp).
    uint32_t no_followup;
    uint32_t max_line_bytes;   // the promise itself (0: none)
    uint32_t caller_no_sync;   // host side only: the caller asked for no synchronisation (gx_batch_opts.no_sync): a path that needs one refuses
    // tile kernel: the workgroups' tile counters, u32[2][GX_STEAL_MAX * GX_STEAL_STRIDE] of the launch's stream slot (every GX_STEAL_STRIDE-th word is a counter).  A launch draws from row
    // steal_parity and zeroes the other row, which the stream's next launch draws from.
    uint32_t* steal;
    uint32_t steal_parity;
    // tile kernel on UTF-16 code units (wide = 1): flags[n] (1: the line holds a unit above 0xFF; launch_extract_flagged takes it
    // again) and the word that receives `seq` when there is any such line
    uint8_t* wide_flags;
    uint32_t* wide_any;
};

// A handle's flag words come in blocks of GX_SLOT_WORDS (= LaunchSlots::N, one word per launch slot): a slot's flag word, and
// GX_SLOT_WORDS words behind it the count of the slot's launches that have left a line.
constexpr uint32_t GX_SLOT_WORDS = 32;

#ifdef __HIPCC__
// A batch kernel leaves a line to the follow-up launch (or, under a max_line_bytes promise, to nobody): `seq` into the launch's
// flag word, and one more launch in the slot's count if this is the launch's first such line -- the launches of a slot run one
// after the other, so the word holds another number until then.  System scope: the words may be in pinned host memory.
__device__ inline void announce_left_line(uint32_t* flag, uint32_t seq) {
    if (__hip_atomic_exchange(flag, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != seq)
        __hip_atomic_fetch_add(flag + GX_SLOT_WORDS, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
#endif

// More than 64 KiB of dynamic LDS needs the attribute, once per kernel (= per instantiation of this template) and
// per device.
template <typename K>
inline hipError_t allow_full_lds(K kernel) {
    static bool prepared[64] = {};  // (a benign race: setting the attribute twice is harmless)
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64 && prepared[dev]) return hipSuccess;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 163840);
    if (e == hipSuccess && dev >= 0 && dev < 64) prepared[dev] = true;
    return e;
}

// Generic kernel: any table size, any line length, bytes or UTF-16.
hipError_t launch_extract_generic(const GxDev& dev, const GxBatch& b, hipStream_t stream);

// UTF-16 batches: the units' low bytes -> `bytes_at_first_unit` (room for offsets[n] - offsets[0] bytes), flags[i] = 1 for a line
// with a unit above 0xFF; launch_extract_flagged takes those lines again on the code units (per-line walk).
hipError_t launch_narrow_units(const GxBatch& b, uint8_t* bytes_at_first_unit, uint8_t* flags, hipStream_t stream);
// any_word != nullptr: every wave leaves at once unless *any_word == b.seq (the tile kernel's "there was such a line")
hipError_t launch_extract_flagged(const GxDev& dev, const GxBatch& b, const uint8_t* flags, hipStream_t stream, const uint32_t* any_word = nullptr);
// the same walk for the `count` lines whose numbers list[] holds: a lane per LISTED line, so that few flagged lines among many fill
// their waves (UTF-16 code units, 64-bit offsets)
hipError_t launch_extract_listed(const GxDev& dev, const GxBatch& b, const uint64_t* list, uint64_t count, hipStream_t stream);

// Tile kernel (gx_tile.hip): 64-line tiles staged through LDS with coalesced loads, self-loop runs skipped by SWAR
// tests and a per-chunk bitmap.  Byte input only.  `lds_image` is the device copy of the table image.
// at_global != nullptr selects the L2 tier: automaton rows are read from that global-memory table (row =
// state index, GxLds::row_bytes per row) instead of from LDS.  A line longer than the staging area is not
// processed: the kernel stores b.seq into *b.oversize_flag and launch_extract_oversize (same stream, right after)
// takes those lines with the per-line kernel.  dev_stamps: developer builds (-DGX_DEV) only, else ignored.
hipError_t launch_extract_tile(const GxDev& dev, const GxLds& lds, const uint8_t* lds_image, const uint8_t* at_global, int num_cus,
                               const GxBatch& b, hipStream_t stream, unsigned long long* dev_stamps);
// by_length 0: the lines for which (bytes in memory) + (address & 15) + 48 > limit (the tile kernel's staging predicate, limit =
// GxLds::stage_bytes); 1: the lines longer than `limit` bytes without their terminator (lane and hop slice kernels: 65 535, or
// 65 534 with compact rows under the lane kernel).
hipError_t launch_extract_oversize(const GxDev& dev, const GxBatch& b, uint32_t limit, int by_length, hipStream_t stream);
// Lane kernel (gx_lanes.hip): tables in global memory (GxLds::tier 1 or 3), every lane keeps its own line in registers;
// lds.nwaves waves per workgroup; lds.regs_wave_bytes = the wave's LDS area (register block of lds.stage_bytes bytes + result rows).
// Lines longer than 65 535 bytes are left to launch_extract_oversize (stage_bytes = 65 535 + 48).
// (with lds.sort_chunk set the launch draws lanes_sorted_tickets(...) tickets from *b.chunk_ctr)
uint32_t lanes_sorted_tickets(uint64_t n, uint32_t chunk_lines, int num_cus);
hipError_t launch_extract_lanes(const GxDev& dev, const GxLds& lds, const uint8_t* lds_image, const uint8_t* at_global, int num_cus,
                                const GxBatch& b, hipStream_t stream, unsigned long long* dev_stamps);
// Slice kernel: the same tables, lines staged 64 bytes at a time (GxLds::stage_bytes = 64 * 80); fused automaton or match only.
hipError_t launch_extract_slices(const GxDev& dev, const GxLds& lds, const uint8_t* lds_image, const uint8_t* at_global, int num_cus,
                                 const GxBatch& b, hipStream_t stream);

// Hop slice kernel: the hop tier's tables (GxLds::tier 4), lines staged GX_HOP_SLICE_BYTES at a time from each lane's own
// position (GxLds::stage_bytes = 64 * (GX_HOP_SLICE_BYTES + 16) + 16); captures only.
hipError_t launch_extract_hop_slices(const GxDev& dev, const GxLds& lds, const uint8_t* lds_image, const uint8_t* at_global, int num_cus,
                                     const GxBatch& b, hipStream_t stream, unsigned long long* stamps = nullptr);
// (with b.chunk_ctr set the launch draws hop_slices_tickets(...) tickets from it: the pool of chunks its waves share)
uint32_t hop_slices_tickets(uint64_t n, uint32_t nwaves, int num_cus);

// The resident one-line service (gx_service.hip): one wave, the dense-rows image in LDS, requests through `mailbox` and answers
// through `answer` (both pinned host memory, device addresses), `state` (pinned): 1 resident, 2 gone.  mode 0: match automaton
// alone, 1: fused automaton with "register := position" programs.
hipError_t launch_one_service(int mode, const GxLds& lds, const uint8_t* lds_image, const uint32_t* mailbox, int32_t* answer, uint32_t* state,
                              uint32_t last_seq, int max_groups, unsigned long long idle_ticks, unsigned long long life_ticks, hipStream_t stream);

// Line ingestion (gx_ingest.hip): raw bytes -> CSR offsets of readLine()-style lines, terminators included.
// `workspace` holds split_workspace_bytes(size) bytes; *d_n_lines receives the device address of the line count.
size_t split_workspace_bytes(uint64_t size, bool with_flags = false);
// d_max_line (optional): *d_max_line receives the device address of the longest line's length, terminator included.
// esc_bits (optional, 32-bit offsets, no line flags): 2 048 u16 per 32 KiB of text (whole blocks: ((size + 32767) / 32768) * 4096 bytes), a bit per byte of the text that takes ONE more byte inside a JSON string, and
// the word behind the longest line (d_max_line[1]) != 0 when some byte takes five more (a control character): launch_jsonl_sizes.
hipError_t launch_split_lines(const uint8_t* data, uint64_t size, void* offsets, int offsets64, uint64_t cap_lines, uint8_t* flags,
                              void* workspace, uint64_t** d_n_lines, hipStream_t stream, uint64_t** d_max_line = nullptr,
                              uint16_t* esc_bits = nullptr, int passthrough = 0);


// Result materialisation (gx_jsonl.hip): per-extraction JSON templates on the device.  A template is a list of
// segments; segment s = literal bytes lits[lit_off[s] .. +lit_len[s]) followed by capture group group[s] (-1: none).
struct GxJsonl {
    const uint32_t* seg_off;    // [n_rules + 1]
    const uint32_t* lit_off;    // [n_segs]
    const uint32_t* lit_len;    // [n_segs]
    const int32_t* group;       // [n_segs]
    const uint32_t* fixed_len;  // [n_rules] sum of the template's literal lengths
    const uint8_t* lits;
    uint32_t lits_bytes, n_rules, n_segs;
};
size_t jsonl_workspace_bytes(uint64_t n);
// one line out of / into pinned host memory (gx_kernels.hip: k_extract_one); hipErrorInvalidValue for a line of more than 16 384 code units
hipError_t launch_extract_one(const GxDev& dev, const uint16_t* units, uint32_t len, const GxBatch& b, hipStream_t stream);
// mean_in / mean_out: mean bytes per line of input and of output text; they size the LDS staging of the tile kernels
// esc_bits (optional): launch_split_lines' bits of this batch's text, when its hard word is 0: the sizes come from the bits, not the text
hipError_t launch_jsonl_sizes(const GxJsonl& tm, const GxBatch& b, int slots, int passthrough, uint32_t mean_in, uint64_t* line_out_off,
                              void* workspace, hipStream_t stream, const uint32_t* esc_bits = nullptr);
hipError_t launch_count_outcomes(const int32_t* match_id, uint64_t n, unsigned long long* d_counts, hipStream_t stream);
hipError_t launch_pack_results(const int32_t* match_id, const int32_t* caps, uint64_t n, int slots, uint16_t* packed,
                               unsigned long long* d_overflow, hipStream_t stream);
hipError_t launch_unpack_results(const uint16_t* packed, uint64_t n, int slots, int32_t* match_id, int32_t* caps, hipStream_t stream);
hipError_t launch_unpack_results8(const uint8_t* rows, uint64_t n, int slots, int32_t* match_id, int32_t* caps, hipStream_t stream);
hipError_t launch_jsonl_write(const GxJsonl& tm, const GxBatch& b, int slots, int passthrough, uint32_t mean_in, uint32_t mean_out,
                              const uint64_t* line_out_off, uint8_t* out, void* workspace, hipStream_t stream);

// Outcomes of a finished batch (gx_select.hip): the histogram over the outcome index (2K + 2 bins) and the selection of lines by
// outcome.  The passes' device workspace, cut out of one allocation of select_workspace_bytes(n, K, select) bytes:
struct SelectWs {
    unsigned long long* counts;   // [2K + 2]
    uint32_t* status;             // != 0: a line of 4 G code units or more
    uint8_t* want;                // [2K + 1] the mask, put there by the caller of launch_select_flags
    uint32_t* slab;               // the workgroups' histograms
    uint64_t* block_sums;         // the scans'
    uint64_t* idx_off;            // [n + 1] kept lines before line i; [n]: all of them
    uint64_t* dst_off;            // [n + 1] kept code units before line i; [n]: all of them
    uint32_t* klen;               // [n] the line's code units when it is kept, else 0
    uint8_t* flags;               // [n] kept
    size_t bytes;
};
SelectWs select_workspace(void* ws, uint64_t n, uint32_t K, bool select);   // select = false: counts, status and slab alone
size_t select_workspace_bytes(uint64_t n, uint32_t K, bool select);
// what the copy pass writes, each part optional (nullptr): the kept lines' numbers, their code units, their offsets (the width of the
// input's), and up to two fixed-size columns (result rows; or match ids and dense capture rows)
struct SelectOut {
    uint32_t* index;
    void* bytes;
    void* offsets;
    const void* col_src[2];
    void* col_dst[2];
    uint32_t col_width[2];        // units per line
    uint32_t col_unit_bytes[2];   // 1, 2 or 4
};
// ids: int32[n] (ROWS_DENSE, row_units 1) or rows of row_units units whose first is the id.  offsets == nullptr: counts alone.
hipError_t launch_select_flags(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64,
                               const SelectWs& w, hipStream_t stream);
hipError_t launch_select_copy(const SelectOut& o, const void* data, const void* offsets, int offsets64, int wide, uint64_t n, const SelectWs& w,
                              hipStream_t stream);
constexpr uint32_t SELECT_LDS_BINS = 8192;   // bins a workgroup's LDS histogram takes (32 KiB, the want mask behind it)
hipError_t launch_select_scans(uint64_t n, const SelectWs& w, hipStream_t stream);   // the two scans behind either flags pass

// The flags pass of gx_select_lines_where (gx_where.hip; the rule: gx_where.hpp), in launch_select_flags' place: a kept line's outcome
// is wanted AND, where its extraction has terms, every term holds on what the line captured.
struct WhereArgs {
    const void* data;      // the batch's code units
    int wide;              // 1: UTF-16 code units
    const int32_t* caps;   // ROWS_DENSE: [n][slots]; compact rows carry their offsets themselves
    uint32_t slots;        // 2 * max_groups
    const void* image;     // WhereHead + the literals, on the device, 16-byte aligned
    uint32_t image_bytes;  // a multiple of 16
    uint32_t formats;      // WhereHead::formats: a term's group has a number format other than LONG
};
// counts: also the histogram of outcomes in w.counts
hipError_t launch_where_flags(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64,
                              const WhereArgs& a, bool counts, const SelectWs& w, hipStream_t stream);

// The reduction of gx_capture_stats (gx_stats.hip; the rule: gx_stats.hpp): per measure -- one group of one extraction -- the lines
// that count, classed as numbers / unset / no numbers, and the numbers' minimum, maximum, exact sum and histogram.
struct StatsArgs {
    const void* data;            // the batch's code units
    int wide;                    // 1: UTF-16 code units
    const int32_t* caps;         // ROWS_DENSE: [n][slots]; compact rows carry their offsets themselves
    uint32_t slots;              // 2 * max_groups
    const void* image;           // StatsHead + the edges, on the device, 16-byte aligned
    uint32_t image_bytes;        // a multiple of 16
    const void* where_image;     // WhereHead + the literals, or nullptr: no terms
    uint32_t where_image_bytes;  // a multiple of 16; 0: no terms
    uint32_t n_measures, n_bins;
    uint32_t formats;            // a measure's or a term's group has a number format other than LONG
};
uint32_t stats_blocks(uint64_t n);
size_t stats_workspace_bytes(uint64_t n, uint32_t n_measures, uint32_t n_bins);
// n > 0, a.n_measures > 0.  Leaves in ws: n_measures x STATS_WORDS 64-bit words, then n_bins 64-bit bins, then the status word
// (!= 0: a line of 4 G code units or more).
hipError_t launch_capture_stats(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const StatsArgs& a,
                                void* ws, hipStream_t stream);

// The lines of a finished batch grouped by the text they captured (gx_group.hip; the rule: gx_group.hpp): a hash table of the distinct
// values, per value its first line, its lines and -- with a value group -- what gx_capture_stats would say of them, and per line the
// number of its value.
struct GroupArgs {
    const void* data;            // the batch's code units
    int wide;                    // 1: UTF-16 code units
    const int32_t* caps;         // ROWS_DENSE: [n][slots]; compact rows carry their offsets themselves
    uint32_t slots;              // 2 * max_groups
    const void* image;           // GroupHead, on the device, 16-byte aligned
    const void* where_image;     // WhereHead + the literals, or nullptr: no terms
    uint32_t where_image_bytes;  // a multiple of 16; 0: no terms
    uint32_t has_values;         // a part has a value group: the slots have stats words
    uint32_t formats;            // a value group's or a term's group has a number format other than LONG
};
// The passes' device workspace: the slots' words (group_table_bytes) and the per-line arrays (group_lines_bytes).
struct GroupWs {
    uint32_t n_slots;             // a power of two
    uint64_t* table;              // [n_slots] the slot words
    uint64_t* head_words;         // [n_slots][GROUP_HEAD_WORDS]
    uint64_t* stats_words;        // [n_slots][GROUP_STATS_WORDS], with values
    uint64_t* totals;             // [8]: lines that count, lines without a key, status bits (1: a line of 4 G units, 2: the table is full)
    uint32_t* keynum;             // [n_slots] the slot's key number, written by the emit pass (gx_top_groups' emit: the rank of the slot's key)
    uint64_t* idx_off;            // [n + 1] first lines before line i; [n]: the keys
    uint64_t* dst_off;            // [n + 1] key units before line i's; [n]: all of them
    uint64_t *sums_a, *sums_b;    // the scans'
    uint32_t* slot_of;            // [n] the line's slot, GROUP_NONE: it has no key
    uint32_t* klen;               // [n] the key's units where the line is its key's first, else 0
    uint8_t* flags;               // [n] the line is its key's first
};
// what the emit pass writes, each part optional (nullptr)
struct GroupOut {
    void* key_units;
    void* key_offsets;
    uint32_t* key_first_line;
    uint64_t* key_lines;
    uint64_t* key_stats;          // [n_keys][8]: gx_measure_stats' fields
    uint32_t* line_key;
    int offsets64;                // key_offsets: uint64, else uint32
};
size_t group_table_zero_bytes(uint32_t n_slots, bool values);
size_t group_table_bytes(uint32_t n_slots, bool values);
size_t group_lines_bytes(uint64_t n);
GroupWs group_workspace(void* table_mem, void* lines_mem, uint64_t n, uint32_t n_slots, bool values);
// n > 0, parts > 0.  Build, flags and the two scans; then -- behind the host's look at w.totals, w.idx_off[n], w.dst_off[n] -- the emit.
hipError_t launch_group_build(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const GroupArgs& a,
                              const GroupWs& w, hipStream_t stream);
hipError_t launch_group_emit(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const GroupArgs& a,
                             const GroupWs& w, const GroupOut& out, uint64_t n_keys, uint64_t key_units, hipStream_t stream);

// The lines of a finished batch looked up in a dictionary the caller supplies (gx_lookup.hip; the rule: gx_lookup.hpp): a table of the
// entries in gx_group.hpp's form, per entry the lowest entry with its text, its lines, first line and stats, per line its entry.
struct LookupDict {
    const void* units;            // the entries' code units (the batch's kind)
    const void* offsets;          // [m + 1], uint64 or uint32
    int offsets64;
    uint64_t m;
    uint32_t weak_hash;           // GROUP_WEAK_HASH is among the call's flags (the probe reads them from the part image, the build from here)
};
// The passes' device workspace: the slots' words (lookup_table_bytes), and the per-entry and per-line arrays (lookup_lines_bytes).
struct LookupWs {
    uint32_t n_slots;             // group_slots(m), a power of two
    uint64_t* table;              // [n_slots] the slot words
    uint64_t* low;                // [n_slots] the lowest entry with the slot's text (lookup_low_word)
    uint64_t* head_words;         // [n_slots][GROUP_HEAD_WORDS]
    uint64_t* stats_words;        // [n_slots][GROUP_STATS_WORDS], with values
    uint64_t* totals;             // [8]: lines, unset, status bits (1: a line or an entry of 4 G units, 2: the table is full), hits, misses,
                                  //      distinct entries, hit entries
    uint32_t* slot_of_entry;      // [m] the entry's slot
    uint32_t* line_slot;          // [n] the line's slot, LOOKUP_MISS or LOOKUP_NONE
};
// what the emit passes write, each part optional (nullptr)
struct LookupOut {
    uint32_t* line_entry;
    uint32_t* entry_same;
    uint64_t* entry_lines;
    uint32_t* entry_first_line;
    uint64_t* entry_stats;        // [m][8]: gx_measure_stats' fields
};
size_t lookup_table_zero_bytes(uint32_t n_slots, bool values);
size_t lookup_table_bytes(uint32_t n_slots, bool values);
size_t lookup_lines_bytes(uint64_t n, uint64_t m);
LookupWs lookup_workspace(void* table_mem, void* lines_mem, uint64_t n, uint64_t m, uint32_t n_slots, bool values);
// Zeroes the slots' words, then (m > 0) k_lookup_build, (n > 0) k_lookup_probe, (m > 0) k_lookup_count: leaves w.totals.  a: the batch as
// launch_group_build takes it.  keep != 0: the probe also leaves sel->flags and sel->klen for launch_select_scans.
hipError_t launch_lookup_probe(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const GroupArgs& a,
                               const LookupDict& d, uint32_t keep, const LookupWs& w, const SelectWs* sel, hipStream_t stream);
// Behind the host's look at w.totals: k_lookup_emit over the entries (when a per-entry output is wanted) and k_lookup_line_entry.
hipError_t launch_lookup_emit(uint64_t n, uint64_t m, bool values, const LookupWs& w, const LookupOut& out, hipStream_t stream);

// The lines of a finished batch grouped by TWO captured texts (gx_pairs.hip; the rule: gx_pairs.hpp), behind gx_group_lines' passes on
// the same stream: a second table keyed by (key slot, second text).  The passes' device workspace: the pair slots' words
// (pairs_table_bytes) and the per-line arrays (pairs_lines_bytes).
struct PairsWs {
    uint32_t n_slots;             // pair slots, a power of two
    uint32_t n_key_slots;         // GroupWs::n_slots
    uint64_t* table;              // [n_slots] the pair slot words
    uint64_t* head_words;         // [n_slots][GROUP_HEAD_WORDS]: lines, first line
    uint64_t* kpairs;             // [n_key_slots] the pairs of the key slot
    uint64_t* totals;             // [8] PairsDev
    uint32_t* pairnum;            // [n_slots] the pair slot's pair number, written by the emit pass
    uint64_t* idx_off;            // [n + 1] first-of-pair lines before line i; [n]: the pairs
    uint64_t* dst_off;            // [n + 1] second units before line i's; [n]: all of them
    uint64_t *sums_a, *sums_b;    // the scans'
    uint32_t* pslot_of;           // [n] the line's pair slot, GROUP_NONE: it is not paired
    uint32_t* plen;               // [n] the second's units where the line is its pair's first, else 0
    uint8_t* flags;               // [n] the line is its pair's first
};
// what the pair emit writes, each part optional (nullptr)
struct PairsOut {
    void* pair_units;
    void* pair_offsets;
    uint32_t* pair_key;
    uint32_t* pair_first_line;
    uint64_t* pair_lines;
    uint64_t* key_pairs;
    uint32_t* line_pair;
    int offsets64;                // pair_offsets: uint64, else uint32
};
size_t pairs_table_zero_bytes(uint32_t n_slots, uint32_t n_key_slots);
size_t pairs_table_bytes(uint32_t n_slots, uint32_t n_key_slots);
size_t pairs_lines_bytes(uint64_t n);
PairsWs pairs_workspace(void* table_mem, void* lines_mem, uint64_t n, uint32_t n_slots, uint32_t n_key_slots);
// n > 0, parts > 0, behind launch_group_build (g.slot_of); pairs_image: a PairsHead on the device, 16-byte aligned.  Build, flags and
// the two scans; behind them the host reads w.totals, w.idx_off[n], w.dst_off[n].
hipError_t launch_pairs_build(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const GroupArgs& a,
                              const void* pairs_image, const GroupWs& g, const PairsWs& w, hipStream_t stream);
// Behind launch_group_emit (g.keynum) and the host's check of the capacities: n_pairs <= the per-pair arrays' capacity, pair_units <=
// pair_units' capacity, n_keys <= key_pairs' capacity.
hipError_t launch_pairs_emit(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const GroupArgs& a,
                             const void* pairs_image, const GroupWs& g, const PairsWs& w, const PairsOut& out, uint64_t n_pairs, uint64_t pair_units,
                             uint64_t n_keys, hipStream_t stream);

// The lines of a finished batch counted and measured per interval of a number they captured (gx_bucket.hip; the rule: gx_bucket.hpp): a
// hash table of the distinct bucket numbers with gx_group_lines' per-slot words, the buckets sorted by their number.  GroupArgs::image is
// a BucketHead here.  The passes' device workspace: the slots' words and arrays (bucket_table_bytes), the lines' slots
// (bucket_lines_bytes) and, sized by the buckets the host has read, the sort's (bucket_sort_workspace_bytes).
struct BucketWs {
    uint32_t n_slots;             // a power of two
    uint64_t* table;              // [n_slots] the slot words: group_max_word(bucket), 0 = empty
    uint64_t* head_words;         // [n_slots][GROUP_HEAD_WORDS]
    uint64_t* stats_words;        // [n_slots][GROUP_STATS_WORDS], with values
    uint64_t* totals;             // [8] BucketDev
    uint64_t* before;             // [n_slots + 1] occupied slots before slot s; [n_slots]: the buckets
    uint64_t* sums;               // the scan's
    uint32_t* rank_of_slot;       // [n_slots] the rank of the slot's bucket, written by the emit pass
    uint8_t* occupied;            // [n_slots]
    uint32_t* slot_of;            // [n] the line's slot, GROUP_NONE: it has no bucket
};
struct BucketSortWs {
    uint64_t* word[2];            // [m] the buckets' words, ping and pong
    uint32_t* slot[2];            // [m] their slots
    uint32_t* slab;               // the sort's counts, bin-major
    uint64_t* bases;              // their scan
    uint64_t* block_sums;
    size_t bytes;
};
// what the emit passes write, each part optional (nullptr)
struct BucketOut {
    int64_t* bucket_number;
    uint32_t* bucket_first_line;
    uint64_t* bucket_lines;
    uint64_t* bucket_stats;       // [n_buckets][8]: gx_measure_stats' fields
    uint32_t* line_bucket;
};
size_t bucket_table_zero_bytes(uint32_t n_slots, bool values);
size_t bucket_table_bytes(uint32_t n_slots, bool values);
size_t bucket_lines_bytes(uint64_t n);
BucketWs bucket_workspace(void* table_mem, void* lines_mem, uint64_t n, uint32_t n_slots, bool values);
size_t bucket_sort_workspace_bytes(uint64_t m);
BucketSortWs bucket_sort_workspace(void* ws, uint64_t m);
// n > 0, parts > 0.  Build, flags and the scan; then -- behind the host's look at w.totals and w.before[n_slots] -- the pairs, the sort
// over n_digits digits and the emits.
hipError_t launch_bucket_build(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const GroupArgs& a,
                               const BucketWs& w, hipStream_t stream);
hipError_t launch_bucket_emit(uint64_t n, uint64_t m, uint32_t n_digits, const BucketWs& w, const BucketSortWs& s, const BucketOut& out, hipStream_t stream);

// The lines of a finished batch counted and measured per (captured text, interval of a captured number) (gx_series.hip; the rule:
// gx_series.hpp), behind gx_group_lines' passes on the same stream: a one-word table of the distinct bucket numbers, a one-word table of
// the distinct (key slot, bucket slot) cells with gx_group_lines' per-slot words, the buckets sorted into an axis and the cells sorted by
// (key number, rank on the axis).  Its build pass adds to a cell slot with gx_group_dev.hpp's GroupAdd / group_add, as gx_group.hip's
// and gx_bucket.hip's do.  Both tables have n_slots slots.  The passes' device workspace: the slots' words and arrays
// (series_table_bytes), the lines' cell slots (series_lines_bytes) and, sized by the cells the host has read, the sorts'
// (series_sort_workspace_bytes).
struct SeriesWs {
    uint32_t n_slots;             // a power of two, of EACH table
    uint64_t* btable;             // [n_slots] the bucket slot words: group_max_word(bucket), 0 = empty
    uint64_t* ctable;             // [n_slots] the cell slot words: cell_word(key slot, bucket slot), 0 = empty
    uint64_t* head_words;         // [n_slots][GROUP_HEAD_WORDS] of the cell slots
    uint64_t* stats_words;        // [n_slots][GROUP_STATS_WORDS] of the cell slots, with values
    uint64_t* totals;             // [8] SeriesDev
    uint64_t *bbefore, *cbefore;  // [n_slots + 1] occupied slots before slot s; [n_slots]: the buckets, the cells
    uint64_t *bsums, *csums;      // the scans'
    uint32_t* rank_of_bslot;      // [n_slots] the bucket slot's index on the axis, written by k_series_axis
    uint32_t* rank_of_cslot;      // [n_slots] the cell slot's cell number, written by k_series_emit
    uint8_t *boccupied, *coccupied;   // [n_slots]
    uint32_t* cslot_of;           // [n] the line's cell slot, GROUP_NONE: it is in no cell
};
struct SeriesSortWs {
    BucketSortWs sort;            // for m cells; the buckets are sorted in it first
    uint32_t* knum;               // [m] the sorted cells' key numbers
};
// what the emit passes write, each part optional (nullptr)
struct SeriesOut {
    int64_t* bucket_number;
    uint32_t* cell_key;
    uint32_t* cell_bucket;
    uint32_t* cell_first_line;
    uint64_t* cell_lines;
    uint64_t* cell_stats;         // [n_cells][8]: gx_measure_stats' fields
    uint64_t* key_cell_begin;     // [n_keys + 1]
    uint32_t* line_cell;
};
size_t series_table_zero_bytes(uint32_t n_slots, bool values);
size_t series_table_bytes(uint32_t n_slots, bool values);
size_t series_lines_bytes(uint64_t n);
SeriesWs series_workspace(void* table_mem, void* lines_mem, uint32_t n_slots, bool values);
size_t series_sort_workspace_bytes(uint64_t m);
SeriesSortWs series_sort_workspace(void* ws, uint64_t m);
// n > 0, parts > 0, behind launch_group_build (g.slot_of); series_image: a SeriesHead on the device, 16-byte aligned; formats: a value
// group's or a number group's format is not LONG.  Build, flags and the two scans; behind them the host reads w.totals,
// w.bbefore[n_slots] and w.cbefore[n_slots].
hipError_t launch_series_build(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const GroupArgs& a,
                               const void* series_image, bool formats, const GroupWs& g, const SeriesWs& w, hipStream_t stream);
// Behind launch_group_emit (g.keynum) and the host's check of the capacities: the two sorts (b_digits, c_digits digits), the axis, the
// cells' rows, the keys' bounds and the lines' cells.  0 < n_buckets <= n_cells.
hipError_t launch_series_emit(uint64_t n, uint64_t n_keys, uint64_t n_buckets, uint64_t n_cells, uint32_t b_digits, uint32_t c_digits, const GroupWs& g,
                              const SeriesWs& w, const SeriesSortWs& s, const SeriesOut& out, hipStream_t stream);

// The lines of a finished batch ranked by a number they captured (gx_top.hip; the rule: gx_top.hpp): the n_wanted largest (or smallest)
// numbers' lines, ordered by (value, input line).
struct TopArgs {
    const void* data;            // the batch's code units
    int wide;                    // 1: UTF-16 code units
    const int32_t* caps;         // ROWS_DENSE: [n][slots]; compact rows carry their offsets themselves
    uint32_t slots;              // 2 * max_groups
    const void* image;           // TopHead, on the device, 16-byte aligned
    const void* where_image;     // WhereHead + the literals, or nullptr: no terms
    uint32_t where_image_bytes;  // a multiple of 16; 0: no terms
    uint32_t smallest;           // GX_TOP_SMALLEST
    uint32_t n_wanted;           // <= TOP_MAX_LINES
    uint32_t formats;            // a value group's or a term's group has a number format other than LONG
};
// The passes' device workspace, cut out of one allocation of top_workspace_bytes(n) bytes:
struct TopWs {
    uint8_t* head;                // TopDev (gx_top.hpp): the class counts, the select's state, a digit's histogram
    uint32_t* slab;               // the workgroups' counts, then their histograms
    uint64_t* block_sums;         // the scans'
    uint64_t* keys;               // [n] a candidate's key
    uint64_t* col;                // [n] 1: a candidate above the threshold, 2^32: one equal to it
    uint64_t* before;             // [n + 1] col scanned: both kinds before line i; [n]: all of them
    uint64_t* ckeys;              // [TOP_MAX_LINES] the chosen candidates in line order: keys ...
    int64_t* values;              // [TOP_MAX_LINES] the delivered lines' numbers, in rank order
    uint64_t* dst_off;            // [n_wanted + 1] code units before output line j
    uint32_t* clines;             // ... and lines
    uint32_t* perm;               // [TOP_MAX_LINES] the input line of output line j
    uint32_t* plen;               // [n_wanted] its code units, 0 from n_top on
    uint8_t* cand;                // [n] the line's value is a number
    size_t bytes;
};
TopWs top_workspace(void* ws, uint64_t n);
size_t top_workspace_bytes(uint64_t n);
// n > 0, parts > 0.  Everything before the emit; behind the host's look at the head, w.before[n] and w.dst_off[n_wanted] the emit is
// launch_partition_copy with w.perm and w.dst_off.
hipError_t launch_top_select(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const TopArgs& a,
                             const TopWs& w, hipStream_t stream);
// The keys pass of launch_top_select alone and the sum of its class counts, for the calls that share it (gx_quantile.hip): n > 0,
// parts > 0.  Of w it uses keys, cand and slab (top_keys_blocks(n) * TOP_COUNTS words); counts[TOP_COUNTS] lies on the device.
uint32_t top_keys_blocks(uint64_t n);
hipError_t launch_top_keys(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const TopArgs& a,
                           const TopWs& w, uint32_t* counts, hipStream_t stream);

// The percentiles of a number the lines of a finished batch captured (gx_quantile.hip; the rule: gx_quantile.hpp).  The lines that
// count, their class and the key are gx_top_lines': TopArgs with smallest = 0 (n_wanted is not looked at), whose image holds a
// QuantHead between the TopHead and the terms.
struct QuantWs {
    uint8_t* head;                // QuantDev (gx_quantile.hpp): the class counts, the result rows, the selects' state
    uint32_t* slab;               // the workgroups' counts, then their histograms: [workgroup][group][256]
    uint64_t* block_sums;         // the scan's
    uint64_t* keys;               // [n] a candidate's key
    uint64_t* before;             // [n + 1] cand scanned: the candidates before line i
    uint64_t* ckeys;              // [n] the candidates' keys, dense, in line order
    uint8_t* cand;                // [n] the line's value is a number
    size_t bytes;
};
QuantWs quant_workspace(void* ws, uint64_t n);
size_t quant_workspace_bytes(uint64_t n);
// n > 0, parts > 0.  Every pass; behind it the head's counts and rows are final.  quant_head: the QuantHead inside the image.
hipError_t launch_quantiles(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const TopArgs& a,
                            const void* quant_head, uint32_t n_quantiles, const QuantWs& w, hipStream_t stream);

// The percentiles of a captured number per captured text (gx_group_quantile.hip; the rule: gx_group_quantile.hpp), behind
// gx_group_lines' passes on the same stream.  The value's class and key are gx_top_lines': TopArgs whose image is a TopHead of the
// parts that have a value group (smallest = 0; n_wanted is not looked at).
struct GqPlan;
struct GqWs {
    uint8_t* head;                // GqDev (gx_group_quantile.hpp): class counts, the value keys' OR and AND, the candidates
    uint64_t* masks;              // the compaction's workgroups' OR and AND
    uint32_t* slab;               // the keys pass's counts, then a digit's counts, bin-major
    uint64_t* bases;              // the digit's counts scanned
    uint64_t* block_sums;         // the scans'
    uint64_t* keys;               // [n] a line's value key
    uint64_t* before;             // [n + 1] the candidates before line i
    uint64_t* vkey[2];            // [n] the pairs' value keys, ping and pong (vkey[1] is keys)
    uint32_t* knum[2];            // [n] the pairs' key numbers, ping and pong (knum[1]: the slots, until they are numbered)
    uint8_t* cand;                // [n] the line is a candidate
    size_t bytes;
};
GqWs gq_workspace(void* ws, uint64_t n);
size_t gq_workspace_bytes(uint64_t n);
bool gq_sorts_all_digits();       // the build sorts every value digit (-DGX_GQ_ALL_DIGITS)
// n > 0, parts > 0; slot_of: launch_group_build's.  Behind it the host reads GqDev at w.head.
hipError_t launch_gq_collect(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const TopArgs& a,
                             const uint32_t* slot_of, const GqWs& w, hipStream_t stream);
// Behind launch_group_emit (keynum).  0 < m <= n candidates; rows: n_keys x n_q QuantOut on the device; quant_head: a QuantHead there.
hipError_t launch_gq_sort_pick(const GqWs& w, uint64_t m, const GqPlan& plan, const uint32_t* keynum, uint32_t n_slots, const void* quant_head, uint32_t n_q,
                               uint64_t n_keys, void* rows, hipStream_t stream);

// The keys of a finished batch ranked by their lines or numbers (gx_top_groups.hip; the rule: gx_top_groups.hpp), behind
// launch_group_build on the same stream and the host's look at its totals.  The passes' device workspace, cut out of one allocation of
// top_groups_workspace_bytes(n, n_slots, n_keys) bytes; the columns are indexed by key number:
struct TopGroupsWs {
    uint8_t* head;                // TgDev (gx_top_groups.hpp): candidates, the keys' OR and AND, the select's state, a digit's histogram
    uint8_t* slab;                // the keys pass's workgroups' partial reductions (64-bit), then their histograms (32-bit)
    uint64_t* block_sums;         // the scans'
    uint64_t *key_hi, *key_lo;    // [n_keys] the key's 128-bit key
    uint64_t* col;                // [n_keys] 1: a candidate above the threshold, 2^32: one equal to it
    uint64_t* before;             // [n_keys + 1] col scanned: both kinds before key j; [n_keys]: all of them
    uint64_t *c_hi, *c_lo;        // [TG_MAX] the chosen candidates in key-number order: keys ...
    uint64_t* dst_off;            // [n_wanted + 1] key units before rank r
    uint32_t* first_of;           // [n_keys] the key's first line
    uint32_t* slot_of_key;        // [n_keys] the key's slot
    uint32_t* c_num;              // ... and key numbers
    uint32_t *r_num, *r_first, *r_slot;   // [TG_MAX] per rank: the key's number, first line and slot
    uint32_t* plen;               // [n_wanted] its key's units, 0 from n_top on
    uint8_t* cand;                // [n_keys] the key is a candidate
    size_t bytes;
};
// what the emit pass writes, each part optional (nullptr); all in rank order but line_rank
struct TopGroupsOut {
    void* key_units;
    void* key_offsets;
    uint32_t* key_number;
    uint32_t* key_first_line;
    uint64_t* key_lines;
    uint64_t* key_stats;          // [n_top][8]: gx_measure_stats' fields
    uint32_t* line_rank;          // [n]
    int offsets64;                // key_offsets: uint64, else uint32
};
bool top_groups_by_slots(uint64_t n, uint32_t n_slots);   // the keys pass reaches the keys through the slots, not the flagged first lines
TopGroupsWs top_groups_workspace(void* ws, uint64_t n, uint32_t n_slots, uint64_t n_keys);
size_t top_groups_workspace_bytes(uint64_t n, uint32_t n_slots, uint64_t n_keys);
// 0 < n_keys <= n, n_wanted <= TG_MAX.  Everything before the emit; behind it the host reads TgDev at w.head, w.before[n_keys] and
// w.dst_off[n_wanted] (n_wanted > 0).
hipError_t launch_top_groups_select(uint64_t n, const GroupArgs& a, const GroupWs& g, uint64_t n_keys, uint32_t rank_by, uint32_t smallest, uint32_t n_wanted,
                                    const TopGroupsWs& w, hipStream_t stream);
hipError_t launch_top_groups_emit(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const GroupArgs& a,
                                  const GroupWs& g, const TopGroupsWs& w, const TopGroupsOut& out, uint32_t n_top, uint64_t units_top,
                                  hipStream_t stream);

// Every key's lines together (gx_by_key.hip; the rule: gx_by_key.hpp), behind gx_group_lines' passes on the same stream.  The passes'
// device workspace, cut out of one allocation of by_key_workspace_bytes(n) bytes:
struct ByKeyWs {
    uint8_t* head;                // ByKeyDev (gx_by_key.hpp): the kept lines, their units, the kept keys
    uint64_t* sums;               // the kept pass's workgroups' units and keys
    uint32_t* slab;               // a digit's counts, bin-major
    uint64_t* bases;              // ... scanned
    uint64_t* block_sums;         // the scans'
    uint64_t* before;             // [n + 1] the kept lines before line i; [n]: all of them
    uint64_t* dst_off;            // [m + 1] code units before output line j (the same memory as `before`, behind the compaction)
    uint32_t* knum[2];            // [n] the entries' key numbers, ping and pong
    uint32_t* line[2];            // [n] their line numbers, likewise
    uint32_t* len;                // [n] every line's code units
    uint32_t* plen;               // [m] the same in output order
    uint8_t* kept;                // [n] the line is kept
    size_t bytes;
};
ByKeyWs by_key_workspace(void* ws, uint64_t n);
size_t by_key_workspace_bytes(uint64_t n);
// n > 0; g: launch_group_build's, behind it.  Behind this the host reads ByKeyDev at w.head.
hipError_t launch_by_key_kept(uint64_t n, const void* offsets, int offsets64, const GroupWs& g, uint64_t min_lines, uint64_t max_lines, const ByKeyWs& w,
                              hipStream_t stream);
// Behind launch_group_emit (g.keynum).  0 < m <= n kept lines; key_out_lines / key_out_units: n_keys + 1 each on the device, optional.
// Behind it the copy is launch_partition_copy with *perm and w.dst_off.
hipError_t launch_by_key_sort(uint64_t n, uint64_t m, uint64_t n_keys, uint32_t n_passes, const GroupWs& g, const ByKeyWs& w, uint64_t* key_out_lines,
                              uint64_t* key_out_units, uint32_t** perm, hipStream_t stream);

// A whole batch ordered by a number its lines captured (gx_sort.hip; the rule: gx_sort.hpp).  The lines that count, their class and the
// key are gx_top_lines': TopArgs (n_wanted is not looked at).  The passes' device workspace, cut out of one allocation of
// sort_workspace_bytes(n) bytes:
struct SortPlan;
struct SortWs {
    uint8_t* head;                // SortDev (gx_sort.hpp): the class counts, the entries' OR / AND / min / max, the totals
    uint64_t* sums;               // the entries pass's workgroups' words
    uint32_t* slab;               // the keys pass's counts, then a digit's counts, bin-major
    uint64_t* bases;              // ... scanned
    uint64_t* block_sums;         // the scans'
    uint64_t* keys;               // [n] a stamped line's key
    uint64_t* ckeys;              // [n] the stamped keys, dense, in line order
    uint64_t* word[2];            // [n] the pairs' keys, ping and pong (word[1] is keys)
    uint64_t* before;             // [n + 1] the stamped lines before line i; [n]: all of them
    uint64_t* dst_off;            // [lines_out + 1] code units before output line j (the same memory as `before`, behind the entries pass)
    uint32_t* line[2];            // [n] the pairs' line numbers, likewise; the rest lines behind the entries in both
    uint32_t* len;                // [n] every line's code units
    uint32_t* plen;               // [lines_out] the same in output order
    uint8_t* cand;                // [n] the line is stamped
    uint8_t* cls;                 // [n] SORT_STAMPED / SORT_CARRIED / SORT_REST
    size_t bytes;
};
SortWs sort_workspace(void* ws, uint64_t n);
size_t sort_workspace_bytes(uint64_t n);
// 0 < n <= 2^30; a == nullptr: no parts, every line is a rest line; flags: GX_SORT_*.  Behind it the host reads SortDev at w.head.
hipError_t launch_sort_entries(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const TopArgs* a,
                               uint32_t flags, const SortWs& w, hipStream_t stream);
// Behind the host's read: m entries, 0 < lines_out <= n lines that leave; out_values / out_class: lines_out each on the device, optional.
// Behind it the copy is launch_partition_copy with *perm and w.dst_off.
hipError_t launch_sort_emit(uint64_t n, uint64_t m, uint64_t lines_out, const SortPlan& plan, uint32_t flags, const SortWs& w, int64_t* out_values,
                            uint8_t* out_class, uint32_t** perm, hipStream_t stream);

// A key's lines ordered by a captured time and cut into sessions (gx_sessions.hip; the rule: gx_sessions.hpp), behind launch_group_build
// on the same stream (g.slot_of, g.head_words, g.idx_off: a key's number is idx_off[its first line]); launch_group_emit is not needed.
// The passes' device workspace: per line, cut out of one allocation of sessions_workspace_bytes(n, values) bytes --
struct SessionsWs {
    uint8_t* image;               // SessionsHead (gx_sessions.hpp), put there by the caller, 16-byte aligned
    uint8_t* dev;                 // SessionsDev: the classes of the keyed lines, the time words' OR / AND / minimum / maximum
    uint64_t* tword;              // [n] an entry's time word: top_key(time, false)
    uint64_t* before;             // [n + 1] the entries before line i; [n]: all of them
    uint64_t* sums;               // the scan's
    int64_t* val;                 // [n] an entry's value, with a value group (else nullptr)
    uint8_t* ent;                 // [n] the line is an entry
    uint8_t* vcls;                // [n] an entry's value's class -- 0: a number, 1: unset, 2: no number, 3: none to measure; nullptr as val
    size_t bytes;
};
// -- and per entry, sized by the m entries the host has read: sessions_sort_workspace_bytes(m, stats) bytes.
struct SessionsSortWs {
    uint8_t* dev2;                // SessionsDev2: the sessions, the longest
    BucketSortWs by_time;         // (time word, line) pairs; behind the sort its other buffer holds times and lines in the final order
    BucketSortWs by_key;          // (key number, place in time order) pairs
    uint64_t* sbefore;            // [m + 1] the heads before entry e; [m]: the sessions
    uint64_t* sums;               // the scans'
    uint32_t* start;              // [m + 1] the first entry of session s; [n_sessions] = m
    uint32_t* skey;               // [m] the sessions' key numbers
    uint8_t* head;                // [m] entry e begins a session
    uint64_t* col[4];             // with stats: [m] numbers | unset << 32, not_numbers, the sum's low and high halves ...
    uint64_t* pre[4];             // ... and [m + 1] their scans
    uint64_t *smin, *smax;        // [m] per session: group_min_word / group_max_word merged by maximum
    size_t bytes;
};
// what the emit passes write, each part optional (nullptr)
struct SessionsOut {
    uint32_t* session_key;
    int64_t* session_begin;
    int64_t* session_end;
    uint32_t* session_first_line;
    uint64_t* session_lines;
    uint64_t* session_stats;      // [n_sessions][8]: gx_measure_stats' fields
    uint64_t* session_entry_begin;   // [n_sessions + 1]
    uint64_t* key_session_begin;  // [n_keys + 1]
    uint32_t* entry_line;         // [m]
    uint32_t* line_session;       // [n]
};
SessionsWs sessions_workspace(void* ws, uint64_t n, bool values);
size_t sessions_workspace_bytes(uint64_t n, bool values);
SessionsSortWs sessions_sort_workspace(void* ws, uint64_t m, bool stats);
size_t sessions_sort_workspace_bytes(uint64_t m, bool stats);
// n > 0, parts > 0; formats: a value group's or a number group's format is not LONG.  Behind it the host reads SessionsDev at w.dev.
hipError_t launch_sessions_keys(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const GroupArgs& a,
                                bool formats, const GroupWs& g, const SessionsWs& w, hipStream_t stream);
// 0 < m <= 2^30 entries; plan: sessions_time_plan's; key_digits: sessions_key_digits'.  Behind it the host reads SessionsDev2 at s.dev2.
hipError_t launch_sessions_sort(uint64_t n, uint64_t m, const SortPlan& plan, uint32_t key_digits, int64_t max_gap, const GroupWs& g, const SessionsWs& w,
                                const SessionsSortWs& s, uint32_t* time_buf, uint32_t* key_buf, hipStream_t stream);
// 0 < ns <= m sessions, each output within its capacity (the host has checked it); time_buf / key_buf: launch_sessions_sort's.
hipError_t launch_sessions_emit(uint64_t n, uint64_t m, uint64_t ns, uint64_t n_keys, const SessionsWs& w, const SessionsSortWs& s, uint32_t time_buf, uint32_t key_buf,
                                const SessionsOut& out, hipStream_t stream);
// The two halves of the above that gx_group_windows shares.  The ORDER: compact, time sort, key numbers, key sort and the gather; leaves
// key numbers in by_key.word[*key_buf], times and lines in by_time.word[*time_buf] / .slot[*time_buf], and with head (nullptr: not
// wanted) head[e] under max_gap.
hipError_t launch_sessions_order(uint64_t n, uint64_t m, const SortPlan& plan, uint32_t key_digits, const GroupWs& g, const SessionsWs& w, const BucketSortWs& by_time,
                                 const BucketSortWs& by_key, int64_t max_gap, uint8_t* head, uint32_t* time_buf, uint32_t* key_buf, hipStream_t stream);
// The entries' values as four columns and their scans (col / pre as in SessionsSortWs); with head also the sessions' minima and maxima.
hipError_t launch_sessions_value_prefix(const uint32_t* eline, const uint8_t* head, const uint64_t* sbefore, uint64_t m, uint64_t n, const SessionsWs& w,
                                        uint64_t* const* col, uint64_t* const* pre, uint64_t* sums, uint64_t* smin, uint64_t* smax, hipStream_t stream);

// Trailing time windows per key (gx_windows.hip; the rule: gx_windows.hpp): the lines of a key within `window` before each of its
// entries, behind launch_sessions_keys (SessionsWs is shared as it is) and the host's read of SessionsDev.  The passes' device workspace
// per entry and key, sized by the m entries and n_keys keys the host has read: windows_workspace_bytes(m, n_keys, sums) bytes.
struct WindowsWs {
    uint8_t* dev2;                // WindowsDev2: the trips, the tripped keys, the peak
    BucketSortWs by_time;         // (time word, line) pairs; behind the sort its other buffer holds times and lines in the final order
    BucketSortWs by_key;          // (key number, place in time order) pairs
    uint64_t* tbefore;            // [m + 1] the trips before entry e; [m]: the trips
    uint64_t* sums;               // the scans'
    uint64_t* kpeak;              // [n_keys] window_peak_word merged by maximum; 0: the key has no entry
    uint32_t* wl;                 // [m] window_lines(e)
    uint32_t* ekey;               // [m] the entries' key numbers
    uint32_t* tent;               // [m] the entry of trip t
    uint32_t* tkey;               // [m] the key number of trip t
    uint8_t* flag;                // [m] entry e trips
    uint64_t* col[4];             // with sums: [m] numbers | unset << 32, not_numbers, the sum's low and high halves ...
    uint64_t* pre[4];             // ... and [m + 1] their scans
    size_t bytes;
};
// what the emit passes write, each part optional (nullptr)
struct WindowsOut {
    uint32_t* entry_line;         // [m]
    uint32_t* entry_key;
    int64_t* entry_time;
    uint32_t* entry_window_lines;
    uint64_t* entry_window_sum;   // [m][4]: gx_window_sum's fields
    uint64_t* key_entry_begin;    // [n_keys + 1]
    uint32_t* key_peak_lines;     // [n_keys]
    uint32_t* key_peak_line;      // [n_keys]
    uint32_t* line_window_lines;  // [n]
    uint32_t* trip_key;           // [n_trips]
    uint32_t* trip_line;
    int64_t* trip_time;
    uint32_t* trip_entry;
    uint64_t* key_trip_begin;     // [n_keys + 1]
};
WindowsWs windows_workspace(void* ws, uint64_t m, uint64_t n_keys, bool sums);
size_t windows_workspace_bytes(uint64_t m, uint64_t n_keys, bool sums);
// 0 < m <= 2^30 entries of 0 < n_keys keys; plan: sessions_time_plan's; key_digits: sessions_key_digits'; window >= 0.  Behind it the host
// reads WindowsDev2 at s.dev2.
hipError_t launch_windows_pass(uint64_t n, uint64_t m, uint64_t n_keys, const SortPlan& plan, uint32_t key_digits, int64_t window, uint32_t threshold,
                               const GroupWs& g, const SessionsWs& w, const WindowsWs& s, uint32_t* time_buf, uint32_t* key_buf, hipStream_t stream);
// nt trips, each output within its capacity (the host has checked it); time_buf / key_buf: launch_windows_pass'.  out.entry_window_sum
// needs a workspace made with sums and w.val / w.vcls.
hipError_t launch_windows_emit(uint64_t n, uint64_t m, uint64_t nt, uint64_t n_keys, const SessionsWs& w, const WindowsWs& s, uint32_t time_buf, uint32_t key_buf,
                               const WindowsOut& out, hipStream_t stream);

// A key's BEGIN and END lines paired in input order (gx_spans.hip; the rule: gx_spans.hpp), behind launch_group_build on the same stream
// (g.slot_of, g.head_words, g.idx_off: a key's number is idx_off[its first line]); launch_group_emit is not needed.  The passes' device
// workspace: per line, cut out of one allocation of spans_workspace_bytes(n) bytes --
struct SpansWs {
    uint8_t* image;               // SpansHead (gx_spans.hpp), put there by the caller, 16-byte aligned
    int64_t* tval;                // [n] an entry's time where its class is "number", else 0
    uint64_t* before;             // [n + 1] the entries before line i; [n]: all of them
    uint64_t* sums;               // the scan's
    uint8_t* ent;                 // [n] the line is an entry (it is keyed)
    uint8_t* tcr;                 // [n] an entry's time's class and its role (span_pack)
    size_t bytes;
};
// -- and per entry and key, sized by the m entries and n_keys keys the host has read: spans_pair_workspace_bytes(m, n_keys) bytes.
struct SpansPairWs {
    uint8_t* dev;                 // SpansDev: the states' counts, the durations' minimum and maximum
    BucketSortWs sort;            // (key number, line) pairs
    uint64_t* sbefore;            // [m + 1] the span ends before entry e; [m]: the spans
    uint64_t* sums;               // the scans'
    uint64_t* col[4];             // [m] of a span's end: numbers | unset << 32, not_numbers | out_of_range << 32, the sum's low and high halves ...
    uint64_t* pre[4];             // ... and [m + 1] their scans
    uint64_t *kmin, *kmax;        // [n_keys] per key: group_min_word / group_max_word of its durations merged by maximum
    uint8_t* state;               // [m] span_state of entry e
    uint8_t* flag;                // [m] entry e ends a span
    size_t bytes;
};
// what the emit passes write, each part optional (nullptr)
struct SpansOut {
    uint32_t* span_key;
    uint32_t* span_begin_line;
    uint32_t* span_end_line;
    int64_t* span_begin;
    int64_t* span_end;
    int64_t* span_duration;
    uint8_t* span_class;
    uint64_t* key_span_begin;     // [n_keys + 1]
    uint64_t* key_span_stats;     // [n_keys][8]: gx_measure_stats' fields
    uint32_t* key_open_line;      // [n_keys]
    uint32_t* line_span;          // [n]
    uint8_t* line_state;          // [n]
};
SpansWs spans_workspace(void* ws, uint64_t n);
size_t spans_workspace_bytes(uint64_t n);
SpansPairWs spans_pair_workspace(void* ws, uint64_t m, uint64_t n_keys);
size_t spans_pair_workspace_bytes(uint64_t m, uint64_t n_keys);
// n > 0, parts > 0; formats: a number group's format is not LONG.  Behind it the host reads the entries at w.before[n].
hipError_t launch_spans_entries(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const GroupArgs& a,
                                bool formats, const GroupWs& g, const SpansWs& w, hipStream_t stream);
// 0 < m <= 2^30 entries of 0 < n_keys keys; key_digits: spans_key_digits'.  Behind it the host reads SpansDev at s.dev, s.sbefore[m] and
// s.pre[q][m].
hipError_t launch_spans_pair(uint64_t n, uint64_t m, uint64_t n_keys, uint32_t key_digits, const GroupWs& g, const SpansWs& w, const SpansPairWs& s, uint32_t* buf,
                             hipStream_t stream);
// ns spans, each output within its capacity (the host has checked it); buf: launch_spans_pair's.
hipError_t launch_spans_emit(uint64_t n, uint64_t m, uint64_t ns, uint64_t n_keys, const SpansWs& w, const SpansPairWs& s, uint32_t buf, const SpansOut& out,
                             hipStream_t stream);

// The partition of a finished batch by outcome (gx_partition.hip): the kept lines ordered by (outcome index, input line number).
// The passes' device workspace, cut out of one allocation of partition_workspace_bytes(n, K) bytes:
struct PartWs {
    uint64_t* groups;             // [2K + 3] output lines before group x, then [2K + 3] the same in code units; [2K + 2]: the totals
    uint32_t* status;             // behind them; != 0: a line of 4 G code units or more
    uint8_t* want;                // [2K + 1] the mask, put there by the caller of launch_partition_sort
    uint64_t* block_sums;         // the scans'
    uint32_t* slab;               // [64][workgroups] a digit's counts
    uint64_t* bases;              // ... scanned
    uint64_t* dst_off;            // [n + 1] code units before output line j
    uint32_t* keys[2];            // [n] the keys, before and behind a digit's scatter
    uint32_t* perm[2];            // [n] the line numbers, likewise
    uint32_t* klen;               // [n] the line's code units when it is kept, else 0
    uint32_t* plen;               // [n] the same in output order
    uint32_t* perm_sorted;        // perm[0] or perm[1]: the input line of output line j, left by launch_partition_sort
    size_t bytes;
};
PartWs partition_workspace(void* ws, uint64_t n, uint32_t K);
size_t partition_workspace_bytes(uint64_t n, uint32_t K);
uint32_t partition_digits(uint32_t K);   // six-bit digits of the keys 0 .. 2K + 1
// ids, offsets: as launch_select_flags takes them; w.want holds the mask
hipError_t launch_partition_sort(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, PartWs& w,
                                 hipStream_t stream);
// kept: w.groups[2K + 2] as the host has read it
hipError_t launch_partition_copy(const SelectOut& o, const void* data, const void* offsets, int offsets64, int wide, uint64_t n, uint64_t kept, const PartWs& w,
                                 hipStream_t stream);
hipError_t launch_partition_pick(const uint64_t* from, const uint64_t* at, uint32_t count, uint64_t* out, hipStream_t stream);   // out[i] = from[at[i]]

// UTF-8 lines as UTF-16 code units (gx_utf8.hip; the rule: gx_utf8.hpp).  The passes' device workspace, cut out of one allocation of
// utf8_workspace_bytes(n) bytes:
struct Utf8Ws {
    uint64_t* unit_off;             // [n + 1] units before line i; [n]: all of them
    uint64_t* block_sums;           // the scan's
    unsigned long long* flagged;    // the lines that were counted (flagged ones, or all)
    uint32_t* status;               // != 0: a line of 4 G units or more
    uint32_t* counts;               // [n] the line's units, 0 for a line that is not flagged
    uint8_t* flags;                 // [n] for the flag sweep, when the caller brings none
    uint64_t* list;                 // [n] the flagged lines' numbers, *flagged of them, in the order the waves met them
};
size_t utf8_workspace_bytes(uint64_t n);
Utf8Ws utf8_workspace(void* ws, uint64_t n);
// flags[i] = 1 for every line that holds a byte >= 0x80, else 0 (what launch_split_lines' flags say)
hipError_t launch_utf8_flags(const uint8_t* data, const void* offsets, int offsets64, uint64_t n, uint8_t* flags, hipStream_t stream);
// flags == nullptr: every line.  Leaves w.unit_off (n = 0 too), *w.flagged and *w.status, and with flags w.list.
hipError_t launch_utf8_count(const uint8_t* data, const void* offsets, int offsets64, uint64_t n, const uint8_t* flags, const Utf8Ws& w, hipStream_t stream);
// unit_byte (optional, one u32 per unit): the byte, from the line's first, of the item the unit starts in
hipError_t launch_utf8_write(const uint8_t* data, const void* offsets, int offsets64, uint64_t n, const uint8_t* flags, const uint64_t* unit_off, uint16_t* units,
                             uint32_t* unit_byte, hipStream_t stream);
hipError_t launch_utf8_offsets32(const uint64_t* unit_off, uint64_t n, uint32_t* out, hipStream_t stream);   // out[0 .. n]
// b: the BYTE batch and its result rows; the rows of flagged lines go from unit offsets to byte offsets (clipped ones += *b.overflow)
hipError_t launch_utf8_offsets_to_bytes(const GxDev& dev, const GxBatch& b, const uint8_t* flags, const uint64_t* unit_off, const uint32_t* unit_byte,
                                        hipStream_t stream);

}  // namespace gx
