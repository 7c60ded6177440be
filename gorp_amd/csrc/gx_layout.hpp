// gx_layout.hpp -- the LDS layout of the batch kernels' table images, and the sizes it is planned with.  No HIP: the host code
// that builds the images and plans the layouts (gx_images.cpp) is plain C++; the kernels read the same struct (gx_device.hpp).
#pragma once
#include <cstdint>

namespace gx {

constexpr uint32_t LDS_BYTES = 163840;          // 160 KiB per CU on gfx950
constexpr uint32_t LDS_TABLE_BUDGET = 96 * 1024;

// Layout of the LDS-resident table image used by the tile kernel: byte offsets
// from the start of dynamic LDS.  The image [0, table_bytes) is built on the
// host, kept in HBM next to the other tables and copied into LDS by every
// workgroup's prologue.
struct GxLds {
    uint32_t cmap;        // u16[272] byte -> class * 4 (the byte offset of the class's column in a row), entry 256 = the
                          // identity column; always at offset 0 (the kernel indexes LDS by 2 * byte value)
    uint32_t ncls;        // number of classes = index of the identity column
    uint32_t at;          // automaton rows, u32[rows][ncls + 3]: one row per state of the match automaton and of
                          // the fused automaton (or of every extraction's capture automaton).  Columns
                          // 0..ncls-1: successor | capture program << 16, where the successor is the LDS byte
                          // address of its row (LDS tier; always < 65536) or its state index (L2 tier); column
                          // ncls: identity (self, no program); column ncls+1: self-loop byte interval as
                          // lo | (0x7F - hi) << 8 (0x8000: none), bit 16 set when the state also loops on every byte
                          // of the hot interval (hot_lo4 / hot_k4 below); column ncls+2: info (match automaton: first
                          // accepting extraction or -1; capture automaton: byte offset of the state's final
                          // record, or -1 / -2-k)
    uint32_t row_bytes;   // (ncls + 3) * 4
    uint32_t c_base;      // L2 tier: byte offset of the capture rows inside the global row image (0 in the LDS tier)
    uint32_t m_start;     // row (LDS address / state index) of the match automaton's start state
    uint32_t m_dead;      // row of its absorbing dead state
    uint32_t c_rule;      // u32[n_rules * 2]: row of the rule's start state, group count
    uint32_t u_start;     // row of the fused automaton's start state, or 0xFFFFFFFF when absent
    uint32_t u_dead;      // row of its dead state
    uint32_t ops_off;     // u32[n_oplists + 1]
    uint32_t ops;         // u16 pairs
    uint32_t fin_tags;    // final records (gx_rows.hpp: line_result): LDS address, or byte offset in the global row image (L2 tier)
    uint32_t table_bytes; // size of the image, multiple of 16
    uint32_t simple_ops;  // 1: every capture program is one "register := position"; the program field is then
                          // (register + 1) * 128 = byte offset of the register's column in the wave's register
                          // block (0 = the dummy column = no program) and steps are branch-free;
                          // 0: program field 0 = none, 0x8000 | register = single set, else op-list index
    uint32_t regs;        // u16[nwaves][1 + max_regs][64]; column 0 is a write-only dummy
    uint32_t regs_wave_bytes;
    uint32_t bitmap;      // tile kernel: u64[nwaves][18], bit c of a wave's map = "all 16 bytes of staged chunk c lie in
                          // the hot interval" (written when the tile is staged, read by the walk to jump over runs)
    uint32_t counter;     // tile kernel: u32, the workgroup's next tile (gx_tile.hip)
    uint32_t stage;       // u8[nwaves][stage_bytes]
    uint32_t stage_bytes; // multiple of 16
    uint32_t nwaves;
    uint32_t total_bytes; // dynamic LDS size to launch with
    // Hot interval: the widest self-loop byte interval of the automata (typically \S+ or .*), in the form the SWAR
    // range test consumes (lo and 0x7F - hi in every byte; hot_k4 = 0x80808080: none, no chunk ever qualifies).
    uint32_t hot_lo4, hot_k4;
    // Record tier (tier == 2; gx_images.cpp: records_from_dense): states are 8-byte range records at LDS address rec,
    // a state is the index of its first record, cmap holds class ids (renumbered), acc_tab[first class of the self
    // range] is the state's self-loop interval word.
    uint32_t tier;        // 0: dense rows in LDS, 1: dense rows in global memory, 2: records in LDS
    uint32_t rec, acc_tab;
    uint32_t rec_indexed; // states with an index >= this keep one record per class (state index + class), behind all the others
    uint32_t sort_lds;    // lane kernel, length-sorted mode: LDS address of u16 perm[sort_chunk] + u32 hist[64] + u32 cursor[64]
    uint32_t sort_chunk;  // ... lines per chunk (0: tiles in input order)
    uint32_t hop_sets;    // hop tier: LDS address of the loop sets (gx_hop.cpp: u8 lo[4], u8 k[4] per entry, entry 0 = none)
    uint32_t fin_unset;   // hop tier: the final records' tags name columns, as byte offsets from a wave's dummy column (tag 0: the
                          // dummy column, which takes the line's length); this tag names a column that does not exist: unset
    uint32_t fin_state_off, fin_state_rec;   // hop tier: the final records by state in the global image (byte offset, 0: none; bytes per record)
};
constexpr uint32_t GX_STEAL_MAX = 3072;         // workgroups of a tile-kernel launch at most (256 CUs x 12)
constexpr uint32_t GX_STEAL_STRIDE = 32;        // u32 words between two workgroups' counters: a cache line each (atomics on ONE line
                                                // take their turns at 11 ns apiece, whichever words of it they want)
constexpr uint32_t GX_BITMAP_WAVE_BYTES = 144;  // 16 x u64 (1024 chunks = 16 KB of staging) + one word read ahead

// Hop slice kernel's piece of a line (gx_device.hpp: launch_extract_hop_slices)
#ifndef GX_HOP_SLICE_BYTES
#define GX_HOP_SLICE_BYTES 128u   // (a power of two times 16, at most 1024: one piece is loaded by 64 / (bytes / 16) ... lanes per line)
#endif
constexpr uint32_t GX_SERVICE_MAX_BYTES = 56u + 16u * 60u;   // the longest line a request of the resident service holds (1 016 bytes)

// The three formats a batch's results leave a kernel in (gx_batch_opts.compact_results, include/gorp_hip.h).  A line's result is its
// match id and slots = 2 * max_groups offsets (begin, end per group; -1: no match / unset):
//   ROWS_DENSE  int32 match_id[n] and int32 caps[n][slots];
//   ROWS_U16    u16[1 + slots] per line: int16 id, offsets with 0xFFFF = unset, an offset above 65 534 stored as 65 534 and counted;
//   ROWS_U8     u8[1 + slots] per line: int8 id, offsets with 0xFF = unset, an offset above 254 stored as 254 and counted.
// Everything about a format is here, once: kernels (gx_rows.hpp), host code and tests use these functions.
enum RowFormat : uint32_t { ROWS_DENSE = 0, ROWS_U16 = 1, ROWS_U8 = 2 };
constexpr RowFormat row_format(bool compact, bool narrow) { return !compact ? ROWS_DENSE : narrow ? ROWS_U8 : ROWS_U16; }
constexpr uint32_t row_unit_bytes(RowFormat f) { return f == ROWS_U8 ? 1u : f == ROWS_U16 ? 2u : 4u; }
constexpr uint32_t row_bytes(RowFormat f, uint32_t slots) { return row_unit_bytes(f) + row_unit_bytes(f) * slots; }   // (dense: id + caps of a line)
constexpr uint32_t row_unset(RowFormat f) { return f == ROWS_U8 ? 0xFFu : f == ROWS_U16 ? 0xFFFFu : 0xFFFFFFFFu; }   // also the unit mask
constexpr int32_t row_max_offset(RowFormat f) { return f == ROWS_U8 ? 254 : f == ROWS_U16 ? 65534 : 0x7FFFFFFF; }
struct RowUnit { uint32_t unit, clipped; };   // an offset as stored, and 1 when it was above row_max_offset (stored as that)
constexpr RowUnit encode_offset(RowFormat f, int32_t v) {
    return v < 0 ? RowUnit{row_unset(f), 0u}
                 : v > row_max_offset(f) ? RowUnit{static_cast<uint32_t>(row_max_offset(f)), 1u} : RowUnit{static_cast<uint32_t>(v), 0u};
}
constexpr int32_t decode_offset(RowFormat f, uint32_t unit) { return unit == row_unset(f) ? -1 : static_cast<int32_t>(unit); }
constexpr uint32_t encode_id(RowFormat f, int32_t id) { return static_cast<uint32_t>(id) & row_unset(f); }   // (at most 32 767 / 127 extractions)
constexpr int32_t decode_id(RowFormat f, uint32_t unit) {
    return f == ROWS_U8 ? static_cast<int8_t>(unit) : f == ROWS_U16 ? static_cast<int16_t>(unit) : static_cast<int32_t>(unit);
}

}  // namespace gx
