// gx_rows.hpp -- where a line's result leaves a batch kernel.  What a row holds (the formats, the unset values, the largest
// storable offset, encode / decode) is gx_layout.hpp's; this header turns the final record of the state a line's walk ended in
// into rows of those formats:
//   line_result   the line's groups, block by block of four (resolve_tags: the tag rule), handed to an emit callback;
//   RowOut        where a batch's results go; id() / cap() store one element (the per-line kernels);
//   store_row     a lane's whole row in as few stores as the format allows (the slice kernels);
//   store_tile    a tile's 64 rows through the wave's LDS area, then out as 16-byte stores (the tile and lane kernels).
// Clipping (an offset above row_max_offset stored as that and counted in *overflow) is one rule in three forms: per element in
// id() / cap(); in store_row and store_tile only when a lane writing a row at that point has a line longer than row_max_offset (a
// ballot over the active lanes: every offset is at most the line's length); and not at all where the kernel knows that no
// line is that long (store_tile's CLIP = false).
#pragma once
#include "gx_walk.hpp"

namespace gx {

struct RowOut {
    int32_t* match_id;              // ROWS_DENSE: [n]
    int32_t* caps;                  // ROWS_DENSE: [n][slots]
    uint8_t* rows;                  // ROWS_U16 / ROWS_U8: row_bytes(format, slots) bytes per line
    unsigned long long* overflow;   // compact rows: += the number of offsets stored clipped (null: not counted)
    RowFormat format;
    uint32_t slots;                 // 2 * max_groups

    __device__ __forceinline__ void id(uint64_t i, int32_t k) const {
        if (format == ROWS_U8) rows[i * row_bytes(ROWS_U8, slots)] = static_cast<uint8_t>(encode_id(ROWS_U8, k));
        else if (format == ROWS_U16) *reinterpret_cast<uint16_t*>(rows + i * row_bytes(ROWS_U16, slots)) = static_cast<uint16_t>(encode_id(ROWS_U16, k));
        else match_id[i] = k;
    }
    __device__ __forceinline__ void cap(uint64_t i, int t, int32_t v) const {
        if (format == ROWS_DENSE) { caps[i * static_cast<uint64_t>(slots) + t] = v; return; }
        const RowUnit u = encode_offset(format, v);
        if (u.clipped && overflow) atomicAdd(overflow, 1ull);
        uint8_t* p = rows + i * row_bytes(format, slots) + row_unit_bytes(format) * (1u + t);
        if (format == ROWS_U8) *p = static_cast<uint8_t>(u.unit);
        else *reinterpret_cast<uint16_t*>(p) = static_cast<uint16_t>(u.unit);
    }
};

inline RowOut row_out(const GxDev& dev, const GxBatch& b) {
    return RowOut{b.match_id, b.caps, reinterpret_cast<uint8_t*>(b.packed), b.overflow, row_format(b.packed != nullptr, b.narrow != 0),
                  2u * static_cast<uint32_t>(dev.max_groups)};
}

// Final records (gx_images.cpp: build_tile_image; gx_hop.cpp): u16 [begin tag, end tag] x max_groups, padded to a multiple of four
// groups, then the extraction id (int16).  A tag is 0 = unset, 1 = the line length, else the byte offset of a register column from the
// wave's dummy column.  TIER_HOP: every tag names a column -- a register's, "the length" or "unset" (hop_unset: its offset; the lane
// has filled both in) -- and a group with one end unset has both unset: two reads and one test per group, no selects on tag values.
// One block = the tags of four groups (a dword each): tag_columns reads the four groups' columns (two LDS round trips per block: all
// tags, then all registers), tag_offsets makes one group's offsets of them, -1 / -1 for an unset group.
template <int TIER>
__device__ __forceinline__ void tag_columns(const u32x4& t, uint32_t regs, uint32_t (&tw)[4], uint32_t (&vb)[4], uint32_t (&ve)[4]) {
    const uint32_t dummy_col = regs - 128u;
    tw[0] = t.x; tw[1] = t.y; tw[2] = t.z; tw[3] = t.w;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        vb[q] = lds_ld<uint16_t>(dummy_col + (tw[q] & (TIER == TIER_HOP ? 0xFFFFu : 0xFF80u)));
        ve[q] = lds_ld<uint16_t>(dummy_col + (TIER == TIER_HOP ? tw[q] >> 16 : (tw[q] >> 16) & 0xFF80u));
    }
}
template <int TIER>
__device__ __forceinline__ void tag_offsets(uint32_t tw, uint32_t vb, uint32_t ve, uint32_t len, uint32_t hop_unset, int32_t& pb, int32_t& pe) {
    const uint32_t tb = tw & 0xFFFFu, te = tw >> 16;
    if (TIER == TIER_HOP) {
        const bool unset = tb == hop_unset;
        pb = unset ? -1 : static_cast<int32_t>(vb);
        pe = unset ? -1 : static_cast<int32_t>(ve);
    } else {
        pb = tb == 1u ? static_cast<int32_t>(len) : static_cast<int32_t>(vb);
        pe = te == 1u ? static_cast<int32_t>(len) : static_cast<int32_t>(ve);
        if (tb == 0u || te == 0u) { pb = -1; pe = -1; }
    }
}
template <int TIER>
__device__ __forceinline__ void resolve_tags(const u32x4& t, uint32_t regs, uint32_t len, uint32_t hop_unset, int32_t (&pb)[4], int32_t (&pe)[4]) {
    uint32_t tw[4], vb[4], ve[4];
    tag_columns<TIER>(t, regs, tw, vb, ve);
#pragma unroll
    for (int q = 0; q < 4; ++q) tag_offsets<TIER>(tw[q], vb[q], ve[q], len, hop_unset, pb[q], pe[q]);
}

// The final record a line's info word names: info < 0 is -1 (null) or -2-k (ExtractionException) and takes record 0, which has
// every tag unset (gx_images.cpp, gx_hop.cpp), so the loads are unconditional.  In LDS, or in global memory (TIER_L2 / TIER_RECG;
// TIER_HOP when its records did not fit LDS: fin_g != nullptr, wave-uniform).
struct FinRec {
    uint32_t fin_lds;
    const uint8_t* fin_g;
    uint32_t rec;   // (byte offset of the record in either)
    bool global;
    __device__ __forceinline__ u32x4 tags(int g0) const {
        return global ? *reinterpret_cast<const u32x4*>(fin_g + rec + 4u * g0) : lds_ld<u32x4>(fin_lds + rec + 4u * g0);
    }
    __device__ __forceinline__ uint32_t id_of(int G) const {   // (the extraction id behind the tags)
        const uint32_t id_at = rec + 16u * static_cast<uint32_t>((G + 3) >> 2);
        return global ? *reinterpret_cast<const uint16_t*>(fin_g + id_at) : lds_ld<uint16_t>(fin_lds + id_at);
    }
};
template <int TIER>
__device__ __forceinline__ FinRec fin_rec(int32_t info, uint32_t fin_lds, const uint8_t* fin_g) {
    const bool global = TIER == TIER_L2 || TIER == TIER_RECG || (TIER == TIER_HOP && fin_g != nullptr);
    return FinRec{fin_lds, fin_g, info >= 0 ? static_cast<uint32_t>(info) : 0u, global};
}

// The final record OF THE STATE (hop slice kernel; gx_hop.cpp: fin_state_off): the same tags, and behind them the extraction's index,
// or -1 / -2-k for a state that accepts nothing (every tag unset).  A lane asks for the first twelve groups' tags and the index when
// its line is over, behind the walk (load); the row store then finds them here and the rest in global memory (at).
struct FinAhead {
    u32x4 t0 = {0u, 0u, 0u, 0u}, t1 = {0u, 0u, 0u, 0u}, t2 = {0u, 0u, 0u, 0u};
    uint32_t id = 0u;
    __device__ __forceinline__ void load(const uint8_t* __restrict__ recp, int G) {
        const int nblk = (G + 3) >> 2;
        t0 = *reinterpret_cast<const u32x4*>(recp);
        t1 = *reinterpret_cast<const u32x4*>(recp + (nblk > 1 ? 16 : 0));
        t2 = *reinterpret_cast<const u32x4*>(recp + (nblk > 2 ? 32 : 0));
        id = *reinterpret_cast<const uint16_t*>(recp + 16 * nblk);
    }
    struct At {
        u32x4 t0, t1, t2;
        uint32_t id;
        const uint8_t* recp;
        __device__ __forceinline__ u32x4 tags(int g0) const {
            if (g0 >= 12) return *reinterpret_cast<const u32x4*>(recp + 4 * g0);
            const u32x4 a = t0, b = t1, c = t2;   // (values, not members to pick from: picking an address puts them in scratch memory)
            return g0 == 0 ? a : g0 == 4 ? b : c;
        }
        __device__ __forceinline__ uint32_t id_of(int) const { return id; }
    };
    __device__ __forceinline__ At at(const uint8_t* recp) const { return At{t0, t1, t2, id, recp}; }
};

// The result of one line: emit(g, begin, end) for g = 0 .. G-1, (-1, -1) for an unset group; returns the match id.
// Two LDS round trips per four groups: all tags, then all registers, then the selects.
// (Round 5: the first twelve groups' tags, then all their registers, then the rows -- two trips for config 3's ten groups instead of six:
// 0.778 against 0.755 ms, one device; the 36 values it holds at once cost more than the trips.  Not kept.)
template <int TIER, typename EMIT>
__device__ __forceinline__ int32_t line_result(int32_t info, uint32_t fin_lds, const uint8_t* fin_g, uint32_t regs, uint32_t len, int G,
                                               EMIT emit, uint32_t hop_unset = 0u) {
    const uint32_t rec = info >= 0 ? static_cast<uint32_t>(info) : 0u;
    const uint32_t id_at = rec + 16u * static_cast<uint32_t>((G + 3) >> 2);
    uint32_t id;
    const bool FIN_GLOBAL = TIER == TIER_L2 || TIER == TIER_RECG || (TIER == TIER_HOP && fin_g != nullptr);
    if (FIN_GLOBAL) id = *reinterpret_cast<const uint16_t*>(fin_g + id_at);
    else id = lds_ld<uint16_t>(fin_lds + id_at);
    for (int g0 = 0; g0 < G; g0 += 4) {
        u32x4 t;
        if (FIN_GLOBAL) t = *reinterpret_cast<const u32x4*>(fin_g + rec + 4u * g0);
        else t = lds_ld<u32x4>(fin_lds + rec + 4u * g0);
        uint32_t tw[4], vb[4], ve[4];
        tag_columns<TIER>(t, regs, tw, vb, ve);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (g0 + q < G) {
                int32_t pb, pe;
                tag_offsets<TIER>(tw[q], vb[q], ve[q], len, hop_unset, pb, pe);
                emit(g0 + q, pb, pe);
            }
        }
    }
    return info >= 0 ? static_cast<int32_t>(static_cast<int16_t>(id)) : info;
}

// A line's whole row from its lane (the slice kernels: a lane holds a line of its own, its row goes where no neighbour's does --
// 1 + 2 G scattered stores of two bytes each were a sixth of the hop slice kernel on BASELINE configs[4]).  Four groups at a time,
// as the final records hold their tags: dense results leave as two 16-byte stores, u16 rows as one (the row's first halfword is the
// id, so a word is one group's end and the next group's begin: `carry`), u8 rows as one of 8 bytes; global memory takes them at any
// alignment.  rec: FinRec, or FinAhead::At (info = 0: the id of a state's record is the result, -1 and -2-k included).
struct __attribute__((packed)) UnalignedU32x4 { u32x4 v; };
struct __attribute__((packed)) UnalignedU32x2 { u32x2 v; };
struct __attribute__((packed)) UnalignedU32 { uint32_t v; };
struct __attribute__((packed)) UnalignedU16 { uint16_t v; };

template <int TIER, typename REC>
__device__ __forceinline__ void store_row(const RowOut& out, uint64_t i, int32_t info, const REC& rec, uint32_t regs, uint32_t len, int G,
                                          uint32_t hop_unset = 0u) {
    const RowFormat f = out.format;
    const int32_t mid = info >= 0 ? static_cast<int32_t>(static_cast<int16_t>(rec.id_of(G))) : info;
    uint8_t* row = f != ROWS_DENSE ? out.rows + i * row_bytes(f, out.slots) : reinterpret_cast<uint8_t*>(out.caps + i * static_cast<uint64_t>(out.slots));
    if (f == ROWS_DENSE) out.match_id[i] = mid;
    uint32_t carry = encode_id(f, mid);
    uint32_t clipped = 0u;
    // (wave-uniform, of the lanes that are here: config 5's u16 rows clip on 1 % of the lines)
    const bool may_clip = __builtin_amdgcn_ballot_w64(len > static_cast<uint32_t>(row_max_offset(f))) != 0ull;
    for (int g0 = 0; g0 < G; g0 += 4) {
        int32_t pb[4], pe[4];
        resolve_tags<TIER>(rec.tags(g0), regs, len, hop_unset, pb, pe);
        const int cnt = G - g0 < 4 ? G - g0 : 4;
        if (f == ROWS_DENSE) {
            uint8_t* dst = row + 8u * g0;
            if (cnt == 4) {
                reinterpret_cast<UnalignedU32x4*>(dst)->v = u32x4{static_cast<uint32_t>(pb[0]), static_cast<uint32_t>(pe[0]), static_cast<uint32_t>(pb[1]), static_cast<uint32_t>(pe[1])};
                reinterpret_cast<UnalignedU32x4*>(dst + 16)->v = u32x4{static_cast<uint32_t>(pb[2]), static_cast<uint32_t>(pe[2]), static_cast<uint32_t>(pb[3]), static_cast<uint32_t>(pe[3])};
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) if (q < cnt) reinterpret_cast<UnalignedU32x2*>(dst + 8 * q)->v = u32x2{static_cast<uint32_t>(pb[q]), static_cast<uint32_t>(pe[q])};
            }
            continue;
        }
        uint32_t hb[4], he[4];
        if (!may_clip) {   // (every offset fits: -1 is the unset value, everything else is itself)
#pragma unroll
            for (int q = 0; q < 4; ++q) { hb[q] = static_cast<uint32_t>(pb[q]) & row_unset(f); he[q] = static_cast<uint32_t>(pe[q]) & row_unset(f); }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const RowUnit b = encode_offset(f, pb[q]), e = encode_offset(f, pe[q]);
                hb[q] = b.unit;
                he[q] = e.unit;
                clipped += b.clipped + e.clipped;
            }
        }
        if (f == ROWS_U16) {
            uint8_t* dst = row + 4u * g0;   // (the halfword before group g0's begin: the id, or the end of the group before)
            if (cnt == 4) {
                reinterpret_cast<UnalignedU32x4*>(dst)->v = u32x4{carry | hb[0] << 16, he[0] | hb[1] << 16, he[1] | hb[2] << 16, he[2] | hb[3] << 16};
                carry = he[3];
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (q >= cnt) break;
                    reinterpret_cast<UnalignedU32*>(dst + 4 * q)->v = carry | hb[q] << 16;
                    carry = he[q];
                }
            }
        } else {
            uint8_t* dst = row + 2u * g0;
            if (cnt == 4) {
                reinterpret_cast<UnalignedU32x2*>(dst)->v = u32x2{carry | hb[0] << 8 | he[0] << 16 | hb[1] << 24, he[1] | hb[2] << 8 | he[2] << 16 | hb[3] << 24};
                carry = he[3];
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (q >= cnt) break;
                    reinterpret_cast<UnalignedU16*>(dst + 2 * q)->v = static_cast<uint16_t>(carry | hb[q] << 8);
                    carry = he[q];
                }
            }
        }
    }
    if (f != ROWS_DENSE) {
        // the row's last unit; slots beyond the definition's groups do not exist (slots == 2 * max_groups == 2 G)
        if (f == ROWS_U8) row[2 * G] = static_cast<uint8_t>(carry);
        else reinterpret_cast<UnalignedU16*>(row + 4 * G)->v = static_cast<uint16_t>(carry);
        if (clipped && out.overflow) atomicAdd(out.overflow, static_cast<unsigned long long>(clipped));
    }
}

// A tile's 64 rows: lane l holds line i (valid: it has one; full: the wave's lines are the 64 lines i - lane .. i - lane + 63, all
// valid, so their rows are one contiguous block of the output).  A full tile's rows go through the wave's LDS area [area, area +
// area_bytes) -- free by now -- so that each store instruction writes 1 KiB of consecutive bytes, instead of every lane writing pieces
// of its own row; otherwise (no room, rows not 16-byte aligned, a partial tile) every valid lane stores its own row.  result(emit) is
// the lane's line_result; slots = out.slots, as the kernel has it at hand (from the walk's G: no register for out.slots).  CLIP = false: the kernel knows that no offset is above row_max_offset(F).  Overflow: one add per wave
// (every lane of the wave is here).
template <RowFormat F, bool CLIP, typename RESULT>
__device__ __forceinline__ void store_tile(const RowOut& out, uint32_t slots, uint64_t i, uint32_t lane, bool valid, bool full, uint32_t area,
                                           uint32_t area_bytes, uint32_t len, RESULT result, uint32_t dev_flags = 0u) {
    (void)dev_flags;
    if (F != ROWS_DENSE) {
        constexpr uint32_t U = row_unit_bytes(F);
        const uint32_t row_b = row_bytes(F, slots);
        constexpr int32_t max = row_max_offset(F);
        auto st = [&](uint32_t lds_at, int32_t v) {
            if (U == 1) lds_st<uint8_t>(lds_at, static_cast<uint8_t>(v));
            else lds_st<uint16_t>(lds_at, static_cast<uint16_t>(v));
        };
        const bool rows_aligned = (reinterpret_cast<uintptr_t>(out.rows) & 15u) == 0u;  // (64 rows are a multiple of 16 bytes)
        uint32_t clipped = 0;
        if (full && rows_aligned && 64u * row_b + 16u <= area_bytes) {
            const uint32_t my_row = area + lane * row_b;
            int32_t id;
            if (!CLIP || !__any(len > static_cast<uint32_t>(max))) {
                // (no offset of this tile's lines is above the limit: nothing to clip or to count)
                id = result([&](int g, int32_t pb, int32_t pe) {
                    st(my_row + U + 2u * U * g, pb);
                    st(my_row + 2u * U + 2u * U * g, pe);
                });
            } else {
                id = result([&](int g, int32_t pb, int32_t pe) {
                    clipped += (pb > max ? 1u : 0u) + (pe > max ? 1u : 0u);
                    st(my_row + U + 2u * U * g, pb > max ? max : pb);
                    st(my_row + 2u * U + 2u * U * g, pe > max ? max : pe);
                });
            }
            st(my_row, id);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            uint8_t* out_rows = out.rows + (i - lane) * static_cast<uint64_t>(row_b);
            for (uint32_t c = lane; c < 4u * row_b; c += 64u) {  // 64 * row_b / 16 chunks
#ifdef GX_DEV
                if (dev_flags & 2u) { __builtin_nontemporal_store(lds_ld<u32x4>(area + (c << 4)), reinterpret_cast<u32x4*>(out_rows + (c << 4))); continue; }
                if ((dev_flags & 4u) && c != 0u) continue;  // experiment: (almost) no result stores
#endif
                *reinterpret_cast<u32x4*>(out_rows + (c << 4)) = lds_ld<u32x4>(area + (c << 4));
            }
        } else if (valid) {
            using Unit = typename std::conditional<U == 1, uint8_t, uint16_t>::type;
            Unit* rp = reinterpret_cast<Unit*>(out.rows) + i * static_cast<uint64_t>(1u + slots);
            auto gst = [&](uint32_t k, int32_t v) { rp[k] = static_cast<Unit>(v); };
            const int32_t id = result([&](int g, int32_t pb, int32_t pe) {
                if (CLIP) {
                    clipped += (pb > max ? 1u : 0u) + (pe > max ? 1u : 0u);
                    gst(1 + 2 * g, pb > max ? max : pb);
                    gst(2 + 2 * g, pe > max ? max : pe);
                } else {
                    gst(1 + 2 * g, pb);
                    gst(2 + 2 * g, pe);
                }
            });
            gst(0, id);
        }
        if (CLIP && out.overflow && __any(clipped != 0u)) {   // (one atomic per wave: the tile kernel is built without the compiler's atomic optimizer)
            uint32_t sum = clipped;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) sum += static_cast<uint32_t>(__shfl_xor(static_cast<int>(sum), d));
            if (lane == 0) atomicAdd(out.overflow, static_cast<unsigned long long>(sum));
        }
    } else {
        const uint32_t row_b = slots * 4u;
        const bool caps_aligned = ((reinterpret_cast<uintptr_t>(out.caps) | reinterpret_cast<uintptr_t>(out.match_id)) & 15u) == 0u;
        if (full && caps_aligned && 64u * row_b + 256u <= area_bytes) {
            const uint32_t my_row = area + lane * row_b;
            const int32_t id = result([&](int g, int32_t pb, int32_t pe) {
                lds_st<u32x2>(my_row + 8u * g, u32x2{static_cast<uint32_t>(pb), static_cast<uint32_t>(pe)});
            });
            const uint32_t ids = area + 64u * row_b;  // the tile's 64 match ids = 256 bytes
            lds_st<uint32_t>(ids + 4u * lane, static_cast<uint32_t>(id));
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            uint8_t* dst = reinterpret_cast<uint8_t*>(out.caps + (i - lane) * static_cast<uint64_t>(slots));
            for (uint32_t c = lane; c < 4u * row_b; c += 64u)  // 64 * row_b / 16 chunks
                *reinterpret_cast<u32x4*>(dst + (c << 4)) = lds_ld<u32x4>(area + (c << 4));  // (nontemporal: measured slower)
            if (lane < 16u)
                *reinterpret_cast<u32x4*>(out.match_id + (i - lane) + 4u * lane) = lds_ld<u32x4>(ids + 16u * lane);
        } else if (valid) {
            int32_t* cp = out.caps + i * static_cast<uint64_t>(slots);
            out.match_id[i] = result([&](int g, int32_t pb, int32_t pe) {   // (this path takes caps at any 4-byte alignment)
                cp[2 * g] = pb;
                cp[2 * g + 1] = pe;
            });
        }
    }
}

}  // namespace gx
