// gx_by_key.hip -- the passes of gx_lines_by_key / gx_text_lines_by_key behind gx_group_lines' own (gx_group.hip): every key's lines
// together, keys in order of their first line, lines in input order inside each, on the device.  The reference's caller does this behind
// the extraction (README.md:26,63-79): byRequest.computeIfAbsent(requestId, k -> new ArrayList<>()).add(line).  The rule -- the keep
// rule, the digit plan, a key's run -- is gx_by_key.hpp; DESIGN.md section 5.4.
//
// Before the host's ONE read of the totals (launch_by_key_kept, behind launch_group_build on the same stream):
//   kept     one lane per line: kept[i] = slot_of[i] is a slot and the slot's line count (the table's head words) is within the bounds;
//            len[i] = the line's units.  Every workgroup leaves the units of its kept lines and the kept lines that are their key's
//            first (the build's flags: one per key); ONE scan (gx_scan.hpp) of the 1-byte flags counts the kept lines before every
//            line; k_bk_totals, one workgroup, adds the workgroups' sums -- integers: the order does not matter -- and leaves ByKeyDev.
// Behind it and behind launch_group_emit, which numbers the slots' keys (launch_by_key_sort):
//   compact  the kept lines' (key number, line number) densely, in line order.
//   sort     per digit of the plan: count (a workgroup owns BK_BLOCK consecutive entries and leaves its 64 counts, bin-major), a scan of
//            the counts, scatter (every entry to the base of its bin + its rank among the entries before it).  The ranks come from
//            ballots (gx_radix_dev.hpp), never from atomics: the sort is stable whatever the waves' timing.  The last scatter also
//            leaves the lines' lengths in output order (no pass at all -- one key -- and the compaction leaves them).
//   bounds   a scan of those lengths gives the destination offsets; one lane per key j in 0 .. n_keys writes key_out_lines[j] and
//            key_out_units[j] by lower bound over the sorted key numbers.
//   copy     launch_partition_copy (gx_partition.hip) with this workspace's permutation and destination offsets, called by gx_api.cpp.
// The sort's two kernels are the third instance of gx_partition.hip's and gx_group_quantile.hip's (what travels with the key differs:
// here the line number, and the lengths are gathered by it at the end); DESIGN.md section 5.4 says why they are not one template.
// No atomics in global memory but the status bit the build pass also sets, no workgroup waits for another, every loop is bounded by an
// argument or a constant.
//
// The workspace, per line of the batch: 8 (the scan, later the destination offsets) + 2 x 4 (the key numbers, ping and pong) + 2 x 4
// (the line numbers) + 4 (the lengths by line) + 4 (the lengths in output order) + 1 (the flags) = 33 bytes, and 768 bytes per BK_BLOCK
// lines of counts and bases.
#include <algorithm>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "gx_by_key.hpp"
#include "gx_device.hpp"
#include "gx_group.hpp"
#include "gx_radix_dev.hpp"
#include "gx_scan.hpp"

namespace gx {
namespace {

typedef unsigned long long u64;

constexpr uint32_t BK_TILES = 8;                      // 64-entry tiles a wave owns in the sort's passes
constexpr uint32_t BK_BLOCK = 4u * BK_TILES * 64u;    // entries a sort workgroup (four waves) owns: 2 048
constexpr uint32_t BK_LINE_BLOCKS = 2048;

// sums[2 b], sums[2 b + 1] = workgroup b's kept units and kept keys
template <typename OFF>
__global__ void __launch_bounds__(256) k_bk_kept(uint64_t n, const uint32_t* __restrict__ slot_of, const uint64_t* __restrict__ gw, uint32_t n_slots,
                                                 const uint8_t* __restrict__ first, const OFF* __restrict__ off, uint64_t min_lines, uint64_t max_lines,
                                                 uint8_t* __restrict__ kept, uint32_t* __restrict__ len, uint64_t* __restrict__ sums, u64* __restrict__ totals) {
    __shared__ uint64_t w_units[4], w_keys[4];
    uint64_t units = 0, keys = 0;
    bool too_long = false;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += stride) {
        const uint32_t slot = slot_of[i];
        const bool k = slot < n_slots && by_key_kept(gw[static_cast<uint64_t>(slot) * GROUP_HEAD_WORDS + GROUP_W_LINES], min_lines, max_lines);
        const uint64_t l = static_cast<uint64_t>(off[i + 1]) - static_cast<uint64_t>(off[i]);
        const bool lng = l > 0xFFFFFFFFull;   // (a line of 4 G code units, or offsets that go backwards: refused by the host)
        too_long |= lng;
        const uint32_t l32 = lng ? 0u : static_cast<uint32_t>(l);
        kept[i] = k ? 1 : 0;
        len[i] = l32;
        if (k) {
            units += l32;
            keys += first[i] ? 1u : 0u;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        units += static_cast<uint64_t>(__shfl_xor(static_cast<u64>(units), d));
        keys += static_cast<uint64_t>(__shfl_xor(static_cast<u64>(keys), d));
    }
    if ((threadIdx.x & 63u) == 0u) { w_units[threadIdx.x >> 6] = units; w_keys[threadIdx.x >> 6] = keys; }
    if (__ballot(too_long) != 0ull && (threadIdx.x & 63u) == 0u) atomicOr(totals + 2, 1ull);   // (the build pass's bit)
    __syncthreads();
    if (threadIdx.x == 0u) {
        sums[2u * blockIdx.x] = w_units[0] + w_units[1] + w_units[2] + w_units[3];
        sums[2u * blockIdx.x + 1u] = w_keys[0] + w_keys[1] + w_keys[2] + w_keys[3];
    }
}

__global__ void __launch_bounds__(256) k_bk_totals(const uint64_t* __restrict__ sums, uint32_t blocks, const uint64_t* __restrict__ total, ByKeyDev* __restrict__ head) {
    __shared__ uint64_t w_units[4], w_keys[4];
    uint64_t units = 0, keys = 0;
    for (uint32_t b = threadIdx.x; b < blocks; b += 256u) { units += sums[2u * b]; keys += sums[2u * b + 1u]; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        units += static_cast<uint64_t>(__shfl_xor(static_cast<u64>(units), d));
        keys += static_cast<uint64_t>(__shfl_xor(static_cast<u64>(keys), d));
    }
    if ((threadIdx.x & 63u) == 0u) { w_units[threadIdx.x >> 6] = units; w_keys[threadIdx.x >> 6] = keys; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        head->lines_out = *total;
        head->units_out = w_units[0] + w_units[1] + w_units[2] + w_units[3];
        head->keys_kept = w_keys[0] + w_keys[1] + w_keys[2] + w_keys[3];
        head->spare = 0;
    }
}

// knum[at], line[at] = line i's key number and i, at = the kept lines before line i; plen (one key: no pass follows): its length too
__global__ void __launch_bounds__(256) k_bk_compact(uint64_t n, const uint8_t* __restrict__ kept, const uint64_t* __restrict__ before,
                                                    const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ keynum, uint32_t n_slots,
                                                    const uint32_t* __restrict__ len, uint64_t m, uint32_t* __restrict__ knum, uint32_t* __restrict__ line,
                                                    uint32_t* __restrict__ plen) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += stride) {
        if (!kept[i]) continue;
        const uint64_t at = before[i];
        if (at >= m) continue;   // (it is not: the scan counted these very flags, and the host read m from it)
        const uint32_t slot = slot_of[i];
        knum[at] = slot < n_slots ? keynum[slot] : GROUP_NONE;   // (it is: a kept line has a slot)
        line[at] = static_cast<uint32_t>(i);
        if (plen) plen[at] = len[i];
    }
}

// slab[bin * gridDim.x + workgroup] = the workgroup's entries whose digit is `bin` (k_part_count's layout)
__global__ void __launch_bounds__(256) k_bk_count(const uint32_t* __restrict__ knum, uint32_t m, uint32_t shift, uint32_t* __restrict__ slab) {
    __shared__ uint32_t wcnt[4][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * BK_BLOCK + static_cast<uint64_t>(wave) * (BK_TILES * 64u);
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t t = 0; t < BK_TILES; ++t) {
        const uint64_t i = base + t * 64u + lane;
        const bool valid = i < m;
        const uint32_t digit = valid ? gq_digit(knum[i], shift) : 0u;
        cnt += static_cast<uint32_t>(__popcll(bin_mask(digit_ballots(digit, valid), lane)));
    }
    wcnt[wave][lane] = cnt;
    __syncthreads();
    if (wave == 0) slab[static_cast<uint64_t>(lane) * gridDim.x + blockIdx.x] = wcnt[0][lane] + wcnt[1][lane] + wcnt[2][lane] + wcnt[3][lane];
}

// The key number and the line number travel.  LAST: the lines' lengths leave in output order too (len[] is by input line, n of them).
template <bool LAST>
__global__ void __launch_bounds__(256) k_bk_scatter(const uint32_t* __restrict__ kin, const uint32_t* __restrict__ lin, uint32_t m, uint32_t shift,
                                                    const uint64_t* __restrict__ bases, uint32_t* __restrict__ kout, uint32_t* __restrict__ lout,
                                                    const uint32_t* __restrict__ len, uint64_t n, uint32_t* __restrict__ plen) {
    __shared__ uint32_t wcnt[4][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * BK_BLOCK + static_cast<uint64_t>(wave) * (BK_TILES * 64u);
    uint32_t k[BK_TILES], l[BK_TILES];
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t t = 0; t < BK_TILES; ++t) {
        const uint64_t i = base + t * 64u + lane;
        const bool valid = i < m;
        k[t] = valid ? kin[i] : 0u;
        l[t] = valid ? lin[i] : 0u;
        cnt += static_cast<uint32_t>(__popcll(bin_mask(digit_ballots(gq_digit(k[t], shift), valid), lane)));
    }
    wcnt[wave][lane] = cnt;
    __syncthreads();
    // lane b: where bin b's next entry of this wave goes (m < 2^32)
    uint32_t next = static_cast<uint32_t>(bases[static_cast<uint64_t>(lane) * gridDim.x + blockIdx.x]);
    for (uint32_t w = 0; w < wave; ++w) next += wcnt[w][lane];
#pragma unroll
    for (uint32_t t = 0; t < BK_TILES; ++t) {
        const uint64_t i = base + t * 64u + lane;
        const bool valid = i < m;
        const uint32_t digit = gq_digit(k[t], shift);
        const DigitBallots b = digit_ballots(digit, valid);
        const uint64_t same = bin_mask(b, digit);
        const uint32_t rank = static_cast<uint32_t>(__popcll(same & ((1ull << lane) - 1ull)));
        const uint32_t to = static_cast<uint32_t>(__shfl(static_cast<int>(next), static_cast<int>(digit))) + rank;
        next += static_cast<uint32_t>(__popcll(bin_mask(b, lane)));
        if (valid && to < m) {   // (it is: the bases and the ranks count these very m entries)
            kout[to] = k[t];
            lout[to] = l[t];
            if (LAST) plen[to] = l[t] < n ? len[l[t]] : 0u;   // (it is: a line number of the batch)
        }
    }
}

// One lane per j in 0 .. n_keys: the first output line of key j (j = n_keys: all of them) and the code units before it.
__global__ void __launch_bounds__(256) k_bk_bounds(const uint32_t* __restrict__ knum, uint64_t m, uint64_t n_keys, const uint64_t* __restrict__ dst_off,
                                                   uint64_t* __restrict__ key_out_lines, uint64_t* __restrict__ key_out_units) {
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (j > n_keys) return;
    const uint64_t at = by_key_begin(knum, m, j);   // (<= m; dst_off has m + 1 entries)
    if (key_out_lines) key_out_lines[j] = at;
    if (key_out_units) key_out_units[j] = dst_off[at];
}

uint64_t pad16(uint64_t v) { return (v + 15) & ~static_cast<uint64_t>(15); }
uint64_t bk_blocks(uint64_t m) { return (m + BK_BLOCK - 1) / BK_BLOCK; }
uint32_t line_blocks(uint64_t n) { return static_cast<uint32_t>(std::min<uint64_t>((n + 255) / 256, BK_LINE_BLOCKS)); }

}  // namespace

ByKeyWs by_key_workspace(void* ws, uint64_t n) {
    const uint64_t slab = GQ_BINS * bk_blocks(n);
    ByKeyWs w{};
    uintptr_t p = reinterpret_cast<uintptr_t>(ws);
    auto take = [&](uint64_t bytes) { const uintptr_t at = p; p += pad16(bytes); return reinterpret_cast<uint8_t*>(at); };
    w.head = take(sizeof(ByKeyDev));
    w.sums = reinterpret_cast<uint64_t*>(take(BK_LINE_BLOCKS * 16u));
    w.slab = reinterpret_cast<uint32_t*>(take(slab * 4));
    w.bases = reinterpret_cast<uint64_t*>(take((slab + 1) * 8));
    w.block_sums = reinterpret_cast<uint64_t*>(take(std::max(scan_sums_bytes(n), scan_sums_bytes(slab))));
    w.before = reinterpret_cast<uint64_t*>(take((n + 1) * 8));
    w.dst_off = w.before;   // (the kept lines before line i are read for the last time by the compaction, before the scan of the lengths)
    for (int q = 0; q < 2; ++q) {
        w.knum[q] = reinterpret_cast<uint32_t*>(take(n * 4));
        w.line[q] = reinterpret_cast<uint32_t*>(take(n * 4));
    }
    w.len = reinterpret_cast<uint32_t*>(take(n * 4));
    w.plen = reinterpret_cast<uint32_t*>(take(n * 4));
    w.kept = take(n);
    w.bytes = static_cast<size_t>(p - reinterpret_cast<uintptr_t>(ws));
    return w;
}
size_t by_key_workspace_bytes(uint64_t n) { return by_key_workspace(nullptr, n).bytes; }

// Behind launch_group_build on `stream`; n > 0.  Leaves ByKeyDev at w.head, w.kept, w.len and w.before[0 .. n].
hipError_t launch_by_key_kept(uint64_t n, const void* offsets, int offsets64, const GroupWs& g, uint64_t min_lines, uint64_t max_lines, const ByKeyWs& w,
                              hipStream_t stream) {
    const unsigned lb = line_blocks(n);
    u64* totals = reinterpret_cast<u64*>(g.totals);
    if (offsets64)
        hipLaunchKernelGGL(k_bk_kept<uint64_t>, dim3(lb), dim3(256), 0, stream, n, g.slot_of, g.head_words, g.n_slots, g.flags, static_cast<const uint64_t*>(offsets),
                           min_lines, max_lines, w.kept, w.len, w.sums, totals);
    else
        hipLaunchKernelGGL(k_bk_kept<uint32_t>, dim3(lb), dim3(256), 0, stream, n, g.slot_of, g.head_words, g.n_slots, g.flags, static_cast<const uint32_t*>(offsets),
                           min_lines, max_lines, w.kept, w.len, w.sums, totals);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_exclusive_scan<uint8_t>(w.kept, n, w.block_sums, w.before, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_bk_totals, dim3(1), dim3(256), 0, stream, w.sums, lb, w.before + n, reinterpret_cast<ByKeyDev*>(w.head));
    return hipGetLastError();
}

// Behind launch_by_key_kept, the host's read of ByKeyDev and launch_group_emit (g.keynum) on `stream`: m = the kept lines (0 < m <= n),
// n_passes from by_key_passes.  key_out_lines / key_out_units (device, n_keys + 1 each, optional).  Leaves the input line of output
// line j in *perm (one of w.line[]) and the code units before it in w.dst_off[0 .. m]: what launch_partition_copy reads.
hipError_t launch_by_key_sort(uint64_t n, uint64_t m, uint64_t n_keys, uint32_t n_passes, const GroupWs& g, const ByKeyWs& w, uint64_t* key_out_lines,
                              uint64_t* key_out_units, uint32_t** perm, hipStream_t stream) {
    if (m == 0 || m > n || n > 0xFFFFFFFFull || n_passes > BY_KEY_MAX_PASSES) return hipErrorInvalidValue;
    const uint32_t m32 = static_cast<uint32_t>(m);
    const uint64_t blocks64 = bk_blocks(m);
    const unsigned blocks = static_cast<unsigned>(blocks64);
    hipLaunchKernelGGL(k_bk_compact, dim3(line_blocks(n)), dim3(256), 0, stream, n, w.kept, w.before, g.slot_of, g.keynum, g.n_slots, w.len, m, w.knum[0], w.line[0],
                       n_passes == 0u ? w.plen : nullptr);
    uint32_t cur = 0;
    for (uint32_t p = 0; p < n_passes; ++p) {
        const uint32_t shift = by_key_shift(p);
        hipLaunchKernelGGL(k_bk_count, dim3(blocks), dim3(256), 0, stream, w.knum[cur], m32, shift, w.slab);
        const hipError_t e = launch_exclusive_scan<uint32_t>(w.slab, GQ_BINS * blocks64, w.block_sums, w.bases, stream);
        if (e != hipSuccess) return e;
        if (p + 1u == n_passes)
            hipLaunchKernelGGL(k_bk_scatter<true>, dim3(blocks), dim3(256), 0, stream, w.knum[cur], w.line[cur], m32, shift, w.bases, w.knum[cur ^ 1u], w.line[cur ^ 1u],
                               w.len, n, w.plen);
        else
            hipLaunchKernelGGL(k_bk_scatter<false>, dim3(blocks), dim3(256), 0, stream, w.knum[cur], w.line[cur], m32, shift, w.bases, w.knum[cur ^ 1u], w.line[cur ^ 1u],
                               w.len, n, w.plen);
        cur ^= 1u;
    }
    // (cur == by_key_result_buffer(n_passes))
    *perm = w.line[cur];
    hipError_t e = launch_exclusive_scan<uint32_t>(w.plen, m, w.block_sums, w.dst_off, stream);
    if (e != hipSuccess) return e;
    if (key_out_lines || key_out_units)
        hipLaunchKernelGGL(k_bk_bounds, dim3(static_cast<unsigned>((n_keys + 1 + 255) / 256)), dim3(256), 0, stream, w.knum[cur], m, n_keys, w.dst_off, key_out_lines,
                           key_out_units);
    return hipGetLastError();
}

}  // namespace gx
