// gx_sort.hip -- the passes of gx_sort_lines / gx_text_sort_lines: a whole batch ordered by a number its lines captured, lines without
// one carried by the line above them, on the device.  The reference's caller does this behind the extraction (README.md:26,63-79):
// results.sort(comparingLong(ts)).  The rule -- a line's class, its place, the digit plan -- is gx_sort.hpp; DESIGN.md section 5.4.
//
// Before the host's ONE wait (launch_sort_entries):
//   keys     launch_top_keys (gx_top.hip), unchanged: every line's class, its key and the candidate flag; the class counts.
//   scan     before[i] = the stamped lines before line i (gx_scan.hpp).
//   compact  ckeys[before[i]] = keys[i]: the stamped keys in line order.
//   entries  one lane per line: the class; the pair (key, line) at its place, a carried line with ckeys[before[i] - 1]; a rest line
//            behind the entries (in both line buffers: the sort moves the entries alone); len[i] and the class byte.  Every workgroup
//            leaves the OR, AND, minimum and maximum of its entries' keys, the code units that leave, its carried and rest lines,
//            whether a stamped key is below the stamped key before it, and whether a line is too long.
//   totals   one workgroup adds the workgroups' words -- integers and bit operations: the order does not matter -- and leaves SortDev.
// Behind the wait, when outputs are wanted (launch_sort_emit):
//   sort     per digit of the plan: k_bucket_count, a scan of the counts, k_bucket_scatter (gx_bucket_sort_dev.hpp, as they are): ranks
//            from ballots, never from atomics, stable whatever the waves' timing.
//   finish   one lane per output line: its length, its value (top_value of the key; 0 for a rest line) and its class.
//   offsets  a scan of the lengths gives the destination offsets.
//   copy     launch_partition_copy (gx_partition.hip) with this workspace's permutation and offsets, called by gx_api.cpp.
// No atomics in global memory at all (the status travels in the workgroups' words), no workgroup waits for another, every loop is
// bounded by an argument or a constant.
//
// The workspace, per line of the batch: 8 (the keys, later the pairs' keys, pong) + 8 (the stamped keys in line order) + 8 (the pairs'
// keys, ping) + 2 x 4 (the pairs' lines) + 8 (the scan, later the destination offsets) + 4 (the lengths by line) + 4 (the lengths in
// output order) + 1 (the candidate flags) + 1 (the classes) = 50 bytes, and 768 bytes per 2 048 lines of counts and bases.
#include <algorithm>
#include <cstdint>
#include <utility>
#include <hip/hip_runtime.h>

#include "gx_bucket_sort_dev.hpp"
#include "gx_device.hpp"
#include "gx_scan.hpp"
#include "gx_sort.hpp"

namespace gx {
namespace {

// (of gx_bucket_sort_dev.hpp this file launches the pair sort's two kernels; the table's two are gx_bucket.hip's and gx_series.hip's)
[[maybe_unused]] const auto not_launched_here = std::make_pair(&k_bucket_flags, &k_bucket_compact);

constexpr uint32_t SORT_LINE_BLOCKS = 2048;
enum : uint32_t { SORT_S_OR = 0, SORT_S_AND, SORT_S_MIN, SORT_S_MAX, SORT_S_UNITS, SORT_S_CARRIED, SORT_S_REST, SORT_S_BITS, SORT_SUMS };
constexpr uint64_t SORT_BIT_UNORDERED = 1ull, SORT_BIT_LONG = 2ull;

// A workgroup's (256 lanes) words reduced into lane 0 of wave 0: w[] by SORT_S_*.
__device__ __forceinline__ void sort_reduce(uint64_t (&w)[SORT_SUMS], uint64_t (*part)[SORT_SUMS]) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        uint64_t o[SORT_SUMS];
#pragma unroll
        for (uint32_t q = 0; q < SORT_SUMS; ++q) o[q] = static_cast<uint64_t>(__shfl_xor(static_cast<u64>(w[q]), d));
        w[SORT_S_OR] |= o[SORT_S_OR];
        w[SORT_S_AND] &= o[SORT_S_AND];
        w[SORT_S_MIN] = o[SORT_S_MIN] < w[SORT_S_MIN] ? o[SORT_S_MIN] : w[SORT_S_MIN];
        w[SORT_S_MAX] = o[SORT_S_MAX] > w[SORT_S_MAX] ? o[SORT_S_MAX] : w[SORT_S_MAX];
        w[SORT_S_UNITS] += o[SORT_S_UNITS];
        w[SORT_S_CARRIED] += o[SORT_S_CARRIED];
        w[SORT_S_REST] += o[SORT_S_REST];
        w[SORT_S_BITS] |= o[SORT_S_BITS];
    }
    if ((threadIdx.x & 63u) == 0u)
#pragma unroll
        for (uint32_t q = 0; q < SORT_SUMS; ++q) part[threadIdx.x >> 6][q] = w[q];
    __syncthreads();
    if (threadIdx.x == 0u) {
#pragma unroll
        for (uint32_t v = 1; v < 4u; ++v) {
            w[SORT_S_OR] |= part[v][SORT_S_OR];
            w[SORT_S_AND] &= part[v][SORT_S_AND];
            w[SORT_S_MIN] = part[v][SORT_S_MIN] < w[SORT_S_MIN] ? part[v][SORT_S_MIN] : w[SORT_S_MIN];
            w[SORT_S_MAX] = part[v][SORT_S_MAX] > w[SORT_S_MAX] ? part[v][SORT_S_MAX] : w[SORT_S_MAX];
            w[SORT_S_UNITS] += part[v][SORT_S_UNITS];
            w[SORT_S_CARRIED] += part[v][SORT_S_CARRIED];
            w[SORT_S_REST] += part[v][SORT_S_REST];
            w[SORT_S_BITS] |= part[v][SORT_S_BITS];
        }
    }
}
__device__ __forceinline__ void sort_words_begin(uint64_t (&w)[SORT_SUMS]) {
#pragma unroll
    for (uint32_t q = 0; q < SORT_SUMS; ++q) w[q] = 0ull;
    w[SORT_S_AND] = ~0ull;
    w[SORT_S_MIN] = ~0ull;
}

// ckeys[at] = line i's key, at = the stamped lines before line i (< n)
__global__ void __launch_bounds__(256) k_sort_compact(uint64_t n, const uint8_t* __restrict__ cand, const uint64_t* __restrict__ before,
                                                      const uint64_t* __restrict__ keys, uint64_t* __restrict__ ckeys) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += stride) {
        if (!cand[i]) continue;
        const uint64_t at = before[i];
        if (at < n) ckeys[at] = keys[i];   // (it is: at <= i)
    }
}

// sums[blockIdx.x][SORT_SUMS]
template <typename OFF>
__global__ void __launch_bounds__(256) k_sort_entries(uint64_t n, const uint8_t* __restrict__ cand, const uint64_t* __restrict__ before,
                                                      const uint64_t* __restrict__ ckeys, const OFF* __restrict__ off, uint32_t carry, uint32_t rest_last,
                                                      uint64_t* __restrict__ word, uint32_t* __restrict__ line0, uint32_t* __restrict__ line1,
                                                      uint32_t* __restrict__ len, uint8_t* __restrict__ cls, uint64_t* __restrict__ sums) {
    __shared__ uint64_t part[4][SORT_SUMS];
    __shared__ uint64_t s_leading;
    if (threadIdx.x == 0u) s_leading = sort_leading(before, n);
    __syncthreads();
    const uint64_t leading = s_leading;
    const uint64_t m = sort_entries(n, before[n], leading, carry != 0u);
    uint64_t w[SORT_SUMS];
    sort_words_begin(w);
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += stride) {
        const bool stamped = cand[i] != 0;
        const uint64_t b = before[i];
        const uint64_t l = static_cast<uint64_t>(off[i + 1]) - static_cast<uint64_t>(off[i]);
        const bool lng = l > 0xFFFFFFFFull;   // (a line of 4 G code units, or offsets that go backwards: refused by the host)
        const uint32_t l32 = lng ? 0u : static_cast<uint32_t>(l);
        const uint32_t c = sort_class(stamped, b, carry != 0u);
        if (lng) w[SORT_S_BITS] |= SORT_BIT_LONG;
        len[i] = l32;
        cls[i] = static_cast<uint8_t>(c);
        if (c != SORT_REST) {
            const uint64_t key = sort_entry_key(ckeys, c, b);   // (b < n stamped, b - 1 < n carried: a stamped line lies at or before this one)
            const uint64_t at = sort_entry_at(i, b, leading, carry != 0u);
            if (at < m) {   // (it is: the places count these very entries)
                word[at] = key;
                line0[at] = static_cast<uint32_t>(i);
            }
            w[SORT_S_OR] |= key;
            w[SORT_S_AND] &= key;
            w[SORT_S_MIN] = key < w[SORT_S_MIN] ? key : w[SORT_S_MIN];
            w[SORT_S_MAX] = key > w[SORT_S_MAX] ? key : w[SORT_S_MAX];
            w[SORT_S_UNITS] += l32;
            w[SORT_S_CARRIED] += c == SORT_CARRIED ? 1u : 0u;
            // (the entries' keys in line order are the stamped keys, each repeated by the lines it carries)
            if (stamped && b > 0u && key < ckeys[b - 1u]) w[SORT_S_BITS] |= SORT_BIT_UNORDERED;
        } else {
            w[SORT_S_REST] += 1u;
            if (rest_last) {
                const uint64_t at = sort_rest_at(i, b, m);
                if (at < n) {   // (it is: entries and rest lines are the batch's lines)
                    line0[at] = static_cast<uint32_t>(i);
                    line1[at] = static_cast<uint32_t>(i);
                }
                w[SORT_S_UNITS] += l32;
            }
        }
    }
    sort_reduce(w, part);
    if (threadIdx.x == 0u)
#pragma unroll
        for (uint32_t q = 0; q < SORT_SUMS; ++q) sums[static_cast<uint64_t>(blockIdx.x) * SORT_SUMS + q] = w[q];
}

// one workgroup; head->counts: the keys pass's (zeros without parts)
__global__ void __launch_bounds__(256) k_sort_totals(const uint64_t* __restrict__ sums, uint32_t blocks, uint64_t n, const uint64_t* __restrict__ before,
                                                     uint32_t carry, SortDev* __restrict__ head) {
    __shared__ uint64_t part[4][SORT_SUMS];
    uint64_t w[SORT_SUMS];
    sort_words_begin(w);
    for (uint32_t b = threadIdx.x; b < blocks; b += 256u) {
        const uint64_t* s = sums + static_cast<uint64_t>(b) * SORT_SUMS;
        w[SORT_S_OR] |= s[SORT_S_OR];
        w[SORT_S_AND] &= s[SORT_S_AND];
        w[SORT_S_MIN] = s[SORT_S_MIN] < w[SORT_S_MIN] ? s[SORT_S_MIN] : w[SORT_S_MIN];
        w[SORT_S_MAX] = s[SORT_S_MAX] > w[SORT_S_MAX] ? s[SORT_S_MAX] : w[SORT_S_MAX];
        w[SORT_S_UNITS] += s[SORT_S_UNITS];
        w[SORT_S_CARRIED] += s[SORT_S_CARRIED];
        w[SORT_S_REST] += s[SORT_S_REST];
        w[SORT_S_BITS] |= s[SORT_S_BITS];
    }
    sort_reduce(w, part);
    if (threadIdx.x == 0u) {
        const uint64_t leading = sort_leading(before, n);
        head->key_or = w[SORT_S_OR];
        head->key_and = w[SORT_S_AND];
        head->key_min = w[SORT_S_MIN];
        head->key_max = w[SORT_S_MAX];
        head->entries = sort_entries(n, before[n], leading, carry != 0u);
        head->carried = w[SORT_S_CARRIED];
        head->rest = w[SORT_S_REST];
        head->units_out = w[SORT_S_UNITS];
        head->unordered = (w[SORT_S_BITS] & SORT_BIT_UNORDERED) ? 1u : 0u;
        head->leading = leading;
        if (w[SORT_S_BITS] & SORT_BIT_LONG) head->counts[TOP_C_STATUS] = 1u;
    }
}

// One lane per output line j: perm[j] its input line; the first m are the sorted entries, word[j] their keys.
__global__ void __launch_bounds__(256) k_sort_finish(uint64_t lines_out, uint64_t m, uint64_t n, const uint32_t* __restrict__ perm, const uint64_t* __restrict__ word,
                                                     const uint32_t* __restrict__ len, const uint8_t* __restrict__ cls, uint32_t descending,
                                                     uint32_t* __restrict__ plen, int64_t* __restrict__ out_values, uint8_t* __restrict__ out_class) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; j < lines_out; j += stride) {
        const uint32_t line = perm[j];
        const bool in = line < n;   // (it is: a line number of the batch)
        plen[j] = in ? len[line] : 0u;
        if (out_values) out_values[j] = j < m ? top_value(word[j], descending != 0u) : 0;
        if (out_class) out_class[j] = in ? cls[line] : static_cast<uint8_t>(SORT_REST);
    }
}

uint64_t pad16(uint64_t v) { return (v + 15) & ~static_cast<uint64_t>(15); }
uint32_t line_blocks(uint64_t n) { return static_cast<uint32_t>(std::min<uint64_t>((n + 255) / 256, SORT_LINE_BLOCKS)); }

}  // namespace

SortWs sort_workspace(void* ws, uint64_t n) {
    const uint64_t slab = GQ_BINS * sort_blocks(n);
    SortWs w{};
    uintptr_t p = reinterpret_cast<uintptr_t>(ws);
    auto take = [&](uint64_t bytes) { const uintptr_t at = p; p += pad16(bytes); return reinterpret_cast<uint8_t*>(at); };
    w.head = take(sizeof(SortDev));
    w.sums = reinterpret_cast<uint64_t*>(take(static_cast<uint64_t>(SORT_LINE_BLOCKS) * SORT_SUMS * 8u));
    w.slab = reinterpret_cast<uint32_t*>(take(std::max<uint64_t>(slab, static_cast<uint64_t>(top_keys_blocks(n)) * TOP_COUNTS) * 4));
    w.bases = reinterpret_cast<uint64_t*>(take((slab + 1) * 8));
    w.block_sums = reinterpret_cast<uint64_t*>(take(std::max(scan_sums_bytes(n), scan_sums_bytes(slab))));
    w.keys = reinterpret_cast<uint64_t*>(take(n * 8));
    w.ckeys = reinterpret_cast<uint64_t*>(take(n * 8));
    w.word[0] = reinterpret_cast<uint64_t*>(take(n * 8));
    w.word[1] = w.keys;      // (the keys are read for the last time by the compaction, before the sort's first pass)
    w.before = reinterpret_cast<uint64_t*>(take((n + 1) * 8));
    w.dst_off = w.before;    // (the stamped lines before line i are read for the last time by the entries pass, before the scan of the lengths)
    for (int q = 0; q < 2; ++q) w.line[q] = reinterpret_cast<uint32_t*>(take(n * 4));
    w.len = reinterpret_cast<uint32_t*>(take(n * 4));
    w.plen = reinterpret_cast<uint32_t*>(take(n * 4));
    w.cand = take(n);
    w.cls = take(n);
    w.bytes = static_cast<size_t>(p - reinterpret_cast<uintptr_t>(ws));
    return w;
}
size_t sort_workspace_bytes(uint64_t n) { return sort_workspace(nullptr, n).bytes; }

// Every pass before the host's wait, on `stream`; 0 < n <= SORT_MAX_LINES.  a: gx_top_lines' arguments, nullptr: the call has no
// parts and every line is a rest line.  Leaves SortDev at w.head.
hipError_t launch_sort_entries(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const TopArgs* a,
                               uint32_t flags, const SortWs& w, hipStream_t stream) {
    if (n == 0 || n > SORT_MAX_LINES) return hipErrorInvalidValue;
    SortDev* head = reinterpret_cast<SortDev*>(w.head);
    hipError_t e = hipMemsetAsync(head, 0, sizeof(SortDev), stream);
    if (e != hipSuccess) return e;
    if (a) {
        TopWs t{};
        t.keys = w.keys;
        t.cand = w.cand;
        t.slab = w.slab;
        e = launch_top_keys(ids, fmt, row_units, K, n, offsets, offsets64, *a, t, head->counts, stream);
    } else {
        e = hipMemsetAsync(w.cand, 0, n, stream);
    }
    if (e != hipSuccess) return e;
    e = launch_exclusive_scan<uint8_t>(w.cand, n, w.block_sums, w.before, stream);
    if (e != hipSuccess) return e;
    const unsigned lb = line_blocks(n);
    const uint32_t carry = (flags & SORT_CARRY) ? 1u : 0u, rest_last = (flags & SORT_REST_LAST) ? 1u : 0u;
    if (a) hipLaunchKernelGGL(k_sort_compact, dim3(lb), dim3(256), 0, stream, n, w.cand, w.before, w.keys, w.ckeys);
    if (offsets64)
        hipLaunchKernelGGL(k_sort_entries<uint64_t>, dim3(lb), dim3(256), 0, stream, n, w.cand, w.before, w.ckeys, static_cast<const uint64_t*>(offsets), carry,
                           rest_last, w.word[0], w.line[0], w.line[1], w.len, w.cls, w.sums);
    else
        hipLaunchKernelGGL(k_sort_entries<uint32_t>, dim3(lb), dim3(256), 0, stream, n, w.cand, w.before, w.ckeys, static_cast<const uint32_t*>(offsets), carry,
                           rest_last, w.word[0], w.line[0], w.line[1], w.len, w.cls, w.sums);
    hipLaunchKernelGGL(k_sort_totals, dim3(1), dim3(256), 0, stream, w.sums, lb, n, w.before, carry, head);
    return hipGetLastError();
}

// Behind launch_sort_entries and the host's read of SortDev on `stream`: m entries, lines_out lines that leave (m, or m + the rest
// lines; 0 < lines_out <= n), the plan from sort_plan.  out_values / out_class: lines_out each on the device, optional.  Leaves the
// input line of output line j in *perm (one of w.line[]) and the code units before it in w.dst_off[0 .. lines_out]: what
// launch_partition_copy reads.
hipError_t launch_sort_emit(uint64_t n, uint64_t m, uint64_t lines_out, const SortPlan& plan, uint32_t flags, const SortWs& w, int64_t* out_values,
                            uint8_t* out_class, uint32_t** perm, hipStream_t stream) {
    if (lines_out == 0 || m > lines_out || lines_out > n || n > SORT_MAX_LINES || plan.n_passes > SORT_MAX_PASSES || (m == 0 && plan.n_passes != 0))
        return hipErrorInvalidValue;
    const uint32_t m32 = static_cast<uint32_t>(m);
    const uint64_t blocks64 = sort_blocks(m);
    const unsigned blocks = static_cast<unsigned>(blocks64);
    uint32_t cur = 0;
    for (uint32_t p = 0; p < plan.n_passes; ++p) {
        const uint32_t d = plan.digit[p];
        if (d >= SORT_MAX_PASSES) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_bucket_count, dim3(blocks), dim3(256), 0, stream, w.word[cur], m32, d, w.slab);
        const hipError_t e = launch_exclusive_scan<uint32_t>(w.slab, GQ_BINS * blocks64, w.block_sums, w.bases, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_bucket_scatter, dim3(blocks), dim3(256), 0, stream, w.word[cur], w.line[cur], m32, d, w.bases, w.word[cur ^ 1u], w.line[cur ^ 1u]);
        cur ^= 1u;
    }
    // (cur == sort_result_buffer(plan.n_passes))
    *perm = w.line[cur];
    hipLaunchKernelGGL(k_sort_finish, dim3(line_blocks(lines_out)), dim3(256), 0, stream, lines_out, m, n, w.line[cur], w.word[cur], w.len, w.cls,
                       (flags & SORT_DESCENDING) ? 1u : 0u, w.plen, out_values, out_class);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_exclusive_scan<uint32_t>(w.plen, lines_out, w.block_sums, w.dst_off, stream);
}

}  // namespace gx
