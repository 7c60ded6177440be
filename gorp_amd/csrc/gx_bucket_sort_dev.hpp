// gx_bucket_sort_dev.hpp -- device code the passes of gx_bucket_lines (gx_bucket.hip) and of gx_group_series (gx_series.hip) share: the
// occupied flags and the compaction of a table of 64-bit words (0 = empty), and the LSD radix sort of (64-bit word, 32-bit slot) pairs
// over 6-bit digits by ballot ranks (gx_radix_dev.hpp).  The kernels were gx_bucket.hip's and moved here unchanged, as group_lds_entry
// moved into gx_group_dev.hpp: a translation unit that includes this header compiles them as its own.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include "gx_bucket.hpp"
#include "gx_radix_dev.hpp"

namespace gx {
namespace {

typedef unsigned long long u64;

constexpr uint32_t BKT_TILES = 8;                       // 64-pair tiles a wave owns in the sort's passes
constexpr uint32_t BKT_BLOCK = 4u * BKT_TILES * 64u;    // pairs a sort workgroup (four waves) owns: 2 048

// occupied[s] = slot s holds a bucket
__global__ void __launch_bounds__(256) k_bucket_flags(const u64* __restrict__ table, uint32_t n_slots, uint8_t* __restrict__ occupied) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; s < n_slots; s += stride) occupied[s] = table[s] != 0ull ? 1 : 0;
}

// word[at], slot[at] = slot s's word and s, at = the occupied slots before s; m: the buckets the host read from the same scan
__global__ void __launch_bounds__(256) k_bucket_compact(const u64* __restrict__ table, uint32_t n_slots, const uint8_t* __restrict__ occupied,
                                                        const uint64_t* __restrict__ before, uint32_t m, uint64_t* __restrict__ word, uint32_t* __restrict__ slot) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; s < n_slots; s += stride) {
        if (!occupied[s]) continue;
        const uint64_t at = before[s];
        if (at >= m) continue;   // (it is not: the scan counted these very flags, and the host read m from it)
        word[at] = table[s];
        slot[at] = static_cast<uint32_t>(s);
    }
}

// slab[bin * gridDim.x + workgroup] = the workgroup's pairs whose digit is `bin` (k_bk_count's layout)
__global__ void __launch_bounds__(256) k_bucket_count(const uint64_t* __restrict__ word, uint32_t m, uint32_t digit_at, uint32_t* __restrict__ slab) {
    __shared__ uint32_t wcnt[4][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * BKT_BLOCK + static_cast<uint64_t>(wave) * (BKT_TILES * 64u);
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t t = 0; t < BKT_TILES; ++t) {
        const uint64_t i = base + t * 64u + lane;
        const bool valid = i < m;
        const uint32_t digit = valid ? bucket_digit(word[i], digit_at) : 0u;
        cnt += static_cast<uint32_t>(__popcll(bin_mask(digit_ballots(digit, valid), lane)));
    }
    wcnt[wave][lane] = cnt;
    __syncthreads();
    if (wave == 0) slab[static_cast<uint64_t>(lane) * gridDim.x + blockIdx.x] = wcnt[0][lane] + wcnt[1][lane] + wcnt[2][lane] + wcnt[3][lane];
}

// the word and the slot travel
__global__ void __launch_bounds__(256) k_bucket_scatter(const uint64_t* __restrict__ win, const uint32_t* __restrict__ sin, uint32_t m, uint32_t digit_at,
                                                        const uint64_t* __restrict__ bases, uint64_t* __restrict__ wout, uint32_t* __restrict__ sout) {
    __shared__ uint32_t wcnt[4][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * BKT_BLOCK + static_cast<uint64_t>(wave) * (BKT_TILES * 64u);
    uint64_t k[BKT_TILES];
    uint32_t s[BKT_TILES];
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t t = 0; t < BKT_TILES; ++t) {
        const uint64_t i = base + t * 64u + lane;
        const bool valid = i < m;
        k[t] = valid ? win[i] : 0ull;
        s[t] = valid ? sin[i] : 0u;
        cnt += static_cast<uint32_t>(__popcll(bin_mask(digit_ballots(bucket_digit(k[t], digit_at), valid), lane)));
    }
    wcnt[wave][lane] = cnt;
    __syncthreads();
    // lane b: where bin b's next pair of this wave goes (m <= 2^30)
    uint32_t next = static_cast<uint32_t>(bases[static_cast<uint64_t>(lane) * gridDim.x + blockIdx.x]);
    for (uint32_t w = 0; w < wave; ++w) next += wcnt[w][lane];
#pragma unroll
    for (uint32_t t = 0; t < BKT_TILES; ++t) {
        const uint64_t i = base + t * 64u + lane;
        const bool valid = i < m;
        const uint32_t digit = bucket_digit(k[t], digit_at);
        const DigitBallots b = digit_ballots(digit, valid);
        const uint64_t same = bin_mask(b, digit);
        const uint32_t rank = static_cast<uint32_t>(__popcll(same & ((1ull << lane) - 1ull)));
        const uint32_t to = static_cast<uint32_t>(__shfl(static_cast<int>(next), static_cast<int>(digit))) + rank;
        next += static_cast<uint32_t>(__popcll(bin_mask(b, lane)));
        if (valid && to < m) {   // (it is: the bases and the ranks count these very m pairs)
            wout[to] = k[t];
            sout[to] = s[t];
        }
    }
}

inline uint64_t sort_blocks(uint64_t m) { return (m + BKT_BLOCK - 1) / BKT_BLOCK; }

}  // namespace
}  // namespace gx
