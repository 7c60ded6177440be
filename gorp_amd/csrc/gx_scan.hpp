// gx_scan.hpp -- exclusive scan IN[n] -> u64[n + 1] (out[n] = total) in three launches: block sums, a one-workgroup scan of
// them, block scans.  Shared by the JSON Lines passes (gx_jsonl.hip: text sizes -> text offsets) and the selection passes
// (gx_select.hip: kept flags -> output rows, kept lengths -> output offsets).  No workgroup waits for another one: the
// launches are the only ordering.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace gx {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 8;
constexpr uint64_t SCAN_BLOCK = static_cast<uint64_t>(SCAN_THREADS) * SCAN_ITEMS;

// workgroups of a scan over n items, and the bytes of its block_sums array (nblocks + 2 entries, rounded up to 16)
inline uint64_t scan_blocks(uint64_t n) { return (n + SCAN_BLOCK - 1) / SCAN_BLOCK; }
inline uint64_t scan_sums_bytes(uint64_t n) { return ((scan_blocks(n) + 2) * 8 + 15) & ~static_cast<uint64_t>(15); }

#ifdef __HIPCC__
template <typename IN>
__global__ void __launch_bounds__(SCAN_THREADS) k_scan_block_sums(const IN* __restrict__ in, uint64_t n, uint64_t* __restrict__ block_sums) {
    __shared__ uint64_t wsum[SCAN_THREADS / 64];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * SCAN_BLOCK;
    uint64_t t = 0;
#pragma unroll
    for (int it = 0; it < SCAN_ITEMS; ++it) {
        const uint64_t i = base + static_cast<uint64_t>(it) * SCAN_THREADS + threadIdx.x;
        if (i < n) t += in[i];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor(static_cast<unsigned long long>(t), d);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t s = 0;
        for (int w = 0; w < SCAN_THREADS / 64; ++w) s += wsum[w];
        block_sums[blockIdx.x] = s;
    }
}

// in place: block_sums[b] <- sum of the blocks before b; block_sums[nblocks] <- total
static __global__ void __launch_bounds__(1024) k_scan_of_sums(uint64_t* __restrict__ block_sums, uint64_t nblocks) {
    __shared__ uint64_t wsum[16];
    __shared__ uint64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t b0 = 0; b0 < nblocks; b0 += 1024) {
        const uint64_t b = b0 + threadIdx.x;
        const uint64_t v = b < nblocks ? block_sums[b] : 0;
        uint64_t inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t o = __shfl_up(static_cast<unsigned long long>(inc), d);
            if (lane >= static_cast<uint32_t>(d)) inc += o;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        uint64_t wbase = 0;
        for (uint32_t w = 0; w < wave; ++w) wbase += wsum[w];
        const uint64_t c = carry;
        if (b < nblocks) block_sums[b] = c + wbase + inc - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = c + wbase + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) block_sums[nblocks] = carry;
}

template <typename IN>
__global__ void __launch_bounds__(SCAN_THREADS) k_scan_write(const IN* __restrict__ in, uint64_t n, const uint64_t* __restrict__ block_sums,
                                                             uint64_t nblocks, uint64_t* __restrict__ out) {
    __shared__ uint64_t wsum[SCAN_THREADS / 64];
    __shared__ uint64_t running;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * SCAN_BLOCK;
    if (threadIdx.x == 0) running = block_sums[blockIdx.x];
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = block_sums[nblocks];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (int it = 0; it < SCAN_ITEMS; ++it) {
        const uint64_t i = base + static_cast<uint64_t>(it) * SCAN_THREADS + threadIdx.x;
        const uint64_t v = i < n ? in[i] : 0;
        uint64_t inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t o = __shfl_up(static_cast<unsigned long long>(inc), d);
            if (lane >= static_cast<uint32_t>(d)) inc += o;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        uint64_t wbase = 0;
        for (uint32_t w = 0; w < wave; ++w) wbase += wsum[w];
        const uint64_t r0 = running;
        if (i < n) out[i] = r0 + wbase + inc - v;
        __syncthreads();
        if (threadIdx.x == SCAN_THREADS - 1) running = r0 + wbase + inc;
        __syncthreads();
    }
}

// The three launches, n > 0: out[0..n] from in[0..n); block_sums holds scan_sums_bytes(n) bytes.
template <typename IN>
inline hipError_t launch_exclusive_scan(const IN* in, uint64_t n, uint64_t* block_sums, uint64_t* out, hipStream_t stream) {
    const uint64_t nblocks = scan_blocks(n);
    if (nblocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_scan_block_sums<IN>, dim3(static_cast<unsigned>(nblocks)), dim3(SCAN_THREADS), 0, stream, in, n, block_sums);
    hipLaunchKernelGGL(k_scan_of_sums, dim3(1), dim3(1024), 0, stream, block_sums, nblocks);
    hipLaunchKernelGGL(k_scan_write<IN>, dim3(static_cast<unsigned>(nblocks)), dim3(SCAN_THREADS), 0, stream, in, n, block_sums, nblocks, out);
    return hipGetLastError();
}
#endif

}  // namespace gx
