// gx_radix_dev.hpp -- what the stable LSD radix sorts of gx_partition.hip, gx_group_quantile.hip, gx_by_key.hip and gx_bucket.hip share: six bits a digit, 64 bins,
// one per lane of a wave, and a line's rank among the lines of its bin from ballots alone -- no atomics, so the order of the output
// is the order of the input whatever the waves' timing.  Device code only.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace gx {

// The six ballots of a tile's digits.  bin_mask: the lanes whose digit is `mine` (a lane asks for its own digit: the lines it is
// ranked among; or for its lane number: the lines of the bin it counts).
struct DigitBallots {
    uint64_t valid, bit[6];
};
__device__ __forceinline__ DigitBallots digit_ballots(uint32_t digit, bool valid) {
    DigitBallots b;
    b.valid = __ballot(valid);
#pragma unroll
    for (int q = 0; q < 6; ++q) b.bit[q] = __ballot((digit >> q) & 1u);
    return b;
}
__device__ __forceinline__ uint64_t bin_mask(const DigitBallots& b, uint32_t mine) {
    uint64_t m = b.valid;
#pragma unroll
    for (int q = 0; q < 6; ++q) m &= ((mine >> q) & 1u) ? b.bit[q] : ~b.bit[q];
    return m;
}

}  // namespace gx
