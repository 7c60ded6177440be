// gx_stats.hip -- the reduction of gx_capture_stats / gx_text_capture_stats: what the lines of a finished batch captured as numbers,
// summarised on the device.  The reference's caller does this right behind the extraction (README.md:26,63-79):
//     r = gorp.extract(line); if (r != null) metrics.record(Long.parseLong(r.asMap().get("timeTakenInMsec")));
// The capture offsets of a finished batch lie in device memory beside the text; this pass reads them, parses the values they name
// (the rule: gx_stats.hpp, gx_where.hpp) and leaves per measure three counts, the minimum, the maximum, the exact sum and a histogram.
//
// One lane per line, grid-stride, the grid shape of k_where_flags.  The measures, their edges and -- if the call has terms -- the terms
// are copied to LDS once per workgroup; the accumulators and bins live there too.  A wave reduces before it touches LDS, as
// k_select_flags does for its histogram: per distinct extraction of its 64 lines and per measure of that extraction the counts are
// ballot popcounts and lo / hi / min / max a butterfly over the wave, then ONE lane adds them with 64-bit LDS atomics.  A number's
// bin takes one 32-bit LDS add per lane.  Every workgroup leaves its words as one slab and k_stats_sum folds the slabs in a fixed
// order: no atomics in global memory (one atomicOr for a line of 4 G units, which the host refuses).  DESIGN.md section 5.4.
#include <algorithm>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "gx_device.hpp"
#include "gx_outcome.hpp"
#include "gx_stats.hpp"
#include "gx_where_dev.hpp"

namespace gx {
namespace {

extern __shared__ __attribute__((aligned(16))) uint32_t stats_smem[];

__device__ __forceinline__ uint64_t wave_xor64(uint64_t v, int d) { return static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(v), d)); }

// LDS: the measure image (simage_bytes), the term image (wimage_bytes, 0: no terms), n_measures x STATS_WORDS 64-bit words, n_bins
// 32-bit bins.  slab[blockIdx.x][n_measures * STATS_WORDS + n_bins], 64-bit.
template <typename OFF, RowFormat F, typename UNIT, bool NUM>
__global__ void __launch_bounds__(256) k_capture_stats(const void* __restrict__ ids, const int32_t* __restrict__ caps, uint32_t row_units, uint32_t slots,
                                                       uint32_t K, uint64_t n, const OFF* __restrict__ off, const UNIT* __restrict__ data,
                                                       const uint4* __restrict__ simage, uint32_t simage_bytes, const uint4* __restrict__ wimage,
                                                       uint32_t wimage_bytes, unsigned long long* __restrict__ slab, uint32_t* __restrict__ status) {
    uint8_t* smem = reinterpret_cast<uint8_t*>(stats_smem);
    uint4* s_l = reinterpret_cast<uint4*>(smem);
    for (uint32_t q = threadIdx.x; q < (simage_bytes >> 4); q += 256u) s_l[q] = simage[q];
    uint4* w_l = reinterpret_cast<uint4*>(smem + simage_bytes);
    for (uint32_t q = threadIdx.x; q < (wimage_bytes >> 4); q += 256u) w_l[q] = wimage[q];
    __syncthreads();
    const StatsHead* sh = reinterpret_cast<const StatsHead*>(smem);
    const int64_t* edges = reinterpret_cast<const int64_t*>(smem + sizeof(StatsHead));
    const WhereHead* wh = reinterpret_cast<const WhereHead*>(smem + simage_bytes);
    const UNIT* lits = reinterpret_cast<const UNIT*>(smem + simage_bytes + sizeof(WhereHead));
    const uint32_t n_meas = sh->n_measures, n_bins = sh->n_bins, n_ext = sh->n_ext;
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem + simage_bytes + wimage_bytes);
    uint32_t* bins = reinterpret_cast<uint32_t*>(acc + n_meas * STATS_WORDS);
    for (uint32_t q = threadIdx.x; q < n_meas * STATS_WORDS; q += 256u) {
        const uint32_t word = q & (STATS_WORDS - 1u);
        acc[q] = word == STATS_W_MIN ? static_cast<unsigned long long>(STATS_INT64_MAX) : word == STATS_W_MAX ? static_cast<unsigned long long>(STATS_INT64_MIN) : 0ull;
    }
    for (uint32_t q = threadIdx.x; q < n_bins; q += 256u) bins[q] = 0u;
    __syncthreads();
    const uint32_t ext_lo = n_ext ? sh->ext[0] : 1u, ext_hi = n_ext ? sh->ext[n_ext - 1u] : 0u;
    const bool terms = wimage_bytes != 0u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * 256u + (threadIdx.x & ~63u); i0 < n; i0 += stride) {
        const uint64_t i = i0 + lane;
        const bool valid = i < n;
        uint32_t e = n_ext;   // the line's place in ext[]; n_ext: no measure is taken of it
        uint64_t o0 = 0, line_units = 0;
        if (valid) {
            const uint32_t oc = outcome_of(id_of<F>(ids, i, row_units), K);
            o0 = static_cast<uint64_t>(off[i]);
            const uint64_t len = static_cast<uint64_t>(off[i + 1]) - o0;
            if (len > 0xFFFFFFFFull) atomicOr(status, 1u);   // (a line of 4 G code units, or offsets that go backwards: refused by the host)
            line_units = len > 0xFFFFFFFFull ? 0u : len;     // (no value is looked at in a line that is refused anyway)
            if (oc >= ext_lo && oc <= ext_hi) {              // (oc <= ext_hi < K: a matched extraction)
                e = where_find(sh->ext, n_ext, oc);
                if (e < n_ext && terms && !where_line_holds<F, UNIT, NUM>(wh, lits, oc, ids, caps, i, row_units, slots, data + o0, line_units)) e = n_ext;
            }
        }
        // the distinct extractions among the wave's 64 lines that have measures (mostly none or one)
        uint64_t todo = __ballot(e < n_ext);
        while (todo) {
            const uint32_t l = static_cast<uint32_t>(__ffsll(static_cast<unsigned long long>(todo))) - 1u;
            const uint32_t we = static_cast<uint32_t>(__shfl(static_cast<int>(e), static_cast<int>(l)));
            const bool mine = e == we;
            const uint64_t members = __ballot(mine);
            const uint32_t q1 = sh->first[we + 1u];
            for (uint32_t q = sh->first[we]; q < q1; ++q) {   // (the same in every lane)
                const StatsMeasure m = sh->m[q];
                uint32_t cls = 3u;   // 0: a number, 1: unset, 2: no number, 3: not this extraction's line
                int64_t v = 0;
                if (mine) {
                    int32_t pb, pe;
                    pair_of<F>(ids, caps, i, row_units, slots, m.group, pb, pe);
                    if (!where_pair_set(pb, pe, line_units)) cls = 1u;
                    else cls = number_parse_packed<NUM>(m.fmt, data + o0 + static_cast<uint32_t>(pb), static_cast<uint32_t>(pe - pb), &v) ? 0u : 2u;
                }
                unsigned long long* a = acc + q * STATS_WORDS;
#ifdef GX_STATS_PER_LANE
                // (the experiment's other arm, build.py --variant: every lane adds for itself; profiles/capture_stats.txt)
                if (cls == 1u) atomicAdd(a + STATS_W_UNSET, 1ull);
                if (cls == 2u) atomicAdd(a + STATS_W_NOT_NUMBERS, 1ull);
                if (cls == 0u) {
                    atomicAdd(a + STATS_W_NUMBERS, 1ull);
                    atomicAdd(a + STATS_W_LO, static_cast<unsigned long long>(static_cast<uint64_t>(v) & 0xFFFFFFFFull));
                    atomicAdd(a + STATS_W_HI, static_cast<unsigned long long>(stats_high(v)));
                    atomicMin(reinterpret_cast<long long*>(a + STATS_W_MIN), static_cast<long long>(v));
                    atomicMax(reinterpret_cast<long long*>(a + STATS_W_MAX), static_cast<long long>(v));
                    atomicAdd(&bins[m.hist_at + stats_bucket(edges + m.edge_at, m.n_edges, v)], 1u);
                }
#else
                const uint64_t numbers = __ballot(cls == 0u), unset = __ballot(cls == 1u), not_numbers = __ballot(cls == 2u);
                if (lane == l) {
                    if (unset) atomicAdd(a + STATS_W_UNSET, static_cast<unsigned long long>(__popcll(unset)));
                    if (not_numbers) atomicAdd(a + STATS_W_NOT_NUMBERS, static_cast<unsigned long long>(__popcll(not_numbers)));
                }
                if (numbers) {
                    const bool num = cls == 0u;
                    uint64_t lo = num ? (static_cast<uint64_t>(v) & 0xFFFFFFFFull) : 0ull;
                    uint64_t hi = num ? static_cast<uint64_t>(stats_high(v)) : 0ull;   // (two's complement: adds as unsigned)
                    int64_t mn = num ? v : STATS_INT64_MAX, mx = num ? v : STATS_INT64_MIN;
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) {
                        lo += wave_xor64(lo, d);
                        hi += wave_xor64(hi, d);
                        const int64_t omn = static_cast<int64_t>(wave_xor64(static_cast<uint64_t>(mn), d));
                        const int64_t omx = static_cast<int64_t>(wave_xor64(static_cast<uint64_t>(mx), d));
                        mn = omn < mn ? omn : mn;
                        mx = omx > mx ? omx : mx;
                    }
                    if (lane == l) {
                        atomicAdd(a + STATS_W_NUMBERS, static_cast<unsigned long long>(__popcll(numbers)));
                        atomicAdd(a + STATS_W_LO, static_cast<unsigned long long>(lo));
                        atomicAdd(a + STATS_W_HI, static_cast<unsigned long long>(hi));
                        atomicMin(reinterpret_cast<long long*>(a + STATS_W_MIN), static_cast<long long>(mn));
                        atomicMax(reinterpret_cast<long long*>(a + STATS_W_MAX), static_cast<long long>(mx));
                    }
                    if (num) atomicAdd(&bins[m.hist_at + stats_bucket(edges + m.edge_at, m.n_edges, v)], 1u);
                }
#endif
            }
            todo &= ~members;
        }
    }
    __syncthreads();
    const uint32_t words = n_meas * STATS_WORDS;
    unsigned long long* mine = slab + static_cast<uint64_t>(blockIdx.x) * (words + n_bins);
    for (uint32_t q = threadIdx.x; q < words; q += 256u) mine[q] = acc[q];
    for (uint32_t q = threadIdx.x; q < n_bins; q += 256u) mine[words + q] = bins[q];
}

// out[w] = the workgroups' slabs folded, word by word, in a fixed order: min and max for a measure's STATS_W_MIN / _MAX words, a sum
// for every other word and every bin.  One workgroup per word.
__global__ void __launch_bounds__(256) k_stats_sum(const unsigned long long* __restrict__ slab, uint32_t blocks, uint32_t words, uint32_t total,
                                                   unsigned long long* __restrict__ out) {
    __shared__ unsigned long long part[4];
    const uint32_t w = blockIdx.x;
    const uint32_t kind = w < words ? (w & (STATS_WORDS - 1u)) : 0u;
    const bool is_min = kind == STATS_W_MIN, is_max = kind == STATS_W_MAX;
    const unsigned long long identity = is_min ? static_cast<unsigned long long>(STATS_INT64_MAX) : is_max ? static_cast<unsigned long long>(STATS_INT64_MIN) : 0ull;
    auto fold = [&](unsigned long long a, unsigned long long b) -> unsigned long long {
        if (is_min) return static_cast<long long>(b) < static_cast<long long>(a) ? b : a;
        if (is_max) return static_cast<long long>(b) > static_cast<long long>(a) ? b : a;
        return a + b;
    };
    unsigned long long t = identity;
    for (uint32_t b = threadIdx.x; b < blocks; b += 256u) t = fold(t, slab[static_cast<uint64_t>(b) * total + w]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) t = fold(t, wave_xor64(t, d));
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) out[w] = fold(fold(part[0], part[1]), fold(part[2], part[3]));
}

template <typename OFF, typename UNIT, bool NUM>
void launch_stats_as(RowFormat fmt, unsigned blocks, uint32_t lds, hipStream_t stream, const void* ids, uint32_t row_units, uint32_t K, uint64_t n, const void* off,
                     const StatsArgs& a, unsigned long long* slab, uint32_t* status) {
    const OFF* o = static_cast<const OFF*>(off);
    const UNIT* d = static_cast<const UNIT*>(a.data);
    const uint4 *si = static_cast<const uint4*>(a.image), *wi = static_cast<const uint4*>(a.where_image);
    if (fmt == ROWS_U8)
        hipLaunchKernelGGL((k_capture_stats<OFF, ROWS_U8, UNIT, NUM>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, si, a.image_bytes,
                           wi, a.where_image_bytes, slab, status);
    else if (fmt == ROWS_U16)
        hipLaunchKernelGGL((k_capture_stats<OFF, ROWS_U16, UNIT, NUM>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, si, a.image_bytes,
                           wi, a.where_image_bytes, slab, status);
    else
        hipLaunchKernelGGL((k_capture_stats<OFF, ROWS_DENSE, UNIT, NUM>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, si, a.image_bytes,
                           wi, a.where_image_bytes, slab, status);
}

}  // namespace

uint32_t stats_blocks(uint64_t n) { return static_cast<uint32_t>(std::min<uint64_t>((n + 255) / 256, 2048)); }

// ws: [out: total words][status: 16 bytes][slabs: stats_blocks(n) x total words], total = n_measures * STATS_WORDS + n_bins
size_t stats_workspace_bytes(uint64_t n, uint32_t n_measures, uint32_t n_bins) {
    const size_t total = static_cast<size_t>(n_measures) * STATS_WORDS + n_bins;
    return (total * 8 + 16) + static_cast<size_t>(stats_blocks(n)) * total * 8;
}

// The reduction on `stream`: leaves the summed words and bins at ws[0 .. total) and the status word behind them.  n > 0 and
// a.n_measures > 0; the measure image (and the term image, if any) are on the device.
hipError_t launch_capture_stats(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64, const StatsArgs& a,
                                void* ws, hipStream_t stream) {
    const uint32_t words = a.n_measures * STATS_WORDS, total = words + a.n_bins;
    unsigned long long* out = static_cast<unsigned long long*>(ws);
    uint32_t* status = reinterpret_cast<uint32_t*>(out + total);
    unsigned long long* slab = out + total + 2;
    hipError_t e = hipMemsetAsync(status, 0, 16, stream);
    if (e != hipSuccess) return e;
    const uint32_t lds = a.image_bytes + a.where_image_bytes + words * 8u + a.n_bins * 4u;
    if (lds > 64u * 1024u) return hipErrorInvalidValue;   // (64 measures, 1 024 edges, 64 terms of 255 two-byte units: 53 KiB)
    const unsigned blocks = stats_blocks(n);
    // (a.formats: a measure or a term reads a group under another number format than LONG -- the instantiation with the wider parser)
    auto go = [&](auto off_t, auto unit_t) {
        using OFF = decltype(off_t);
        using UNIT = decltype(unit_t);
        if (a.formats) launch_stats_as<OFF, UNIT, true>(fmt, blocks, lds, stream, ids, row_units, K, n, offsets, a, slab, status);
        else launch_stats_as<OFF, UNIT, false>(fmt, blocks, lds, stream, ids, row_units, K, n, offsets, a, slab, status);
    };
    if (a.wide) {
        if (offsets64) go(uint64_t{}, uint16_t{});
        else go(uint32_t{}, uint16_t{});
    } else {
        if (offsets64) go(uint64_t{}, uint8_t{});
        else go(uint32_t{}, uint8_t{});
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_stats_sum, dim3(total), dim3(256), 0, stream, slab, blocks, words, total, out);
    return hipGetLastError();
}

}  // namespace gx
