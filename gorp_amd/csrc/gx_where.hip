// gx_where.hip -- the flags pass of gx_select_lines_where / gx_text_select_where: which lines are kept when the caller asks not only
// WHICH extraction matched but WHAT it captured.  The reference's caller does this right behind the extraction (README.md:26,63-79):
//     r = gorp.extract(line); if (r != null && Long.parseLong(r.asMap().get("timeTakenInMsec")) >= 500) ...
// The capture offsets of a finished batch lie in device memory beside the text; this pass reads them, tests the values they name
// (the rule: gx_where.hpp) and writes the same flags[i] / klen[i] that k_select_flags writes.  The scans and the copy pass behind it are
// gx_select.hip's, unchanged: the copy pass knows nothing of why a line was kept.
//
// One lane per line, the grid shape of k_select_flags.  The terms, their literals and the want mask are copied to LDS once per
// workgroup.  A line is kept when want[outcome] != 0 and, if the outcome is a matched extraction that has terms, every term holds
// (where_line_holds, gx_where_dev.hpp: stated once, for this pass and for gx_stats.hip).
// No atomics per line (one atomicOr for a line of 4 G units, which the host refuses), no histogram (gx_text_select_where takes it from
// k_select_flags' counting form, a read of the id column alone).  DESIGN.md section 5.4.
#include <algorithm>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "gx_device.hpp"
#include "gx_outcome.hpp"
#include "gx_where.hpp"
#include "gx_where_dev.hpp"

namespace gx {
namespace {

extern __shared__ __attribute__((aligned(16))) uint32_t where_smem[];

// image: WhereHead + literals (image_bytes, a multiple of 16).  want_lds != 0: the mask's 2K + 1 bytes go to LDS behind them.
template <typename OFF, RowFormat F, typename UNIT, bool NUM>
__global__ void __launch_bounds__(256) k_where_flags(const void* __restrict__ ids, const int32_t* __restrict__ caps, uint32_t row_units, uint32_t slots,
                                                     uint32_t K, uint64_t n, const OFF* __restrict__ off, const UNIT* __restrict__ data,
                                                     const uint8_t* __restrict__ want, const uint4* __restrict__ image, uint32_t image_bytes,
                                                     uint32_t want_lds, uint8_t* __restrict__ flags, uint32_t* __restrict__ klen,
                                                     uint32_t* __restrict__ status) {
    uint4* img_l = reinterpret_cast<uint4*>(where_smem);
    for (uint32_t q = threadIdx.x; q < (image_bytes >> 4); q += 256u) img_l[q] = image[q];
    const uint8_t* want_l = want;
    if (want_lds) {
        uint8_t* w = reinterpret_cast<uint8_t*>(where_smem) + image_bytes;
        for (uint32_t q = threadIdx.x; q < 2u * K + 1u; q += 256u) w[q] = want[q];
        want_l = w;
    }
    __syncthreads();
    const WhereHead* head = reinterpret_cast<const WhereHead*>(where_smem);
    const UNIT* lits = reinterpret_cast<const UNIT*>(reinterpret_cast<const uint8_t*>(where_smem) + sizeof(WhereHead));
    const uint32_t n_ext = head->n_ext;
    const uint32_t ext_lo = n_ext ? head->ext[0] : 1u, ext_hi = n_ext ? head->ext[n_ext - 1u] : 0u;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += stride) {
        const uint32_t oc = outcome_of(id_of<F>(ids, i, row_units), K);
        bool kept = oc <= 2u * K && want_l[oc] != 0;
        const uint64_t o0 = static_cast<uint64_t>(off[i]), o1 = static_cast<uint64_t>(off[i + 1]);
        const uint64_t len = o1 - o0;
        if (len > 0xFFFFFFFFull) atomicOr(status, 1u);   // (a line of 4 G code units, or offsets that go backwards: refused by the host)
        if (kept && oc >= ext_lo && oc <= ext_hi) {   // (oc <= ext_hi < K: a matched extraction)
            const uint64_t line_units = len > 0xFFFFFFFFull ? 0u : len;   // (no value is looked at in a line that is refused anyway)
            kept = where_line_holds<F, UNIT, NUM>(head, lits, oc, ids, caps, i, row_units, slots, data + o0, line_units);
        }
        flags[i] = kept ? 1 : 0;
        klen[i] = kept ? static_cast<uint32_t>(len) : 0u;
    }
}

template <typename OFF, typename UNIT, bool NUM>
void launch_where_as(RowFormat fmt, unsigned blocks, uint32_t lds, hipStream_t stream, const void* ids, uint32_t row_units, uint32_t K, uint64_t n, const void* off,
                     const WhereArgs& a, uint32_t want_lds, const SelectWs& w) {
    const OFF* o = static_cast<const OFF*>(off);
    const UNIT* d = static_cast<const UNIT*>(a.data);
    const uint4* img = static_cast<const uint4*>(a.image);
    if (fmt == ROWS_U8)
        hipLaunchKernelGGL((k_where_flags<OFF, ROWS_U8, UNIT, NUM>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, w.want, img,
                           a.image_bytes, want_lds, w.flags, w.klen, w.status);
    else if (fmt == ROWS_U16)
        hipLaunchKernelGGL((k_where_flags<OFF, ROWS_U16, UNIT, NUM>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, w.want, img,
                           a.image_bytes, want_lds, w.flags, w.klen, w.status);
    else
        hipLaunchKernelGGL((k_where_flags<OFF, ROWS_DENSE, UNIT, NUM>), dim3(blocks), dim3(256), lds, stream, ids, a.caps, row_units, a.slots, K, n, o, d, w.want, img,
                           a.image_bytes, want_lds, w.flags, w.klen, w.status);
}

}  // namespace

// The flags pass with terms, in launch_select_flags' place: w.want holds the mask, a.image the terms; the pass and the two scans behind
// it leave w.flags, w.idx_off[0..n], w.dst_off[0..n] and w.status.  counts: also the histogram of outcomes in w.counts (k_select_flags'
// counting form, before this pass on the same stream).
hipError_t launch_where_flags(const void* ids, RowFormat fmt, uint32_t row_units, uint32_t K, uint64_t n, const void* offsets, int offsets64,
                              const WhereArgs& a, bool counts, const SelectWs& w, hipStream_t stream) {
    const uint32_t bins = 2u * K + 2u;
    hipError_t e = counts ? launch_select_flags(ids, fmt, row_units, K, n, nullptr, 0, w, stream)   // (zeroes w.counts and w.status first)
                          : hipMemsetAsync(w.status, 0, 16, stream);
    if (e != hipSuccess) return e;
    if (n) {
        const uint32_t want_lds = bins <= SELECT_LDS_BINS ? 1u : 0u;
        const uint32_t lds = a.image_bytes + (want_lds ? ((bins + 15u) & ~15u) : 0u);
        const unsigned blocks = static_cast<unsigned>(std::min<uint64_t>((n + 255) / 256, 2048));
        // (a.formats: a term reads a group under another number format than LONG -- the instantiation with the wider parser)
        auto go = [&](auto off_t, auto unit_t) {
            using OFF = decltype(off_t);
            using UNIT = decltype(unit_t);
            if (a.formats) launch_where_as<OFF, UNIT, true>(fmt, blocks, lds, stream, ids, row_units, K, n, offsets, a, want_lds, w);
            else launch_where_as<OFF, UNIT, false>(fmt, blocks, lds, stream, ids, row_units, K, n, offsets, a, want_lds, w);
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
    }
    return launch_select_scans(n, w, stream);
}

}  // namespace gx
