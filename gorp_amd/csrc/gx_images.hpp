// gx_images.hpp -- the batch kernels' table images and their LDS layouts, and the choice of kernel for a batch.  Host
// arithmetic over Tables, no HIP: gx_api.cpp uploads the images and launches what plan_batch chooses.
#pragma once
#include <vector>

#include "gx_compile.hpp"
#include "gx_hop.hpp"
#include "gx_layout.hpp"

namespace gx {

// A table image under construction: every part starts at a multiple of 16 bytes.
struct Image {
    std::vector<uint8_t> bytes;
    template <typename V> size_t put(const V* p, size_t count) {
        while (bytes.size() % 16) bytes.push_back(0);
        size_t at = bytes.size();
        const uint8_t* b = reinterpret_cast<const uint8_t*>(p);
        bytes.insert(bytes.end(), b, b + count * sizeof(V));
        return at;
    }
    template <typename V> size_t put(const std::vector<V>& v) { return put(v.data(), v.size()); }
};

// An image that a batch kernel copies into LDS: its layout (GxLds::tier 0-3) and its bytes.
// rows / records / fused: what the image was built from, for gx_stat alone -- the automaton rows it covers, the range records they
// became (0: dense rows), whether its capture side is the fused automaton.
struct DenseImage { GxLds L{}; std::vector<uint8_t> bytes; uint32_t rows = 0, records = 0; bool fused = false; };
// The hop tier of one automaton (gx_hop.hpp), laid out for the tile kernel (full) and for the hop slice kernel (small).
struct HopTier { bool ok = false; HopImage img; GxLds full{}, small{}; };

// The images a handle uploads, by id, in the order it uploads them; its device copies are indexed the same way.
// IMG_DENSE + k: dense[k]; IMG_L2: l2; IMG_HOP + 3 k + HOP_FULL / HOP_SMALL / HOP_GLOBAL: hop[k].
enum { IMG_DENSE = 0, IMG_L2 = 2, IMG_HOP = 3, IMG_COUNT = 9 };
enum { HOP_FULL = 0, HOP_SMALL = 1, HOP_GLOBAL = 2 };

struct TileImages {
    bool tile_ok = false, tile_global = false, has_mo = false;
    DenseImage dense[2];            // [0] the batch image (the fused automaton, or all automata); [1] the match automaton alone (has_mo)
    std::vector<uint8_t> l2;        // tiers 1 and 3: rows / records in global memory
    HopTier hop[2];                 // [0] capture batches, [1] match-only batches
    int hop_reason = 4;             // why capture batches have no hop tables (gx_stat(h, 26); 0: they have)
    bool has_capture = false;       // (of the tables: what the planners need of them)
    int max_groups = 0;

    // The dense image of a batch: a match-only batch takes the match automaton's own image where there is one, else the batch
    // image.  (The hop tier has no such fallback: hop[mo].)
    int dense_of(bool mo) const { return mo && has_mo ? 1 : 0; }
    // the bytes of image `id`, or nullptr when the handle has no such image
    const std::vector<uint8_t>* image(int id) const;
};

// Kernel choice at creation: dense rows in LDS when they fit, else range records in LDS, else dense rows in global memory (L2),
// else the per-line kernel alone; and the hop tier beside them.  create_flags: GX_CREATE_*.
TileImages choose_tile_images(const Tables& T, uint32_t create_flags);

// Layouts of one launch.  mo: a match-only batch; wide: the kernel variant that reads UTF-16 code units.
bool plan_tile_layout(GxLds L, uint32_t line_bytes_hint, GxLds* out, bool wide = false);
bool plan_tile_launch(const TileImages& I, uint32_t line_bytes_hint, GxLds* out, bool mo = false, bool wide = false);
bool plan_hop_launch(const TileImages& I, uint32_t line_bytes_hint, GxLds* out, bool mo = false, bool wide = false);
bool plan_lanes_launch(const TileImages& I, GxLds* out, bool mo, bool compact, bool sorted = false, uint64_t n = 0, int num_cus = 256);
bool plan_slice_launch(const TileImages& I, GxLds* out, bool mo = false);
bool plan_hop_slice_launch(const TileImages& I, GxLds* out, bool mo = false);
// the resident one-line service (gx_service.hip): one wave over the dense rows in LDS; false where the handle cannot have it
bool plan_service(const TileImages& I, GxLds* out);

// What plan_batch needs to know of a batch.
struct BatchShape {
    bool wide = false;          // UTF-16 code units
    bool want_states = false;   // GxBatch::state_out
    int match_only = 0;         // GxBatch::match_only
    bool packed = false;        // compact result rows
    uint64_t n = 0;
    uint32_t line_bytes_hint = 0;
    bool uneven = false;
    uint32_t kernel = 0;        // gx_batch_opts.kernel (GX_KERNEL_AUTO: choose)
};
// Which kernel runs a batch, on which images, and how its follow-up launch is sized.
struct BatchPlan {
    bool narrow = false;        // UTF-16 units: narrow them to bytes first, then plan the narrowed copy
    int kernel = GX_KERNEL_PER_LINE;   // GX_KERNEL_* that runs (GX_KERNEL_PER_LINE: the per-line kernel, no tables)
    GxLds L{};
    int image = -1, global = -1;   // IMG_* of the image the kernel copies into LDS and of the one it reads in global memory (-1: none)
    uint32_t fits = 0;          // the longest line the kernel takes (a promise within it needs no follow-up launch)
    uint32_t limit = 0;         // launch_extract_oversize's arguments
    int by_length = 0;
};
BatchPlan plan_batch(const TileImages& I, const BatchShape& s, int num_cus);

}  // namespace gx
