// gx_api.cpp -- C ABI of libgorp_hip.so (declared in include/gorp_hip.h).
// Host logic only: compile tables, upload them once, launch kernels, move
// results.  There is no CPU execution path for the hot loops in this library:
// every extract/match entry point runs the HIP kernels or fails with GX_E_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstddef>
#include <cstdlib>
#include <map>
#include <mutex>
#include <new>
#include <optional>
#include <string>
#include <thread>
#include <atomic>

#include "gx_by_key.hpp"
#include "gx_compile.hpp"
#include "gx_device.hpp"
#include "gx_dsl.hpp"
#include "gx_group.hpp"
#include "gx_group_quantile.hpp"
#include "gx_lookup.hpp"
#include "gx_pairs.hpp"
#include "gx_bucket.hpp"
#include "gx_series.hpp"
#include "gx_sessions.hpp"
#include "gx_windows.hpp"
#include "gx_spans.hpp"
#include "gx_top_groups.hpp"
#include "gx_hop.hpp"
#include "gx_images.hpp"
#include "gx_number.hpp"
#include "gx_slots.hpp"
#include "gx_sort.hpp"
#include "gx_stats.hpp"
#include "gx_quantile.hpp"
#include "gx_top.hpp"
#include "gx_where.hpp"

using namespace gx;

namespace {

thread_local std::string g_last_error;
// gx_create_on_devices: the handle whose table images (already in its device's memory) this thread's upload() copies from, device
// to device, instead of from host memory
thread_local const gx_handle* g_peer_src = nullptr;

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

#define GX_HIP(expr)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) throw GxError(GX_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// An entry point's body: what it throws leaves the C ABI as an error code and gx_last_error().
template <typename F> int guarded(F&& body) {
    try {
        return body();
    } catch (GxError& e) { return fail(e.code, e.what()); }
    catch (std::bad_alloc&) { return fail(GX_E_NOMEM, "out of memory"); }
    catch (std::exception& e) { return fail(GX_E_ARG, e.what()); }
}

// Move-only owners of HIP resources.  One that holds null makes no HIP call: host-only handles are created and destroyed on machines
// without a GPU.
template <typename P, auto Release> class Owned {
    P p_{};

  public:
    Owned() = default;
    Owned(Owned&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
        return *this;
    }
    ~Owned() { reset(); }
    void reset() {
        if (p_) (void)Release(p_);
        p_ = nullptr;
    }
    P* out() { reset(); return &p_; }   // (for the call that creates the resource)
    P get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
};
template <typename T = void> using DevMem = Owned<T*, hipFree>;
template <typename T> using PinnedMem = Owned<T*, hipHostFree>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;
using MemPool = Owned<hipMemPool_t, hipMemPoolDestroy>;

// Device memory for the length of a call (16 bytes for none).
template <typename T = void> DevMem<T> dev_alloc(size_t bytes) {
    DevMem<T> m;
    GX_HIP(hipMalloc(m.out(), bytes ? bytes : 16));
    return m;
}

// A reduction's outputs, which are the caller's device pointers or -- host_out -- host buffers: of() gives what the kernels write, the
// caller's own pointer or a device twin of `bytes` bytes (one allocation each, 16 bytes for none) that lives as long as this object,
// until the call's last wait; deliver() enqueues the twins' way back behind the kernels.  nullptr (not wanted) stays nullptr.
class HostTwins {
    struct Twin {
        void* callers;
        DevMem<> dev;
        size_t bytes;
    };
    std::vector<Twin> twins_;
    bool host_out_ = false;

  public:
    HostTwins() = default;
    explicit HostTwins(bool host_out) : host_out_(host_out) {}
    template <class T> T* of(T* callers, size_t bytes) {
        if (!callers || !host_out_) return callers;
        twins_.push_back(Twin{callers, dev_alloc(bytes), bytes});
        return static_cast<T*>(twins_.back().dev.get());
    }
    void deliver(hipStream_t stream) const {
        for (const Twin& t : twins_)
            if (t.bytes) GX_HIP(hipMemcpyAsync(t.callers, t.dev.get(), t.bytes, hipMemcpyDeviceToHost, stream));
    }
};

// The results that no kernel writes ("no keys", "no lines", "no cells"): `bytes` bytes of `byte` at an output, in host memory or, on the
// stream, in device memory.  Nothing for an output that is not wanted or empty.
void fill_out(void* p, int byte, size_t bytes, bool host_out, hipStream_t stream) {
    if (!p || !bytes) return;
    if (host_out) memset(p, byte, bytes);
    else GX_HIP(hipMemsetAsync(p, byte, bytes, stream));
}

// Device memory kept between calls and grown as they ask (an allocation and a free per call cost more than the kernels that use it).
struct GrowBuf {
    DevMem<> mem;
    size_t cap = 0;
    void* get(size_t need) {
        if (cap < need) {
            cap = 0;
            GX_HIP(hipMalloc(mem.out(), need + need / 8 + 256));
            cap = need + need / 8 + 256;
        }
        return mem.get();
    }
};

// Puts the calling thread's current device back when the scope ends.
struct DeviceScope {
    int saved = 0;
    DeviceScope() { (void)hipGetDevice(&saved); }
    ~DeviceScope() { (void)hipSetDevice(saved); }
};

// n + 1 line offsets in host memory, 32 or 64 bits each.
struct HostOffsets {
    const void* p;
    bool off64;
    uint64_t n;
    uint64_t operator[](uint64_t i) const { return off64 ? static_cast<const uint64_t*>(p)[i] : static_cast<const uint32_t*>(p)[i]; }
    // the first line from `from` on whose start lies at or beyond `at` (n: none)
    uint64_t lines_at_or_after(uint64_t at, uint64_t from) const {
        uint64_t lo = from, hi = n;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) / 2;
            if ((*this)[mid] >= at) hi = mid;
            else lo = mid + 1;
        }
        return lo;
    }
};

// offsets[0] and offsets[n] of an offsets array in device memory: a small synchronous read on `stream`.
std::pair<uint64_t, uint64_t> device_offset_ends(const void* offsets, uint64_t n, bool off64, hipStream_t stream) {
    const size_t w = off64 ? 8 : 4;
    uint64_t first = 0, last = 0;
    GX_HIP(hipMemcpyAsync(&first, offsets, w, hipMemcpyDeviceToHost, stream));
    GX_HIP(hipMemcpyAsync(&last, static_cast<const uint8_t*>(offsets) + n * w, w, hipMemcpyDeviceToHost, stream));
    GX_HIP(hipStreamSynchronize(stream));
    return {first, last};
}

// Asynchronous device-pointer batches that give no line_bytes_hint: the mean line length of the previous such batch, read back
// without a synchronisation (two offsets copied to pinned memory, picked up by the next call once its event is done).
struct HintProbe {
    std::mutex mu;
    PinnedMem<uint64_t> ends;   // offsets[0], offsets[n] of the batch being probed
    Event event;
    bool pending = false;
    uint64_t n = 0;
    bool off64 = false;
    uint32_t learned = 0;
    // the hint for a batch (what the previous such batch measured; 0 until one has), and a probe of this batch for the next call
    uint32_t next(const void* offsets, uint64_t batch_n, bool batch_off64, hipStream_t stream) {
        std::lock_guard<std::mutex> lock(mu);
        if (!ends) {
            GX_HIP(hipHostMalloc(ends.out(), 16, hipHostMallocDefault));
            GX_HIP(hipEventCreateWithFlags(event.out(), hipEventDisableTiming));
        }
        uint64_t* e = ends.get();
        if (pending && hipEventQuery(event.get()) == hipSuccess) {
            const uint64_t first = off64 ? e[0] : (e[0] & 0xFFFFFFFFull), last = off64 ? e[1] : (e[1] & 0xFFFFFFFFull);
            if (n && last >= first) learned = static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>((last - first + n - 1) / n, 4096)));
            pending = false;
        }
        const uint32_t hint = learned;
        if (!pending) {
            const size_t w = batch_off64 ? 8 : 4;
            e[0] = e[1] = 0;
            GX_HIP(hipMemcpyAsync(&e[0], offsets, w, hipMemcpyDeviceToHost, stream));
            GX_HIP(hipMemcpyAsync(&e[1], static_cast<const uint8_t*>(offsets) + batch_n * w, w, hipMemcpyDeviceToHost, stream));
            GX_HIP(hipEventRecord(event.get(), stream));
            pending = true;
            n = batch_n;
            off64 = batch_off64;
        }
        return hint;
    }
};

}  // namespace

struct gx_handle {
    Tables T;
    std::vector<uint8_t> blob;
    bool on_device = false;
    int device = 0;
    DevMem<> dimage;
    size_t image_bytes = 0;
    GxDev dev{};
    int max_regs = 0;
    // the batch kernels' table images and layouts (gx_images.hpp), and their device copies, by IMG_* id
    TileImages tiles;
    DevMem<> d_img[IMG_COUNT];
    int num_cus = 256;
    std::vector<dsl::Extraction> meta;  // names / extractor names / append (from definition text or gx_set_extraction_meta)
    // gx_set_number_format: per extraction and group the packed format (gx_number.hpp: number_pack); an extraction without an entry,
    // and every group of a new handle, is LONG.  Not part of the blob.
    std::vector<std::vector<uint8_t>> number_formats;
    uint8_t number_format_of(int32_t k, int32_t g) const {
        if (static_cast<size_t>(k) >= number_formats.size() || static_cast<size_t>(g) >= number_formats[k].size()) return 0;
        return number_formats[k][g];
    }
    // scratch of the one-String entry points: device, and its pinned host mirror (one_line)
    struct OneScratch {
        DevMem<uint8_t> dev;
        PinnedMem<uint8_t> host;
        size_t cap = 0;
    } one;
    std::vector<std::vector<std::pair<std::string, std::string>>> append_entries;  // per extraction: (key, value JSON), lazily
    struct JsonlImage { DevMem<> d; GxJsonl dev{}; };
    std::map<std::string, JsonlImage> jsonl;  // device templates per id_as ("0" = none, "1" + id_as)
    std::mutex mu;  // serialises host-pointer batches that share nothing else
    // Host-pointer batches (what a JNI caller hands over) go through a small pipeline: the batch is cut into chunks of
    // whole lines, and HOST_WORKERS threads, each with its own stream and persistent device buffers, take alternate
    // chunks -- copy in, kernels, copy out -- so that one chunk's copy-in overlaps another's kernels and copy-out on
    // the bus' two directions.  (Threads, not just streams: a copy from pageable memory holds its host thread.)
    static const int HOST_WORKERS = 4;
    struct HostSlot {
        Stream stream;
        GrowBuf bytes, off, res, caps, states;   // res: match ids, or compact rows
        DevMem<unsigned long long> over;
    } host_slot[HOST_WORKERS];
    uint32_t create_flags = 0;   // GX_CREATE_* given at creation (kernel choice)
    HintProbe hint;
    // the launch slots (gx_slots.hpp): their bookkeeping, under slot_mu, and their device resources
    LaunchSlots slots;
    std::mutex slot_mu;
    DevMem<uint32_t> d_slots;   // [N] oversize flags, [N] counts behind them (announce_left_line; nobody reads these), then [N] chunk
                                // counters of the lane kernel, then [N] "a line of this UTF-16 batch holds a unit above 0xFF" words
    PinnedMem<uint32_t> h_broken;   // [N] the words of batches that promised their longest line, [N] counts (LaunchSlots::broken), mapped
    uint32_t* d_broken = nullptr;   // the device's address of the same words
    DevMem<uint32_t> d_steal[LaunchSlots::N];   // per slot, at its first tile launch: [2][GX_STEAL_MAX * GX_STEAL_STRIDE], the tile kernel's workgroup counters (GxBatch::steal)
    Event shared_event;   // the shared slot's "previous user is done"
    // the resident one-line service (gx_service.hip; GX_CREATE_RESIDENT_ONE)
    struct Service {
        bool enabled = false;
        int mode = 0;
        GxLds L{};
        PinnedMem<uint32_t> host;   // pinned block: mailbox [17 x 16 dwords] | answer [2 + 2 G dwords, padded] | state
        uint32_t* dev = nullptr;    // the device's address of the same block
        Stream stream;
        uint32_t seq = 0;
        bool started = false;
        uint64_t launches = 0;
    } svc;
    DevMem<int32_t> d_pike_scratch;   // thread lists of the lanes that run an extraction's program as it is (GxDev::pike_scratch)
    // ... ONE set of them per handle, a lane's area named by its place in the grid: two per-line kernels of the handle must not run at
    // once (the host pipeline's four streams, a caller's streams, the one-String calls beside a batch).  Every launch of such a
    // handle waits for the one before it, on whatever stream that was (PikeGate).
    std::recursive_mutex pike_mu;
    Event pike_event;
    bool pike_event_set = false;
    int pike_depth = 0;
    Stream multi_stream;    // gx_extract_batch_multi_device: the stream of shards that bring none
    Stream gather_stream;   // gx_gather_rows: this handle's rows leave for the root's device on it (a copy queue of its own: seven peers, seven links)
    Event gather_event;     // ... "the shard's kernel is done", recorded on the kernel's stream
    size_t peer_image_bytes = 0;          // table bytes that came from another device's copy (gx_create_on_devices; gx_stat(h, 30))
    std::atomic<int> last_kernel{0};      // GX_KERNEL_* of the most recent batch launch (gx_stat(h, 25))
    std::atomic<uint64_t> last_utf8_lines{0}, last_utf8_units{0};   // the most recent utf8 batch: lines walked again, units made (gx_stat(h, 33) and (h, 34))
    std::atomic<uint32_t> last_fits{0}, last_limit{0};   // ... and its BatchPlan::fits and ::limit (gx_stat(h, 31) and (h, 32); 0: a kernel that leaves no line)
    // device scratch of gx_results_to_jsonl / gx_text_to_jsonl (sizes, split points, line offsets), kept between calls.  Used under
    // `mu` only, and every call that uses it ends with a stream synchronisation.
    // (8 .. 11: the partitioned batch of gx_text_to_jsonl_by_extraction -- text, offsets, ids, capture rows)
    GrowBuf scratch[12];
    // device workspace of gx_count_outcomes / gx_select_lines / gx_text_select (gx_device.hpp: SelectWs) and of gx_partition_lines /
    // gx_text_to_jsonl_by_extraction (PartWs), kept between calls and used under `mu`.  A no_sync gx_select_lines or gx_partition_lines
    // leaves its copy pass reading it: the next user's stream waits for select_event first.
    GrowBuf select_ws;
    GrowBuf where_image;   // gx_select_lines_where's terms and literals (WhereHead, gx_where.hpp); read by its flags pass alone
    Event select_event;
    bool select_pending = false;
    // gx_capture_stats: its measures, edges and terms on the device (StatsHead, gx_stats.hpp; WhereHead behind it), and the summed words
    // and the workgroups' slabs (gx_stats.hip).  Used under `mu`; every call that uses them ends with a stream synchronisation.
    GrowBuf stats_image, stats_ws;
    // gx_group_lines: its parts and terms on the device (GroupHead, gx_group.hpp; WhereHead behind it), the slots' words and the per-line
    // arrays (gx_group.hip).  Used under `mu`.  With device pointers the emit pass is left running on the caller's stream: the next
    // call's stream waits for group_event first.
    GrowBuf group_image, group_table, group_lines;
    // gx_group_quantiles behind them: its value parts, quantiles and terms (TopHead, QuantHead, WhereHead) and its workspace; they are
    // covered by group_event too
    GrowBuf gq_image, gq_ws;
    // gx_top_groups behind gx_group_lines' build: its workspace (gx_top_groups.hip), covered by group_event too
    GrowBuf tg_ws;
    // gx_lines_by_key behind gx_group_lines' build and emit: its workspace (gx_by_key.hip), covered by group_event too
    GrowBuf by_key_ws;
    // gx_group_pairs behind gx_group_lines' build: its second groups (PairsHead, gx_pairs.hpp), the pair slots' words and the per-line
    // arrays (gx_pairs.hip), covered by group_event too
    GrowBuf pairs_image, pairs_table, pairs_lines;
    // gx_group_series behind gx_group_lines' build: its number groups (SeriesHead, gx_series.hpp) at the head of both tables' slots' words
    // and arrays, and the lines' cell slots (gx_series.hip); behind the one wait, sized by the cells read there, the sorts' workspace.
    // Covered by group_event too
    GrowBuf series_table, series_lines, series_sort;
    // gx_group_sessions behind gx_group_lines' build: its number groups (SessionsHead, gx_sessions.hpp) at the head of the per-line arrays
    // (gx_sessions.hip: SessionsWs); behind the group's wait, sized by the entries read there, the sorts' and the sessions' workspace
    // (SessionsSortWs).  Covered by group_event too
    GrowBuf sessions_lines, sessions_sort;
    // gx_group_windows shares sessions_lines (the same keys pass); per entry and key its own (WindowsWs).  Covered by group_event too
    GrowBuf windows_ws;
    // gx_group_spans behind gx_group_lines' build: its number groups and roles (SpansHead, gx_spans.hpp) at the head of the per-line arrays
    // (gx_spans.hip: SpansWs); behind the group's wait, sized by the entries and keys read there, the sort's and the pairing's workspace
    // (SpansPairWs).  Covered by group_event too
    GrowBuf spans_lines, spans_pair;
    Event group_event;
    bool group_pending = false;
    // gx_lookup_lines: its parts and terms on the device (GroupHead; WhereHead behind it), the dictionary's slots' words and the per-entry
    // and per-line arrays (gx_lookup.hip: LookupWs).  Used under `mu`.  With device pointers the emit is left running on the caller's
    // stream: the next call's stream waits for lookup_event first (its copy pass reads select_ws: select_event likewise).
    GrowBuf lookup_image, lookup_table, lookup_lines;
    Event lookup_event;
    bool lookup_pending = false;
    // gx_bucket_lines: its parts and terms on the device (BucketHead, gx_bucket.hpp; WhereHead behind it), the slots' words and arrays,
    // the lines' slots and the sort's workspace (gx_bucket.hip).  Used under `mu`.  With device pointers the sort and the emit are left
    // running on the caller's stream: the next call's stream waits for bucket_event first.
    GrowBuf bucket_image, bucket_table, bucket_lines, bucket_sort;
    Event bucket_event;
    bool bucket_pending = false;
    // gx_top_lines: its parts and terms on the device (TopHead, gx_top.hpp; WhereHead behind it) and the passes' workspace (gx_top.hip:
    // TopWs).  Used under `mu`.  With device pointers the emit pass is left running on the caller's stream and still reads the
    // workspace: the next call's stream waits for top_event first (gx_partition_lines' rule for its no_sync copy pass).
    GrowBuf top_image, top_ws;
    Event top_event;
    bool top_pending = false;
    // gx_sort_lines: its parts and terms on the device (TopHead; WhereHead behind it) and the passes' workspace (gx_sort.hip: SortWs).
    // Used under `mu`.  With device pointers the sort, the finish and the copy are left running on the caller's stream and still read
    // the workspace: the next call's stream waits for sort_event first.
    GrowBuf sort_image, sort_ws;
    Event sort_event;
    bool sort_pending = false;
    // gx_capture_quantiles: its parts, quantiles and terms on the device (TopHead, QuantHead, WhereHead) and the passes' workspace
    // (gx_quantile.hip: QuantWs).  Used under `mu`; every call that uses them ends with a stream synchronisation.
    GrowBuf quant_image, quant_ws;
    // stream-ordered memory of the UTF-16 batch path (the narrowed copy of a batch): a pool of the handle's own that keeps what a
    // batch frees for the next one (the device's default pool gives everything back at the next synchronisation: an allocation of
    // gigabytes per call, 0.6 of that path's 2.4 ms per 10 M lines)
    MemPool pool;
#ifdef GX_DEV
    unsigned long long* dev_stamps = nullptr;  // developer build: device buffer for the tile kernel's phase cycle counts
#endif
};

namespace {

// One table image into the handle's device: from host memory, or -- gx_create_on_devices -- from the same image on the device of
// the handle that was built first: a copy between devices (over xGMI where the devices are peers; the runtime stages it otherwise).
static void put_image(gx_handle* h, void* dst, const void* host, size_t bytes, const void* peer) {
    if (bytes == 0) return;
    if (peer && g_peer_src && hipMemcpyPeer(dst, h->device, peer, g_peer_src->device, bytes) == hipSuccess) {
        h->peer_image_bytes += bytes;
        return;
    }
    GX_HIP(hipMemcpy(dst, host, bytes, hipMemcpyHostToDevice));
}

// The thread lists of the extractions that run as programs (gx_kernels.hip: pike_capture): a lane's ints -- the largest program's
// lists, stack, marks and boundaries, then the winning thread's boundaries -- and as many workgroups of 256 lanes as the scratch
// budget holds them for (64 at most, one at least).
void pike_sizing(const Tables& T, uint32_t* lane_ints, uint32_t* blocks) {
    uint32_t ints = 0;
    for (size_t k = 0; k < T.rules.size(); ++k) {
        const uint32_t ni = T.pike_off[k + 1] - T.pike_off[k], W = 1u + 2u * static_cast<uint32_t>(T.rules[k].n_groups);
        if (ni) ints = std::max(ints, 2u * ni * W + 3u * (2u * ni + 2u) + ni + 2u * static_cast<uint32_t>(T.rules[k].n_groups));
    }
    ints += 2u * static_cast<uint32_t>(T.max_groups) + 2u;
    *lane_ints = ints;
    *blocks = static_cast<uint32_t>(std::min<uint64_t>(GX_PIKE_BLOCKS, GX_PIKE_SCRATCH_BYTES / (static_cast<uint64_t>(ints) * 4u * 256u)));
    if (*blocks == 0) *blocks = 1;
}

void upload(gx_handle* h) {
    const Tables& T = h->T;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        throw GxError(GX_E_DEVICE, "no HIP device available (libgorp_hip needs a gfx950 GPU; there is no CPU fallback)");
    GX_HIP(hipGetDevice(&h->device));

    Image img;
    const size_t o_cls = img.put(T.cls256, 256);
    const size_t o_hilo = img.put(T.hi_lo);
    const size_t o_hicls = img.put(T.hi_cls);
    size_t o_next16 = 0, o_next32 = 0;
    const bool small = T.m_states <= 65536;
    if (small) {
        std::vector<uint16_t> n16(T.m_next.begin(), T.m_next.end());
        o_next16 = img.put(n16);
    } else o_next32 = img.put(T.m_next);
    const size_t o_acc = img.put(T.m_accept_first);
    std::vector<uint32_t> trans_all, trans_off, fin_off;
    std::vector<int32_t> fin_all, ngroups;
    int max_regs = 0;
    for (auto& r : T.rules) {
        trans_off.push_back(static_cast<uint32_t>(trans_all.size()));
        trans_all.insert(trans_all.end(), r.trans.begin(), r.trans.end());
        fin_off.push_back(static_cast<uint32_t>(fin_all.size()));
        fin_all.insert(fin_all.end(), r.fin.begin(), r.fin.end());
        ngroups.push_back(r.n_groups);
        max_regs = std::max(max_regs, r.n_regs);
    }
    if (trans_all.empty()) { trans_all.push_back(0); trans_off.push_back(0); fin_all.push_back(-1); fin_off.push_back(0); ngroups.push_back(0); }
    h->max_regs = max_regs;
    if (max_regs > 96) throw GxError(GX_E_LIMIT, "capture automaton needs more than 96 registers");
    const size_t o_trans = img.put(trans_all);
    const size_t o_troff = img.put(trans_off);
    const size_t o_fin = img.put(fin_all);
    const size_t o_finoff = img.put(fin_off);
    const size_t o_ng = img.put(ngroups);
    const size_t o_opsoff = img.put(T.ops_off);
    std::vector<uint16_t> ops = T.ops;
    if (ops.empty()) ops.push_back(0);
    const size_t o_ops = img.put(ops);
    std::vector<uint16_t> fin_tags = T.fin_tags;
    if (fin_tags.empty()) fin_tags.push_back(0);
    const size_t o_fintags = img.put(fin_tags);
    // extractions without a capture automaton: their programs (gx_compile.hpp: Tables::pike_*)
    size_t o_pike_off = 0, o_pike_code = 0, o_pike_sets = 0;
    uint32_t pike_lane_ints = 0, pike_blocks = 0;
    if (T.has_pike()) {
        o_pike_off = img.put(T.pike_off);
        o_pike_code = img.put(T.pike_code);
        o_pike_sets = img.put(T.pike_sets);
        pike_sizing(T, &pike_lane_ints, &pike_blocks);
        if (static_cast<uint64_t>(pike_lane_ints) * 4u * (256u * pike_blocks + 1u) > (1ull << 30))
            throw GxError(GX_E_LIMIT, "capture program too large to run as it is (the thread lists of one workgroup beyond 1 GiB)");
    }

    GX_HIP(hipMalloc(h->dimage.out(), img.bytes.size()));
    h->image_bytes = img.bytes.size();
    put_image(h, h->dimage.get(), img.bytes.data(), img.bytes.size(), g_peer_src ? g_peer_src->dimage.get() : nullptr);
    const uint8_t* base = static_cast<const uint8_t*>(h->dimage.get());
    GxDev& d = h->dev;
    d.cls256 = base + o_cls;
    d.hi_lo = reinterpret_cast<const uint16_t*>(base + o_hilo);
    d.hi_cls = reinterpret_cast<const uint16_t*>(base + o_hicls);
    d.n_hi = static_cast<int32_t>(T.hi_lo.size());
    d.ncls = T.ncls;
    d.m_next16 = small ? reinterpret_cast<const uint16_t*>(base + o_next16) : nullptr;
    d.m_next32 = small ? nullptr : reinterpret_cast<const uint32_t*>(base + o_next32);
    d.m_accept_first = reinterpret_cast<const int32_t*>(base + o_acc);
    d.m_states = T.m_states;
    d.m_dead = T.m_dead;
    d.c_trans = reinterpret_cast<const uint32_t*>(base + o_trans);
    d.c_trans_off = reinterpret_cast<const uint32_t*>(base + o_troff);
    d.c_fin = reinterpret_cast<const int32_t*>(base + o_fin);
    d.c_fin_off = reinterpret_cast<const uint32_t*>(base + o_finoff);
    d.c_ngroups = reinterpret_cast<const int32_t*>(base + o_ng);
    d.ops_off = reinterpret_cast<const uint32_t*>(base + o_opsoff);
    d.ops = reinterpret_cast<const uint16_t*>(base + o_ops);
    d.fin_tags = reinterpret_cast<const uint16_t*>(base + o_fintags);
    d.n_rules = T.n_rules;
    d.max_groups = T.max_groups;
    d.max_regs = max_regs;
    d.has_capture = T.has_capture ? 1 : 0;
    if (T.has_pike()) {
        d.pike_off = reinterpret_cast<const uint32_t*>(base + o_pike_off);
        d.pike_code = reinterpret_cast<const uint32_t*>(base + o_pike_code);
        d.pike_sets = reinterpret_cast<const uint32_t*>(base + o_pike_sets);
        d.pike_lane_ints = pike_lane_ints;
        d.pike_blocks = pike_blocks;
        GX_HIP(hipMalloc(h->d_pike_scratch.out(), static_cast<size_t>(pike_lane_ints) * 4u * (256u * pike_blocks + 1u)));
        d.pike_scratch = h->d_pike_scratch.get();
    }

    h->tiles = choose_tile_images(T, h->create_flags);
    const TileImages& I = h->tiles;
    for (int id = 0; id < IMG_COUNT; ++id) {
        const std::vector<uint8_t>* v = I.image(id);
        if (!v) continue;
        GX_HIP(hipMalloc(h->d_img[id].out(), v->size()));
        put_image(h, h->d_img[id].get(), v->data(), v->size(), g_peer_src ? g_peer_src->d_img[id].get() : nullptr);
    }
    if (I.tile_ok || I.hop[0].ok || I.hop[1].ok) {
        static_assert(GX_SLOT_WORDS == LaunchSlots::N, "announce_left_line counts GX_SLOT_WORDS behind a slot's flag word");
        GX_HIP(hipMalloc(h->d_slots.out(), 4 * LaunchSlots::N * sizeof(uint32_t)));
        GX_HIP(hipMemset(h->d_slots.get(), 0, 4 * LaunchSlots::N * sizeof(uint32_t)));
        GX_HIP(hipEventCreateWithFlags(h->shared_event.out(), hipEventDisableTiming));

        GX_HIP(hipHostMalloc(h->h_broken.out(), 2 * LaunchSlots::N * sizeof(uint32_t), hipHostMallocMapped));
        for (int q = 0; q < 2 * LaunchSlots::N; ++q) h->h_broken.get()[q] = 0;
        h->slots.broken = h->h_broken.get();
        h->slots.broken_count = h->h_broken.get() + LaunchSlots::N;
        GX_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->d_broken), h->h_broken.get(), 0));
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) == hipSuccess && cus > 0) h->num_cus = cus;
        // the resident one-line service (gx_service.hip)
        if ((h->create_flags & GX_CREATE_RESIDENT_ONE) && plan_service(I, &h->svc.L)) {
            gx_handle::Service& sv = h->svc;
            sv.mode = T.has_capture ? 1 : 0;
            const size_t dwords = 17 * 16 + 80 + 16;
            GX_HIP(hipHostMalloc(sv.host.out(), dwords * 4, hipHostMallocMapped));
            memset(sv.host.get(), 0, dwords * 4);
            GX_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&sv.dev), sv.host.get(), 0));
            GX_HIP(hipStreamCreateWithFlags(sv.stream.out(), hipStreamNonBlocking));
            sv.enabled = true;
        }
    }
    h->on_device = true;
}

// One batch on the device: tile kernel (LDS tier when the tables fit LDS, else L2 tier), slice kernel for long lines,
// per-line kernel otherwise.  kernel: gx_batch_opts.kernel (0 = choose).
// What a launch leaves for its caller: where a broken max_line_bytes promise would show, and how to make good for it.
struct Launched {
    int slot = -1;
    uint32_t seq = 0;
    bool promised = false;     // no follow-up launch: the caller said that no line is longer than the kernel takes
    uint32_t limit = 0;        // launch_extract_oversize's arguments for this launch
    int by_length = 0;
};

// The launch's flag word (and the lane kernel's chunk counter): the slot of its stream.  Call under h->slot_mu.
LaunchSlots::Use take_slot(gx_handle* h, GxBatch& b, hipStream_t stream) {
    const LaunchSlots::Use u = h->slots.take(stream);
    b.seq = u.seq;
    if (u.wait_shared) GX_HIP(hipStreamWaitEvent(stream, h->shared_event.get(), 0));
    // batches of this stream that promised their longest line, ran without a follow-up launch and met a longer line after all
    // (no_sync batches: nobody has looked yet; one that is still queued shows to a later call)
    if (h->slots.consume_broken(u.slot))
        throw GxError(GX_E_ARG, "an earlier no_sync batch on this stream held a line longer than its gx_batch_opts.max_line_bytes: that line was not "
                                "processed (its result row is unwritten); this batch was not launched");
    b.oversize_flag = h->d_slots.get() + u.slot;
    DevMem<uint32_t>& steal = h->d_steal[u.slot];
    if (!steal) {   // (the slot's first launch: 768 KB, zeroed once -- every launch leaves the next one's row zeroed)
        const size_t bytes = 2 * static_cast<size_t>(GX_STEAL_MAX) * GX_STEAL_STRIDE * sizeof(uint32_t);
        GX_HIP(hipMalloc(steal.out(), bytes));
        GX_HIP(hipMemsetAsync(steal.get(), 0, bytes, stream));   // (on the launch's own stream: in order before its kernel; the shared slot's later users wait for its event)
    }
    b.steal = steal.get();
    b.steal_parity = h->slots.steal_parity[u.slot];
    return u;
}
// The follow-up launch for the lines the batch kernel leaves (longer than `limit`: see launch_extract_oversize) -- unless the
// caller promised that there are none (b.max_line_bytes within `fits`), or the host knows (b.no_followup: the one-line calls).
// Call before the batch kernel is launched; returns what to launch after it.
bool plan_followup(gx_handle* h, GxBatch& b, const LaunchSlots::Use& u, uint32_t fits, Launched* out) {
    if (out) { out->slot = u.slot; out->seq = b.seq; }
    if (b.no_followup) return false;
    if (b.max_line_bytes != 0 && b.max_line_bytes <= fits) {
        b.no_followup = 1;
        b.oversize_flag = h->d_broken + u.slot;
        if (out) out->promised = true;
        return false;
    }
    return true;
}
// Has any batch of this stream's slot -- the caller's own or one before it -- broken its promise since the host last accounted for
// the slot?  Accounts for all of them.  (For a call that waits for its batch itself and has no way to make good: the count is final
// once the stream is idle.  A call that can make good asks LaunchSlots::finished, which tells its own break from an earlier one.)
bool promise_broken_since(gx_handle* h, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(h->slot_mu);
    return h->slots.consume_broken(h->slots.slot_of(stream)) != 0;
}
void done_slot(gx_handle* h, const LaunchSlots::Use& u, hipStream_t stream) {
    if (u.shared) GX_HIP(hipEventRecord(h->shared_event.get(), stream));
}

// Stream-ordered memory out of the handle's own pool (gx_handle::pool) for the length of a scope: freed on the stream when the scope
// ends -- by a return or by an exception (take_slot and plan_followup throw).
struct PoolBuffer {
    void* p = nullptr;
    hipStream_t s;
    PoolBuffer(gx_handle* h, size_t bytes, hipStream_t stream) : s(stream) {
        {
            std::lock_guard<std::mutex> pool_lock(h->slot_mu);   // (device-pointer batches of several threads come here without h->mu)
            if (!h->pool) {
                hipMemPoolProps props{};
                props.allocType = hipMemAllocationTypePinned;
                props.handleTypes = hipMemHandleTypeNone;
                props.location.type = hipMemLocationTypeDevice;
                props.location.id = h->device;
                GX_HIP(hipMemPoolCreate(h->pool.out(), &props));
                uint64_t keep = ~0ull;
                GX_HIP(hipMemPoolSetAttribute(h->pool.get(), hipMemPoolAttrReleaseThreshold, &keep));
            }
        }
        GX_HIP(hipMallocFromPoolAsync(&p, bytes, h->pool.get(), stream));
    }
    ~PoolBuffer() { if (p) (void)hipFreeAsync(p, s); }
    PoolBuffer(const PoolBuffer&) = delete;
    PoolBuffer& operator=(const PoolBuffer&) = delete;
};

// Launches of a handle that runs an extraction's program as it is take their turns across streams: the thread lists are the handle's.
struct PikeGate {
    gx_handle* h;
    hipStream_t s;
    bool on;
    PikeGate(gx_handle* h_, hipStream_t s_) : h(h_), s(s_), on(h_->T.has_pike()) {
        if (!on) return;
        h->pike_mu.lock();
        if (h->pike_depth++ == 0 && h->pike_event_set) (void)hipStreamWaitEvent(s, h->pike_event.get(), 0);
    }
    ~PikeGate() {
        if (!on) return;
        if (--h->pike_depth == 0) {
            if (!h->pike_event) (void)hipEventCreateWithFlags(h->pike_event.out(), hipEventDisableTiming);
            if (h->pike_event && hipEventRecord(h->pike_event.get(), s) == hipSuccess) h->pike_event_set = true;
        }
        h->pike_mu.unlock();
    }
    PikeGate(const PikeGate&) = delete;
    PikeGate& operator=(const PikeGate&) = delete;
};

void launch_batch(gx_handle* h, GxBatch b, uint32_t line_bytes_hint, uint32_t kernel, hipStream_t stream, bool uneven = false, Launched* launched = nullptr) {
    PikeGate pike_gate(h, stream);
    const BatchShape shape{b.wide != 0, b.state_out != nullptr, b.match_only, b.packed != nullptr, b.n, line_bytes_hint, uneven, kernel};
    const BatchPlan p = plan_batch(h->tiles, shape, h->num_cus);
    if (p.narrow) {
        // UTF-16 code units: their low bytes through the byte kernels, then the lines that hold a unit above 0xFF again through
        // the per-line walk (gx_kernels.hip: k_narrow_units).  The copy is n units long -- the one thing this path has to
        // know on the host, so it reads the two ends of the offsets (a small synchronous copy) -- and lives in
        // stream-ordered memory for the length of the call.
        if (b.caller_no_sync)
            throw GxError(GX_E_ARG, "gx_batch_opts.utf16 with no_sync: this batch would take the narrowed copy of its code units (tables other than dense rows "
                                    "in LDS or hop tables, or a kernel named in gx_batch_opts.kernel), which is sized by a read of the offsets on the host; "
                                    "call it without no_sync");
        const auto [first, last] = device_offset_ends(b.offsets, b.n, b.offsets64 != 0, stream);
        const uint64_t units = last >= first ? last - first : 0;
        PoolBuffer tmp_buf(h, units + b.n + 64, stream);
        uint8_t* bytes = static_cast<uint8_t*>(tmp_buf.p);
        uint8_t* flags = bytes + ((units + 15) & ~15ull);
        hipError_t e = launch_narrow_units(b, bytes, flags, stream);
        if (e == hipSuccess) {
            GxBatch nb = b;
            nb.wide = 0;
            nb.max_line_bytes = 0;     // (the copy does not outlive this call: its follow-up launch always runs)
            nb.data = bytes - first;   // (addressed like the units: line i at data + offsets[i])
            launch_batch(h, nb, line_bytes_hint, kernel, stream, uneven, launched);
            e = launch_extract_flagged(h->dev, b, flags, stream);
        }
        GX_HIP(e);
        return;
    }
    const uint8_t* image = p.image >= 0 ? static_cast<const uint8_t*>(h->d_img[p.image].get()) : nullptr;
    const uint8_t* at_global = p.global >= 0 ? static_cast<const uint8_t*>(h->d_img[p.global].get()) : nullptr;
    if (p.kernel == GX_KERNEL_PER_LINE || p.kernel == GX_KERNEL_SLICES) {   // (no slot: these take every line themselves)
        h->last_kernel = p.kernel;
        h->last_fits = 0, h->last_limit = 0;
        if (p.kernel == GX_KERNEL_SLICES) GX_HIP(launch_extract_slices(h->dev, p.L, image, at_global, h->num_cus, b, stream));
        else GX_HIP(launch_extract_generic(h->dev, b, stream));
        return;
    }
    // UTF-16 code units read by the batch kernel itself: the lines that hold a unit above 0xFF are flagged for the per-line walk.
    // (Taken before slot_mu, which PoolBuffer locks itself; given back to the pool when this scope ends, whatever ends it.)
    std::optional<PoolBuffer> flags;
    if (b.wide) flags.emplace(h, b.n + 64, stream);
    hipError_t e = hipSuccess;
    {
        // a slot for the "lines I could not stage" word of this launch, free again once its follow-up kernel has run
        // (submission of slot launches is serialised per handle; the launches themselves are asynchronous)
        std::lock_guard<std::mutex> lock(h->slot_mu);
        const LaunchSlots::Use u = take_slot(h, b, stream);
        const bool followup = plan_followup(h, b, u, p.fits, launched);
        if (launched) { launched->limit = p.limit; launched->by_length = p.by_length; }
        if (b.wide) {
            b.wide_flags = static_cast<uint8_t*>(flags->p);
            b.wide_any = h->d_slots.get() + 3 * LaunchSlots::N + u.slot;
        }
        // (the pool of chunks the launch's waves share: the slot's chunk counter -- the hop slice kernel, the lane kernel's sorted tiles)
        const bool chunks = p.kernel == GX_KERNEL_HOP_SLICES || (p.kernel == GX_KERNEL_LANES && p.L.sort_chunk);
        if (chunks) {
            b.chunk_ctr = h->d_slots.get() + 2 * LaunchSlots::N + u.slot;
            b.chunk_base = h->slots.chunk_tickets[u.slot];
        }
        unsigned long long* stamps = nullptr;
#ifdef GX_DEV
        if (!b.wide) stamps = h->dev_stamps;
#endif
        h->last_kernel = p.kernel;
        h->last_fits = p.fits, h->last_limit = p.limit;
        if (p.kernel == GX_KERNEL_TILES || p.kernel == GX_KERNEL_HOPS) {
            e = launch_extract_tile(h->dev, p.L, image, at_global, h->num_cus, b, stream, stamps);
            if (e == hipSuccess) h->slots.steal_parity[u.slot] ^= 1u;
        } else if (p.kernel == GX_KERNEL_HOP_SLICES) {
            e = launch_extract_hop_slices(h->dev, p.L, image, at_global, h->num_cus, b, stream, stamps);
            if (e == hipSuccess) h->slots.chunk_tickets[u.slot] += hop_slices_tickets(b.n, p.L.nwaves, h->num_cus);   // (what the launch will draw)
        } else {
            e = launch_extract_lanes(h->dev, p.L, image, at_global, h->num_cus, b, stream, stamps);
            if (e == hipSuccess && chunks) h->slots.chunk_tickets[u.slot] += lanes_sorted_tickets(b.n, p.L.sort_chunk, h->num_cus);
        }
        if (e == hipSuccess && b.wide) e = launch_extract_flagged(h->dev, b, static_cast<const uint8_t*>(flags->p), stream, b.wide_any);
        if (e == hipSuccess && followup) e = launch_extract_oversize(h->dev, b, p.limit, p.by_length, stream);
        if (e == hipSuccess) done_slot(h, u, stream);
    }
    GX_HIP(e);
}

// A batch on device buffers as the call that enqueued it leaves it for the call that waits for it.
struct DeviceBatch {
    GxBatch b{};
    Launched done;
    hipStream_t stream = nullptr;
    bool enqueued = false;
};

// Waits for the batch, makes good for its own broken max_line_bytes promise (the follow-up launch it went without, now: the lines the
// batch kernel left and nothing else, so *overflow counts every line once), and reports a promise that a batch BEFORE it on the
// stream broke -- one that nobody waited for: its rows stay unwritten (LaunchSlots::finished tells the two apart).
void finish_device_batch(gx_handle* h, DeviceBatch& d) {
    GX_HIP(hipStreamSynchronize(d.stream));
    LaunchSlots::Verdict v;
    {
        std::lock_guard<std::mutex> lock(h->slot_mu);
        // (a launch of a kernel that leaves no line has no slot: the one its stream owns, for what came before it -- a stream that
        // owns none has had no launch that could break a promise, and the shared slot's reports are not this call's to take)
        const int slot = d.done.slot >= 0 ? d.done.slot : h->slots.slot_of(d.stream);
        if (d.done.slot >= 0 || slot != LaunchSlots::N - 1) v = h->slots.finished(slot, d.done.seq, d.done.slot >= 0 && d.done.promised);
        else v = LaunchSlots::Verdict{false, false};
    }
    if (v.mine) {
        d.b.seq = d.done.seq;
        d.b.oversize_flag = h->d_broken + d.done.slot;   // (it holds d.done.seq: the follow-up's waves stay)
        PikeGate pike_gate(h, d.stream);
        GX_HIP(launch_extract_oversize(h->dev, d.b, d.done.limit, d.done.by_length, d.stream));
        GX_HIP(hipStreamSynchronize(d.stream));
    }
    if (v.earlier)
        throw GxError(GX_E_ARG, "an earlier no_sync batch on this stream held a line longer than its gx_batch_opts.max_line_bytes: that line was not "
                                "processed (its result row is unwritten); this batch itself is complete");
}

// gx_batch_opts.utf8: the fix-up behind a byte batch whose lines are UTF-8 (gx_utf8.hip).  The byte kernels' rows are right for every
// ASCII-only line; the lines that hold a byte >= 0x80 (line_flags: the caller's, from gx_split_lines; nullptr: a sweep finds them) are
// transcoded to the UTF-16 code units of the String Java would see, walked again on those (k_extract_listed, the per-line walk over the list of flagged lines the count pass leaves, overwrites their rows),
// and -- mode 1 -- their capture offsets taken back to bytes.  ONE synchronisation, where the host reads "flagged lines, their units":
// it sizes the units' memory, and with no flagged line everything behind it is skipped.  Call when nothing else will write the rows
// any more (behind finish_device_batch).
void utf8_fixup(gx_handle* h, const GxBatch& b, uint32_t mode, const uint8_t* line_flags, hipStream_t stream) {
    h->last_utf8_lines = 0;
    h->last_utf8_units = 0;
    if (b.n == 0) return;
    const uint8_t* data = static_cast<const uint8_t*>(b.data);
    PoolBuffer ws_buf(h, utf8_workspace_bytes(b.n), stream);
    const Utf8Ws w = utf8_workspace(ws_buf.p, b.n);
    const uint8_t* flags = line_flags;
    if (!flags) {
        GX_HIP(launch_utf8_flags(data, b.offsets, b.offsets64, b.n, w.flags, stream));
        flags = w.flags;
    }
    GX_HIP(launch_utf8_count(data, b.offsets, b.offsets64, b.n, flags, w, stream));
    uint64_t units = 0;
    uint64_t lines_status[2] = {0, 0};   // (neighbours in the workspace)
    GX_HIP(hipMemcpyAsync(&units, w.unit_off + b.n, 8, hipMemcpyDeviceToHost, stream));
    GX_HIP(hipMemcpyAsync(lines_status, w.flagged, 16, hipMemcpyDeviceToHost, stream));
    GX_HIP(hipStreamSynchronize(stream));
    if (lines_status[1] & 0xFFFFFFFFull) throw GxError(GX_E_LIMIT, "gx_batch_opts.utf8: a line of 4 G code units or more");
    h->last_utf8_lines = lines_status[0];
    h->last_utf8_units = units;
    if (lines_status[0] == 0) return;
    const bool to_bytes = mode == 1 && !b.match_only;
    const size_t units_bytes = (static_cast<size_t>(units) * 2 + 64 + 15) & ~static_cast<size_t>(15);
    PoolBuffer units_buf(h, units_bytes + (to_bytes ? static_cast<size_t>(units) * 4 + 16 : 0), stream);
    uint16_t* d_units = static_cast<uint16_t*>(units_buf.p);
    uint32_t* d_unit_byte = to_bytes ? reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(units_buf.p) + units_bytes) : nullptr;
    GX_HIP(launch_utf8_write(data, b.offsets, b.offsets64, b.n, flags, w.unit_off, d_units, d_unit_byte, stream));
    GxBatch ub = b;   // the same lines and rows, on the units
    ub.data = d_units;
    ub.offsets = w.unit_off;
    ub.offsets64 = 1;
    ub.wide = 1;
    {
        PikeGate pike_gate(h, stream);
        GX_HIP(launch_extract_listed(h->dev, ub, w.list, lines_status[0], stream));   // (a lane per flagged line: few among many fill their waves)
    }
    if (to_bytes) GX_HIP(launch_utf8_offsets_to_bytes(h->dev, b, flags, w.unit_off, d_unit_byte, stream));
}

int finish_create(std::unique_ptr<gx_handle>& h, uint32_t flags, gx_handle** out) {
    h->create_flags = flags;
    h->blob = pack_blob(h->T);
    if (!(flags & GX_CREATE_HOST_ONLY)) upload(h.get());
    else h->tiles = choose_tile_images(h->T, flags);
    *out = h.release();
    return GX_OK;
}

// gx_split_lines has no handle to keep its workspace on (an eighth of the text since the text-read-once split: an allocation and a free
// of 250 MB per call were 0.1 ms of a 0.7 ms call): one workspace per device, kept between calls, grown as needed; a call holds the
// lock OF ITS DEVICE while it runs (calls on one device take turns: they would on the device anyway; calls on different devices -- one
// process, eight GPUs -- do not wait for each other).  gx_release_scratch(device) gives a device's workspace back.
struct SplitScratch {
    std::mutex mu[64];
    GrowBuf ws[64];
};
SplitScratch& g_split_scratch = *new SplitScratch;   // (never destroyed: the HIP runtime may be gone when static destructors run)
SplitScratch& g_utf8_scratch = *new SplitScratch;    // gx_utf8_to_utf16's, kept the same way (gx_device.hpp: Utf8Ws)

// Accepts the current gx_batch_opts and every earlier, shorter layout of it (struct_size says which).
gx_batch_opts read_opts(const gx_batch_opts* opts) {
    gx_batch_opts o{};
    if (!opts) return o;
    const size_t v1 = offsetof(gx_batch_opts, strip_eol);  // the first layout; later ones only appended fields
    if (opts->struct_size < v1 || opts->struct_size > sizeof(gx_batch_opts) || (opts->struct_size & 3u))
        throw GxError(GX_E_ARG, "gx_batch_opts.struct_size mismatch");
    memcpy(&o, opts, opts->struct_size);
    // utf8 lies in what was the tail padding of the layout that ended with max_line_bytes: a caller compiled against that layout
    // copies those four bytes in uninitialised
    if (opts->struct_size <= offsetof(gx_batch_opts, utf8) + sizeof(uint32_t)) { o.utf8 = 0; o.utf8_line_flags = nullptr; }
    if (o.utf8 > 2) throw GxError(GX_E_ARG, "gx_batch_opts.utf8: 0, 1 (capture offsets in bytes) or 2 (in UTF-16 code units)");
    return o;
}

}  // namespace

extern "C" {

const char* gx_last_error(void) { return g_last_error.c_str(); }

int gx_release_scratch(int device) {
    DeviceScope scope;
    if (hipSetDevice(device) != hipSuccess) {
        (void)hipGetLastError();   // (the runtime keeps the error for the next hipGetLastError(): a later launch's check would see it)
        return fail(GX_E_DEVICE, "gx_release_scratch: no such device");
    }
    if (device >= 0 && device < 64) {
        std::lock_guard<std::mutex> lock(g_split_scratch.mu[device]);
        g_split_scratch.ws[device] = {};
    }
    if (device >= 0 && device < 64) {
        std::lock_guard<std::mutex> lock(g_utf8_scratch.mu[device]);
        g_utf8_scratch.ws[device] = {};
    }
    return GX_OK;
}

int gx_device_count(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return 0;
    return count;
}

int gx_create_from_patterns(const char* const* automaton_rx, const char* const* jdk_rx, int32_t n, uint32_t flags,
                            gx_handle** out) {
    if (!automaton_rx || !out || n <= 0) return fail(GX_E_ARG, "gx_create_from_patterns: bad argument");
    return guarded([&]() -> int {
        std::vector<ustr> a, j;
        for (int32_t i = 0; i < n; ++i) {
            if (!automaton_rx[i] || (jdk_rx && !jdk_rx[i])) return fail(GX_E_ARG, "gx_create_from_patterns: null pattern");
            a.push_back(utf8_to_u16(automaton_rx[i]));
            if (jdk_rx) j.push_back(utf8_to_u16(jdk_rx[i]));
        }
        std::unique_ptr<gx_handle> h(new gx_handle());
        h->T = compile_tables(a, jdk_rx ? &j : nullptr, (flags & GX_CREATE_PROGRAMS) != 0);
        return finish_create(h, flags, out);
    });
}

int gx_create_from_blob(const void* blob, size_t size, uint32_t flags, gx_handle** out) {
    if (!blob || !out) return fail(GX_E_ARG, "gx_create_from_blob: bad argument");
    return guarded([&]() -> int {
        std::unique_ptr<gx_handle> h(new gx_handle());
        h->T = unpack_blob(blob, size);
        return finish_create(h, flags, out);
    });
}

size_t gx_blob_size(const gx_handle* h) { return h ? h->blob.size() : 0; }

int gx_blob_copy(const gx_handle* h, void* dst, size_t cap) {
    if (!h || !dst || cap < h->blob.size()) return fail(GX_E_ARG, "gx_blob_copy: bad argument");
    memcpy(dst, h->blob.data(), h->blob.size());
    return GX_OK;
}

void gx_destroy(gx_handle* h) {
    if (!h) return;
    if (h->svc.started) {   // the resident wave reads the dense image and the mailbox: tell it to leave, wait for it, before they go
        uint32_t* mb = h->svc.host.get();
        __atomic_store_n(&mb[1], (mb[1] & 0xFFFFu) | 0x10000u, __ATOMIC_RELEASE);
        (void)hipStreamSynchronize(h->svc.stream.get());
    }
    delete h;
}

int32_t gx_num_extractions(const gx_handle* h) { return h ? h->T.n_rules : 0; }
int32_t gx_num_groups(const gx_handle* h, int32_t k) {
    if (!h || k < 0 || k >= static_cast<int32_t>(h->T.rules.size())) return 0;
    return h->T.rules[k].n_groups;
}
int32_t gx_max_groups(const gx_handle* h) { return h ? h->T.max_groups : 0; }

int64_t gx_stat(const gx_handle* h, int32_t which) {
    if (!h) return -1;
    const TileImages& I = h->tiles;
    const HopImage& H = I.hop[0].img;
    switch (which) {
    case 0: return h->T.m_states;
    case 1: return h->T.ncls;
    case 2: { int64_t s = 0; for (auto& r : h->T.rules) s += r.n_states; return s; }
    case 3: { int64_t m = 0; for (auto& r : h->T.rules) m = std::max<int64_t>(m, r.n_regs); return m; }
    case 4: return static_cast<int64_t>(h->blob.size());
    case 5: { GxLds L; return plan_tile_launch(I, 0, &L) ? static_cast<int64_t>(L.total_bytes) : 0; }
    case 6: { GxLds L; return plan_tile_launch(I, 0, &L) ? static_cast<int64_t>(L.nwaves) : 0; }
    case 7: return !I.tile_ok ? 0 : I.dense[0].L.tier == 3 ? 4 : I.tile_global ? 2 : I.dense[0].L.tier == 2 ? 3 : 1;
    case 8: return h->T.has_capture ? 1 : 0;
    case 10: { GxLds L; return plan_lanes_launch(I, &L, false, true) ? static_cast<int64_t>(L.nwaves) : 0; }   // lane kernel: waves per CU, compact rows
    case 11: { GxLds L; return plan_lanes_launch(I, &L, true, false) ? static_cast<int64_t>(L.nwaves) : 0; }   // ... match-only
    case 12: return I.tile_ok ? static_cast<int64_t>(I.dense[0].L.table_bytes) : 0;
    case 13: return I.tile_ok ? static_cast<int64_t>(I.dense[0].L.regs_wave_bytes) : 0;
    case 14: return I.hop[0].ok ? static_cast<int64_t>(H.n_states) : 0;         // hop tier: states (0: no hop image)
    case 15: return I.hop[0].ok ? static_cast<int64_t>(H.full.n_hot) : 0;       // ... whose records live in LDS (tile kernel)
    case 21: return I.hop[0].ok ? static_cast<int64_t>(H.small.n_hot) : 0;      // ... (hop slice kernel)
    case 16: return I.hop[0].ok ? static_cast<int64_t>(H.n_reachable_hot) : 0;  // ... that well-formed lines reach
    case 17: return I.hop[0].ok ? static_cast<int64_t>(H.n_chains) : 0;         // ... that have a chain
    case 18: { GxLds L; return plan_hop_launch(I, 0, &L) ? static_cast<int64_t>(L.nwaves) : 0; }  // hop tier: waves per CU
    case 20: return I.hop[0].ok ? static_cast<int64_t>(H.full.n_lds_rows) : 0;       // ... whose dense row is in LDS too (branching states)
    case 22: return I.hop[1].ok ? static_cast<int64_t>(I.hop[1].img.n_states) : 0;   // hop tier of the match automaton alone (match-only batches): states
    case 24: return static_cast<int64_t>(h->slots.promises_broken.load());
    case 30: return static_cast<int64_t>(h->peer_image_bytes);   // table bytes copied from another handle's device (gx_create_on_devices)
    case 25: return h->last_kernel.load();
    case 31: return h->last_fits.load();
    case 32: return h->last_limit.load();
    case 33: return static_cast<int64_t>(h->last_utf8_lines.load());
    case 34: return static_cast<int64_t>(h->last_utf8_units.load());
    case 26: return I.hop_reason;
    case 28: return static_cast<int64_t>(h->svc.enabled ? h->svc.launches : -1);
    case 27: { int64_t c = 0; for (auto& r : h->T.rules) c += r.pike ? 1 : 0; return c; }
    case 35: {   // workgroups a per-line launch is kept within: GxDev::pike_blocks (a host-only handle: what it would be)
        if (!h->T.has_pike()) return -1;
        uint32_t lane_ints = 0, blocks = 0;
        pike_sizing(h->T, &lane_ints, &blocks);
        return static_cast<int64_t>(blocks);
    }
    case 23: return I.hop[1].ok ? static_cast<int64_t>(I.hop[1].img.full.n_hot) : 0; // ... whose records are in LDS
    case 19: { GxLds L; return plan_hop_slice_launch(I, &L) ? static_cast<int64_t>(L.nwaves) : 0; }  // ... of the hop slice kernel
    case 9: return !I.tile_ok ? 0 : !I.has_mo ? gx_stat(h, 7) : I.dense[1].L.tier == 3 ? 4 : I.dense[1].L.tier == 2 ? 3 : I.dense[1].L.tier == 1 ? 2 : 1;
    // what the table images were built from (read-only, for tests that must know how near an image is to a limit of its format)
    case 36: return I.tile_ok ? static_cast<int64_t>(I.dense[0].records) : 0;                    // range records of the batch image (0: dense rows)
    case 37: return I.tile_ok ? static_cast<int64_t>(I.dense[I.dense_of(true)].records) : 0;     // ... of the image match-only batches walk
    case 38: return I.tile_ok ? static_cast<int64_t>(I.dense[0].rows) : 0;                       // automaton rows (states) the batch image covers
    case 39: return I.tile_ok && I.dense[0].fused ? 1 : 0;                                       // 1: its capture side is the fused automaton
    default: return -1;
    }
}

int gx_split_lines(const uint8_t* bytes, uint64_t size, void* offsets, uint64_t cap_lines, uint64_t* n_lines, uint8_t* line_flags,
                   const gx_batch_opts* opts) {
    return gx_split_lines_max(bytes, size, offsets, cap_lines, n_lines, line_flags, nullptr, opts);
}

int gx_split_lines_max(const uint8_t* bytes, uint64_t size, void* offsets, uint64_t cap_lines, uint64_t* n_lines, uint8_t* line_flags,
                       uint64_t* max_line_bytes, const gx_batch_opts* opts) {
    return guarded([&]() -> int {
        if (!offsets || !n_lines || (size && !bytes)) return fail(GX_E_ARG, "gx_split_lines: bad argument");
        const gx_batch_opts o = read_opts(opts);
        if (!o.offsets64 && size > 0xFFFFFFFFull) return fail(GX_E_ARG, "gx_split_lines: buffers of 4 GiB and more need offsets64");
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
            throw GxError(GX_E_DEVICE, "no HIP device available (libgorp_hip needs a gfx950 GPU; there is no CPU fallback)");
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        const size_t off_w = o.offsets64 ? 8 : 4;
        DevMem<> d_bytes, d_off;
        DevMem<uint8_t> d_flags;
        int dev = 0;
        GX_HIP(hipGetDevice(&dev));
        if (dev < 0 || dev >= 64) return fail(GX_E_DEVICE, "gx_split_lines: device ordinal beyond 63");
        std::lock_guard<std::mutex> ws_lock(g_split_scratch.mu[dev]);
        void* ws = g_split_scratch.ws[dev].get(split_workspace_bytes(size, line_flags != nullptr));
        const uint8_t* src = bytes;
        void* dst_off = offsets;
        uint8_t* dst_flags = line_flags;
        if (o.device_pointers) {
            if (reinterpret_cast<uintptr_t>(bytes) & 15u) return fail(GX_E_ARG, "gx_split_lines: device buffer must be 16-byte aligned");
        } else {
            d_bytes = dev_alloc(size);
            d_off = dev_alloc((cap_lines + 1) * off_w);
            if (line_flags) d_flags = dev_alloc<uint8_t>(cap_lines);
            if (size) GX_HIP(hipMemcpyAsync(d_bytes.get(), bytes, size, hipMemcpyHostToDevice, stream));
            src = static_cast<const uint8_t*>(d_bytes.get());
            dst_off = d_off.get();
            dst_flags = d_flags.get();
        }
        uint64_t* d_n = nullptr;
        uint64_t* d_max = nullptr;
        GX_HIP(launch_split_lines(src, size, dst_off, o.offsets64 ? 1 : 0, cap_lines, dst_flags, ws, &d_n, stream, max_line_bytes ? &d_max : nullptr));
        uint64_t n_and_max[2] = {0, 0};   // (n_lines and max_line are neighbours in the workspace)
        GX_HIP(hipMemcpyAsync(n_and_max, d_n, max_line_bytes ? 16 : 8, hipMemcpyDeviceToHost, stream));
        GX_HIP(hipStreamSynchronize(stream));
        const uint64_t n = n_and_max[0];
        *n_lines = n;
        if (max_line_bytes) *max_line_bytes = n_and_max[1];
        if (n > cap_lines) return fail(GX_E_LIMIT, "gx_split_lines: the buffer holds more lines than cap_lines");
        if (!o.device_pointers) {
            GX_HIP(hipMemcpy(offsets, d_off.get(), (n + 1) * off_w, hipMemcpyDeviceToHost));
            if (line_flags && n) GX_HIP(hipMemcpy(line_flags, d_flags.get(), n, hipMemcpyDeviceToHost));
        }
        return GX_OK;
    });
}

int gx_utf8_to_utf16(const uint8_t* bytes, const void* offsets, uint64_t n, uint16_t* units, uint64_t units_cap, void* unit_offsets,
                     uint64_t* n_units, const gx_batch_opts* opts) {
    return guarded([&]() -> int {
        if (!offsets || !n_units || (units && !unit_offsets)) return fail(GX_E_ARG, "gx_utf8_to_utf16: bad argument");
        *n_units = 0;
        const gx_batch_opts o = read_opts(opts);
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
            throw GxError(GX_E_DEVICE, "no HIP device available (libgorp_hip needs a gfx950 GPU; there is no CPU fallback)");
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        const size_t off_w = o.offsets64 ? 8 : 4;
        int dev = 0;
        GX_HIP(hipGetDevice(&dev));
        if (dev < 0 || dev >= 64) return fail(GX_E_DEVICE, "gx_utf8_to_utf16: device ordinal beyond 63");
        std::lock_guard<std::mutex> ws_lock(g_utf8_scratch.mu[dev]);
        const Utf8Ws w = utf8_workspace(g_utf8_scratch.ws[dev].get(utf8_workspace_bytes(n)), n);
        const bool host = !o.device_pointers;
        DevMem<uint8_t> d_bytes;
        DevMem<> d_off, d_units, d_uoff;
        const uint8_t* data = bytes;
        const void* src_off = offsets;
        if (host) {
            const HostOffsets off{offsets, o.offsets64 != 0, n};
            const uint64_t first = off[0], total = off[n] - first;
            if (total && !bytes) return fail(GX_E_ARG, "gx_utf8_to_utf16: bytes is NULL");
            d_bytes = dev_alloc<uint8_t>(total + 32);
            d_off = dev_alloc((n + 1) * off_w);
            if (total) GX_HIP(hipMemcpyAsync(d_bytes.get() + 16, bytes + first, total, hipMemcpyHostToDevice, stream));
            GX_HIP(hipMemcpyAsync(d_off.get(), offsets, (n + 1) * off_w, hipMemcpyHostToDevice, stream));
            // (line i at data + offsets[i], as in the caller's buffer; the base may lie below the allocation: made as an integer)
            data = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(d_bytes.get()) + 16u - static_cast<uintptr_t>(first));
            src_off = d_off.get();
        }
        // the count / scan / write passes of the utf8 fix-up with every line flagged
        GX_HIP(launch_utf8_count(data, src_off, o.offsets64 ? 1 : 0, n, nullptr, w, stream));
        uint64_t total_units = 0;
        uint64_t lines_status[2] = {0, 0};
        GX_HIP(hipMemcpyAsync(&total_units, w.unit_off + n, 8, hipMemcpyDeviceToHost, stream));
        GX_HIP(hipMemcpyAsync(lines_status, w.flagged, 16, hipMemcpyDeviceToHost, stream));
        GX_HIP(hipStreamSynchronize(stream));
        *n_units = total_units;
        if (lines_status[1] & 0xFFFFFFFFull) return fail(GX_E_LIMIT, "gx_utf8_to_utf16: a line of 4 G code units or more");
        if (!o.offsets64 && total_units > 0xFFFFFFFFull) return fail(GX_E_LIMIT, "gx_utf8_to_utf16: 4 G code units and more need offsets64");
        if (!units) return GX_OK;   // size query
        if (total_units > units_cap) return fail(GX_E_LIMIT, "gx_utf8_to_utf16: units_cap is smaller than the text (see *n_units)");
        uint16_t* dst = units;
        void* dst_off = unit_offsets;
        if (host) {
            d_units = dev_alloc(total_units * 2);
            dst = static_cast<uint16_t*>(d_units.get());
            if (!o.offsets64) { d_uoff = dev_alloc((n + 1) * 4); dst_off = d_uoff.get(); }
        }
        GX_HIP(launch_utf8_write(data, src_off, o.offsets64 ? 1 : 0, n, nullptr, w.unit_off, dst, nullptr, stream));
        if (o.offsets64) GX_HIP(hipMemcpyAsync(unit_offsets, w.unit_off, (n + 1) * 8, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, stream));
        else GX_HIP(launch_utf8_offsets32(w.unit_off, n, static_cast<uint32_t*>(dst_off), stream));
        if (host) {
            if (total_units) GX_HIP(hipMemcpyAsync(units, dst, total_units * 2, hipMemcpyDeviceToHost, stream));
            if (!o.offsets64) GX_HIP(hipMemcpyAsync(unit_offsets, dst_off, (n + 1) * 4, hipMemcpyDeviceToHost, stream));
        }
        GX_HIP(hipStreamSynchronize(stream));
        return GX_OK;
    });
}

// One JSON template per extraction for ExtractionResult.asMap(idAs) (core/ExtractionResult.java:65-88), uploaded once
// per distinct id_as.
static const GxJsonl& jsonl_templates(gx_handle* h, const char* id_as) {
    const std::string key = id_as ? std::string("1") + id_as : std::string("0");
    auto it = h->jsonl.find(key);
    if (it != h->jsonl.end()) return it->second.dev;
    const Tables& T = h->T;
    if (static_cast<int>(h->meta.size()) != T.n_rules)
        throw GxError(GX_E_ARG, "extraction names are unknown: create the handle with gx_create_from_definition or call "
                                "gx_set_extraction_meta for every extraction");
    std::vector<uint32_t> seg_off(1, 0), lit_off, lit_len, fixed_len;
    std::vector<int32_t> group;
    std::vector<uint8_t> lits;
    for (int k = 0; k < T.n_rules; ++k) {
        const dsl::Extraction& x = h->meta[k];
        if (static_cast<int>(x.extractor_names.size()) != T.rules[k].n_groups)
            throw GxError(GX_E_ARG, "extractor names of extraction '" + x.name + "' do not match its capture groups");
        // LinkedHashMap: a key put again keeps its position and takes the new value
        struct Entry { std::string key; int g; std::string raw; };
        std::vector<Entry> entries;
        auto put = [&](const std::string& key_utf8, int g, const std::string& raw) {
            for (auto& e : entries) if (e.key == key_utf8) { e.g = g; e.raw = raw; return; }
            entries.push_back({key_utf8, g, raw});
        };
        if (id_as) put(id_as, -1, dsl::json_quote(x.name));
        for (size_t g = 0; g < x.extractor_names.size(); ++g) put(x.extractor_names[g], static_cast<int>(g), "");
        if (!x.append_json.empty())
            for (auto& kv : dsl::json_object_entries(x.append_json)) put(kv.first, -1, kv.second);
        std::string lit = "{";
        uint32_t fixed = 0;
        auto close_segment = [&](int g) {
            while (lits.size() % 4) lits.push_back(0);  // the write kernel reads literals as aligned 32-bit words
            lit_off.push_back(static_cast<uint32_t>(lits.size()));
            lit_len.push_back(static_cast<uint32_t>(lit.size()));
            group.push_back(g);
            lits.insert(lits.end(), lit.begin(), lit.end());
            fixed += static_cast<uint32_t>(lit.size());
            lit.clear();
        };
        for (size_t e = 0; e < entries.size(); ++e) {
            lit += (e ? "," : "") + dsl::json_quote(entries[e].key) + ":";
            if (entries[e].g >= 0) close_segment(entries[e].g);
            else lit += entries[e].raw;
        }
        lit += "}\n";
        close_segment(-1);
        seg_off.push_back(static_cast<uint32_t>(group.size()));
        fixed_len.push_back(fixed);
    }
    while (lits.empty() || lits.size() % 4) lits.push_back(0);
    Image img;
    const size_t o_seg = img.put(seg_off), o_lo = img.put(lit_off), o_ll = img.put(lit_len), o_g = img.put(group), o_f = img.put(fixed_len),
                 o_l = img.put(lits);
    gx_handle::JsonlImage ji;
    GX_HIP(hipMalloc(ji.d.out(), img.bytes.size()));
    GX_HIP(hipMemcpy(ji.d.get(), img.bytes.data(), img.bytes.size(), hipMemcpyHostToDevice));
    const uint8_t* base = static_cast<const uint8_t*>(ji.d.get());
    ji.dev.seg_off = reinterpret_cast<const uint32_t*>(base + o_seg);
    ji.dev.lit_off = reinterpret_cast<const uint32_t*>(base + o_lo);
    ji.dev.lit_len = reinterpret_cast<const uint32_t*>(base + o_ll);
    ji.dev.group = reinterpret_cast<const int32_t*>(base + o_g);
    ji.dev.fixed_len = reinterpret_cast<const uint32_t*>(base + o_f);
    ji.dev.lits = base + o_l;
    ji.dev.lits_bytes = static_cast<uint32_t>(lits.size());
    ji.dev.n_rules = static_cast<uint32_t>(T.n_rules);
    ji.dev.n_segs = static_cast<uint32_t>(group.size());
    return h->jsonl.emplace(key, std::move(ji)).first->second.dev;
}

// What a pass over a batch's results reads, all of it in device memory: the ids (dense, or compact rows of row_units units), the
// n + 1 line offsets, the text in 8- or 16-bit units (wide), and the dense capture rows (nullptr: none, or compact rows hold them).
struct BatchView {
    const void* ids;
    RowFormat fmt;
    uint32_t row_units;
    uint64_t n;
    const void* offsets;
    bool off64;
    const void* data;
    const int32_t* caps;
    bool wide;
};
// A whole-file call's text on the device: the caller's own pointer (device_pointers; refused unless 16-byte aligned), or a copy that
// lives as long as this object.
namespace {
struct StagedText {
    DevMem<uint8_t> copy;
    const uint8_t* src;
};
}  // namespace
static StagedText stage_text(const uint8_t* text, uint64_t size, const gx_batch_opts& o, hipStream_t stream, const char* name) {
    StagedText t{{}, text};
    if (!o.device_pointers) {
        t.copy = dev_alloc<uint8_t>(size);
        if (size) GX_HIP(hipMemcpyAsync(t.copy.get(), text, size, hipMemcpyHostToDevice, stream));
        t.src = t.copy.get();
    } else if (reinterpret_cast<uintptr_t>(text) & 15u) {
        throw GxError(GX_E_ARG, std::string(name) + ": device text must be 16-byte aligned");
    }
    return t;
}

// Steps 1 and 2 of the whole-file calls (gx_text_to_jsonl, gx_text_select), under h->mu: raw text on the device -> line offsets
// (gx_split_lines semantics, 32-bit) -> the match-and-extract path, enqueued on `stream`.  Everything lives in the handle's scratch:
// 2 split workspace, 3 offsets, 4 ids, 5 captures (dense rows; unset for a handle without capture regexps).  The line count is read
// on the host: one synchronisation.  esc_bits / passthrough: launch_split_lines'.
struct TextLines {
    uint64_t n;
    GxBatch b;
    uint32_t mean_in;
    bool no_control_bytes;   // with esc_bits: no byte of the text takes five more bytes inside a JSON string
    // what the passes behind the path read: dense ids, 32-bit offsets, the text's bytes, dense capture rows
    BatchView view() const { return {b.match_id, ROWS_DENSE, 1, n, b.offsets, false, b.data, b.caps, false}; }
};
// utf8 (gx_batch_opts.utf8 = 1; not with esc_bits: the split pass's first kernel makes EITHER the escape bits or the masks of the bytes
// >= 0x80 that the line flags come from -- launch_split_lines refuses both at once -- so a utf8 text's JSON sizes are taken from the text
// itself, as gx_results_to_jsonl takes them): the text is UTF-8 -- the split pass leaves its line flags, and the lines that are not
// ASCII are walked again as Strings behind the batch kernel (utf8_fixup), their capture offsets back in bytes for the passes that follow.
static TextLines text_lines(gx_handle* h, const uint8_t* src, uint64_t size, size_t slots, hipStream_t stream, uint16_t* esc_bits, int passthrough,
                            bool utf8 = false) {
    // offsets for the guess "64 bytes or more per line"; a text with shorter lines is split a second time
    void* ws_split = h->scratch[2].get(split_workspace_bytes(size, utf8));
    uint64_t cap = size / 64 + 4096;
    void* d_off2 = h->scratch[3].get((cap + 1) * 4);
    uint64_t* d_n = nullptr;
    uint64_t* d_max = nullptr;
    std::optional<PoolBuffer> line_flags;
    if (utf8) line_flags.emplace(h, cap + 64, stream);
    uint8_t* d_flags = utf8 ? static_cast<uint8_t*>(line_flags->p) : nullptr;
    GX_HIP(launch_split_lines(src, size, d_off2, 0, cap, d_flags, ws_split, &d_n, stream, &d_max, esc_bits, passthrough));
    uint64_t n_and_max[3] = {0, 0, 0};   // (the line count, the longest line and the control-character word are neighbours in the workspace)
    GX_HIP(hipMemcpyAsync(n_and_max, d_n, 24, hipMemcpyDeviceToHost, stream));
    GX_HIP(hipStreamSynchronize(stream));
    TextLines t{};
    const uint64_t n = t.n = n_and_max[0];
    uint64_t longest = n_and_max[1];
    t.no_control_bytes = n_and_max[2] == 0;
    if (n > cap) {
        d_off2 = h->scratch[3].get((n + 1) * 4);
        if (utf8) {
            line_flags.emplace(h, n + 64, stream);
            d_flags = static_cast<uint8_t*>(line_flags->p);
        }
        GX_HIP(launch_split_lines(src, size, d_off2, 0, n, d_flags, ws_split, &d_n, stream));
        longest = 0;   // (measured over the first `cap` lines only: no promise)
    }
    void* d_mid = h->scratch[4].get(n * 4 + 16);
    void* d_caps = h->scratch[5].get(n * slots * 4 + 16);
    GxBatch& b = t.b;
    b.data = src; b.offsets = d_off2; b.n = n; b.match_id = static_cast<int32_t*>(d_mid);
    b.caps = h->T.has_capture ? static_cast<int32_t*>(d_caps) : nullptr;
    b.match_only = h->T.has_capture ? 0 : 1;
    b.strip_eol = 1;
    b.max_line_bytes = static_cast<uint32_t>(std::min<uint64_t>(longest, 0xFFFFFFFFull));   // (what the split pass saw: no follow-up launch)
    t.mean_in = n ? static_cast<uint32_t>(std::min<uint64_t>((size + n - 1) / n, 1u << 20)) : 1u;
    launch_batch(h, b, t.mean_in, GX_KERNEL_AUTO, stream);
    if (utf8) utf8_fixup(h, b, 1, d_flags, stream);
    if (!h->T.has_capture && n && slots) GX_HIP(hipMemsetAsync(d_caps, 0xFF, n * slots * 4, stream));
    b.caps = static_cast<int32_t*>(d_caps);
    return t;
}
// A whole-file reduction's batch: the text staged, split and extracted (no escape bits), and the view of what that left (v.n: the text's lines).
namespace {
struct TextBatch {
    StagedText text;
    BatchView v;
};
}  // namespace
static TextBatch stage_text_lines(gx_handle* h, const uint8_t* text, uint64_t size, const gx_batch_opts& o, hipStream_t stream, const char* name) {
    TextBatch t{stage_text(text, size, o, stream, name), {}};
    t.v = text_lines(h, t.text.src, size, 2 * static_cast<size_t>(h->T.max_groups), stream, nullptr, 0, o.utf8 != 0).view();
    return t;
}

int gx_results_to_jsonl(gx_handle* h, const uint8_t* bytes, const void* offsets, uint64_t n, const int32_t* match_id, const int32_t* caps,
                        const char* id_as, uint8_t* out, uint64_t out_cap, uint64_t* out_size, uint64_t* line_out_offsets,
                        const gx_batch_opts* opts) {
    return guarded([&]() -> int {
        if (!h || !offsets || !out_size || (n && !match_id)) return fail(GX_E_ARG, "gx_results_to_jsonl: bad argument");
        if (!h->on_device) return fail(GX_E_DEVICE, "handle was created host-only; no device tables (there is no CPU fallback)");
        const gx_batch_opts o = read_opts(opts);
        const size_t slots = 2 * static_cast<size_t>(h->T.max_groups);
        if (n && slots && !caps) return fail(GX_E_ARG, "gx_results_to_jsonl: caps is NULL");
        if (slots > 128) return fail(GX_E_LIMIT, "gx_results_to_jsonl: more than 64 capture groups per extraction");
        GX_HIP(hipSetDevice(h->device));
        std::lock_guard<std::mutex> lock(h->mu);
        const GxJsonl& tm = jsonl_templates(h, id_as);
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        const size_t off_w = o.offsets64 ? 8 : 4;
        DevMem<> d_bytes, d_off, d_mid, d_caps;
        DevMem<uint8_t> d_out;
        void* ws = h->scratch[0].get(jsonl_workspace_bytes(n));
        GxBatch b{};
        b.n = n;
        b.offsets64 = o.offsets64 ? 1 : 0;
        uint64_t* loff = line_out_offsets;
        // mean line length, for the LDS staging of the kernels (device pointers: from the two ends of the offsets array)
        std::pair<uint64_t, uint64_t> ends{0, 0};
        if (o.device_pointers) {
            b.data = bytes; b.offsets = offsets; b.match_id = const_cast<int32_t*>(match_id); b.caps = const_cast<int32_t*>(caps);
            if (!loff) loff = static_cast<uint64_t*>(h->scratch[1].get((n + 1) * 8));
            if (n) ends = device_offset_ends(offsets, n, o.offsets64 != 0, stream);
        } else {
            const HostOffsets off{offsets, o.offsets64 != 0, n};
            const uint64_t total_in = n ? off[n] : 0;
            d_bytes = dev_alloc(total_in); d_off = dev_alloc((n + 1) * off_w); d_mid = dev_alloc(n * 4); d_caps = dev_alloc(n * slots * 4);
            if (total_in) GX_HIP(hipMemcpyAsync(d_bytes.get(), bytes, total_in, hipMemcpyHostToDevice, stream));
            GX_HIP(hipMemcpyAsync(d_off.get(), offsets, (n + 1) * off_w, hipMemcpyHostToDevice, stream));
            if (n) GX_HIP(hipMemcpyAsync(d_mid.get(), match_id, n * 4, hipMemcpyHostToDevice, stream));
            if (n && slots) GX_HIP(hipMemcpyAsync(d_caps.get(), caps, n * slots * 4, hipMemcpyHostToDevice, stream));
            b.data = d_bytes.get(); b.offsets = d_off.get(); b.match_id = static_cast<int32_t*>(d_mid.get()); b.caps = static_cast<int32_t*>(d_caps.get());
            loff = static_cast<uint64_t*>(h->scratch[1].get((n + 1) * 8));
            if (n) ends = {off[0], off[n]};
        }
        const uint32_t mean_in = n ? static_cast<uint32_t>(std::min<uint64_t>((ends.second - ends.first + n - 1) / n, 1u << 20)) : 1u;
        GX_HIP(launch_jsonl_sizes(tm, b, static_cast<int>(slots), o.utf8_passthrough ? 1 : 0, mean_in, loff, ws, stream));
        uint64_t total = 0;
        GX_HIP(hipMemcpyAsync(&total, loff + n, 8, hipMemcpyDeviceToHost, stream));
        GX_HIP(hipStreamSynchronize(stream));
        *out_size = total;
        if (!o.device_pointers && line_out_offsets) GX_HIP(hipMemcpy(line_out_offsets, loff, (n + 1) * 8, hipMemcpyDeviceToHost));
        if (!out) return GX_OK;  // size query
        if (total > out_cap) return fail(GX_E_LIMIT, "gx_results_to_jsonl: out_cap is smaller than the text (see *out_size)");
        uint8_t* dst = out;
        if (!o.device_pointers) { d_out = dev_alloc<uint8_t>(total); dst = d_out.get(); }
        const uint32_t mean_out = n ? static_cast<uint32_t>(std::min<uint64_t>((total + n - 1) / n, 1u << 20)) : 1u;
        GX_HIP(launch_jsonl_write(tm, b, static_cast<int>(slots), o.utf8_passthrough ? 1 : 0, mean_in, mean_out, loff, dst, ws, stream));
        if (!o.device_pointers && total) GX_HIP(hipMemcpyAsync(out, dst, total, hipMemcpyDeviceToHost, stream));
        GX_HIP(hipStreamSynchronize(stream));
        return GX_OK;
    });
}

int gx_text_to_jsonl(gx_handle* h, const uint8_t* text, uint64_t size, const char* id_as, uint8_t* out, uint64_t out_cap, uint64_t* out_size,
                     uint64_t* n_lines, uint64_t* n_matched, uint64_t* n_exceptions, const gx_batch_opts* opts) {
    return guarded([&]() -> int {
        if (!h || !out_size || (size && !text)) return fail(GX_E_ARG, "gx_text_to_jsonl: bad argument");
        if (!h->on_device) return fail(GX_E_DEVICE, "handle was created host-only; no device tables (there is no CPU fallback)");
        if (size > 0xFFFFFFFFull) return fail(GX_E_LIMIT, "gx_text_to_jsonl: split texts of 4 GiB and more at a line boundary");
        const gx_batch_opts o = read_opts(opts);
        if (o.utf8 == 2) return fail(GX_E_ARG, "gx_text_to_jsonl: gx_batch_opts.utf8 = 1 (the text is written from its bytes)");
        const size_t slots = 2 * static_cast<size_t>(h->T.max_groups);
        if (slots > 128) return fail(GX_E_LIMIT, "gx_text_to_jsonl: more than 64 capture groups per extraction");
        GX_HIP(hipSetDevice(h->device));
        std::lock_guard<std::mutex> lock(h->mu);
        const GxJsonl& tm = jsonl_templates(h, id_as);
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        // (host buffers only; everything between lives in the handle's scratch: 2 split workspace, 3 offsets, 4 ids, 5 captures, 6 counts)
        const StagedText st = stage_text(text, size, o, stream, "gx_text_to_jsonl");
        DevMem<uint8_t> d_out;
        // 1. lines, 2. the path
        // (the split pass also leaves a bit per byte that takes one more byte inside a JSON string, and says whether some byte takes five
        // more -- a control character --: without one, the sizes pass below does not read the text again)
        // (utf8: the split pass makes line flags in their place)
        uint16_t* esc_bits = o.utf8 ? nullptr : static_cast<uint16_t*>(h->scratch[7].get(((size + 32767) / 32768) * 4096 + 64));   // (written in whole blocks of 32 KiB of text)
        const int passthrough = (o.utf8_passthrough || o.utf8) ? 1 : 0;   // (utf8 implies it)
        const TextLines tl = text_lines(h, st.src, size, slots, stream, esc_bits, passthrough, o.utf8 != 0);
        const uint64_t n = tl.n;
        const GxBatch& b = tl.b;
        const uint32_t mean_in = tl.mean_in;
        const bool sizes_from_bits = !o.utf8 && tl.no_control_bytes;   // (utf8: the split pass made line flags, not escape bits)
        void* d_counts = h->scratch[6].get(16);
        GX_HIP(launch_count_outcomes(b.match_id, n, static_cast<unsigned long long*>(d_counts), stream));
        // 3. the text
        void* ws_json = h->scratch[0].get(jsonl_workspace_bytes(n));
        uint64_t* loff = static_cast<uint64_t*>(h->scratch[1].get((n + 1) * 8));
        GX_HIP(launch_jsonl_sizes(tm, b, static_cast<int>(slots), passthrough, mean_in, loff, ws_json, stream,
                                  sizes_from_bits ? reinterpret_cast<const uint32_t*>(esc_bits) : nullptr));
        uint64_t total = 0;
        unsigned long long counts[2] = {0, 0};
        GX_HIP(hipMemcpyAsync(&total, loff + n, 8, hipMemcpyDeviceToHost, stream));
        GX_HIP(hipMemcpyAsync(counts, d_counts, 16, hipMemcpyDeviceToHost, stream));
        GX_HIP(hipStreamSynchronize(stream));
        // (the extraction ran on the split pass's own longest line; a kernel that met a longer one after all left rows unwritten)
        if (promise_broken_since(h, stream)) throw GxError(GX_E_ARG, "internal: gx_text_to_jsonl: a line longer than the split pass reported");
        *out_size = total;
        if (n_lines) *n_lines = n;
        if (n_matched) *n_matched = counts[0];
        if (n_exceptions) *n_exceptions = counts[1];
        if (!out) return GX_OK;
        if (total > out_cap) return fail(GX_E_LIMIT, "gx_text_to_jsonl: out_cap is smaller than the text (see *out_size)");
        uint8_t* dst = out;
        if (!o.device_pointers) { d_out = dev_alloc<uint8_t>(total); dst = d_out.get(); }
        const uint32_t mean_out = n ? static_cast<uint32_t>(std::min<uint64_t>((total + n - 1) / n, 1u << 20)) : 1u;
        GX_HIP(launch_jsonl_write(tm, b, static_cast<int>(slots), passthrough, mean_in, mean_out, loff, dst, ws_json, stream));
        if (!o.device_pointers && total) GX_HIP(hipMemcpyAsync(out, dst, total, hipMemcpyDeviceToHost, stream));
        GX_HIP(hipStreamSynchronize(stream));
        return GX_OK;
    });
}

// The format of an id column as gx_batch_opts.compact_results names it, and the units of one of its rows.
static RowFormat id_format(const gx_handle* h, const gx_batch_opts& o, uint32_t* row_units) {
    if (o.compact_results > 2) throw GxError(GX_E_ARG, "gx_batch_opts.compact_results: 0, 1 or 2");
    const RowFormat f = row_format(o.compact_results != 0, o.compact_results == 2);
    *row_units = f == ROWS_DENSE ? 1u : 1u + 2u * static_cast<uint32_t>(h->T.max_groups);
    return f;
}

// A "lines" call's batch on the device.  With device_pointers the view is of the caller's own pointers; host buffers are copied to
// device memory that lives as long as this object, and the view is of the copies.
namespace {
struct StagedLines {
    BatchView v;
    DevMem<> bytes, offsets, ids, caps;
};
}  // namespace
// what of a host batch a call's passes read besides the ids and the offsets (device pointers travel nowhere)
struct Travels {
    bool text, caps;
};
static StagedLines stage_lines(const gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps, const gx_batch_opts& o,
                               RowFormat fmt, uint32_t row_units, Travels travels, hipStream_t stream, const char* name) {
    StagedLines s{{ids, fmt, row_units, n, offsets, o.offsets64 != 0, bytes, caps, o.utf16 != 0}, {}, {}, {}, {}};
    if (o.device_pointers) return s;
    const size_t off_w = o.offsets64 ? 8 : 4, unit = o.utf16 ? 2 : 1, id_row = static_cast<size_t>(row_units) * row_unit_bytes(fmt);
    const size_t slots = 2 * static_cast<size_t>(h->T.max_groups);
    const size_t in_bytes = static_cast<size_t>(HostOffsets{offsets, o.offsets64 != 0, n}[n]) * unit;
    if (in_bytes && !bytes) throw GxError(GX_E_ARG, std::string(name) + ": bytes is NULL");
    if (travels.text) s.bytes = dev_alloc(in_bytes);
    s.offsets = dev_alloc((n + 1) * off_w);
    s.ids = dev_alloc(n * id_row);
    if (travels.text && in_bytes) GX_HIP(hipMemcpyAsync(s.bytes.get(), bytes, in_bytes, hipMemcpyHostToDevice, stream));
    GX_HIP(hipMemcpyAsync(s.offsets.get(), offsets, (n + 1) * off_w, hipMemcpyHostToDevice, stream));
    if (n) GX_HIP(hipMemcpyAsync(s.ids.get(), ids, n * id_row, hipMemcpyHostToDevice, stream));
    if (travels.caps && n && slots) {
        s.caps = dev_alloc(n * slots * 4);
        GX_HIP(hipMemcpyAsync(s.caps.get(), caps, n * slots * 4, hipMemcpyHostToDevice, stream));
    }
    s.v.data = s.bytes.get(); s.v.offsets = s.offsets.get(); s.v.ids = s.ids.get(); s.v.caps = static_cast<const int32_t*>(s.caps.get());
    return s;
}

// Host offsets: a line of 4 G code units (or offsets that go backwards) is found here; device offsets by the call's first pass.
static void refuse_long_host_lines(const HostOffsets& off, const std::string& name, const char* verb) {
    for (uint64_t i = 0; i < off.n; ++i)
        if (off[i + 1] - off[i] > 0xFFFFFFFFull) throw GxError(GX_E_LIMIT, name + ": a line of 4 G code units or more cannot be " + verb);
}

// A pass left running on a caller's stream still reads one of the handle's workspaces (select_event, group_event, top_event): it
// records the event, and the workspace's next user makes its stream wait for it first.
static void leave_pending(Event& event, bool& pending, hipStream_t stream) {
    if (!event) GX_HIP(hipEventCreateWithFlags(event.out(), hipEventDisableTiming));
    GX_HIP(hipEventRecord(event.get(), stream));
    pending = true;
}
static void wait_pending(const Event& event, bool& pending, hipStream_t stream) {
    if (!pending) return;
    GX_HIP(hipStreamWaitEvent(stream, event.get(), 0));
    pending = false;
}

// Where selected lines go: the caller's pointers, each nullptr when not wanted.
struct LinesOut {
    uint32_t* index;
    void* bytes;
    void* offsets;
    void* ids;
    int32_t* caps;
    bool per_line() const { return index || offsets || ids || caps; }
    bool any() const { return per_line() || bytes; }
};
// What the copy pass (launch_select_copy, launch_partition_copy) writes for `lines` lines of `units` code units: straight to the
// caller's device pointers, or -- host buffers -- to device twins that live as long as this object and that deliver() copies back.
namespace {
struct StagedLinesOut {
    SelectOut dev{};
    HostTwins twins;
    // behind the copy pass, host buffers only: the twins back to the caller's buffers
    void deliver(hipStream_t stream) const { twins.deliver(stream); }
};
}  // namespace
static StagedLinesOut stage_lines_out(const gx_handle* h, const BatchView& v, const LinesOut& out, bool host, uint64_t lines, uint64_t units) {
    const size_t off_w = v.off64 ? 8 : 4, unit = v.wide ? 2 : 1, id_row = static_cast<size_t>(v.row_units) * row_unit_bytes(v.fmt);
    const size_t slots = 2 * static_cast<size_t>(h->T.max_groups);
    StagedLinesOut s;
    s.twins = HostTwins(host);
    s.dev.index = s.twins.of(out.index, lines * 4);
    s.dev.bytes = s.twins.of(out.bytes, units * unit);
    s.dev.offsets = s.twins.of(out.offsets, (lines + 1) * off_w);
    if (out.ids) { s.dev.col_src[0] = v.ids; s.dev.col_dst[0] = s.twins.of(out.ids, lines * id_row); s.dev.col_width[0] = v.row_units; s.dev.col_unit_bytes[0] = row_unit_bytes(v.fmt); }
    if (out.caps) { s.dev.col_src[1] = v.caps; s.dev.col_dst[1] = s.twins.of(out.caps, lines * slots * 4); s.dev.col_width[1] = static_cast<uint32_t>(slots); s.dev.col_unit_bytes[1] = 4; }
    return s;
}

// The histogram of a batch's outcomes beside a reduction of it (k_select_flags' counting form, on the handle's select workspace, under
// h->mu): enqueued on `stream`, and in counts[2K + 2] once the caller's next wait for the stream is over.  Only v's ids are read.
static void counts_beside(gx_handle* h, const BatchView& v, uint64_t* counts, hipStream_t stream) {
    const uint32_t K = static_cast<uint32_t>(h->T.n_rules);
    wait_pending(h->select_event, h->select_pending, stream);
    const SelectWs w = select_workspace(h->select_ws.get(select_workspace_bytes(v.n, K, false)), v.n, K, false);
    GX_HIP(launch_select_flags(v.ids, v.fmt, v.row_units, K, v.n, nullptr, 0, w, stream));
    GX_HIP(hipMemcpyAsync(counts, w.counts, static_cast<size_t>(2u * K + 2u) * 8, hipMemcpyDeviceToHost, stream));
}

// The flags pass and the two scans behind it, on the handle's workspace (under h->mu); then the host reads what it must know
// before anything is written -- the number of kept lines and of kept code units, and whether a line was too long to count -- and
// the histogram if the caller wants it: ONE small synchronisation of the stream, as gx_pack_results has (before it the want mask
// goes to the device: a second small transfer per call, from pageable memory, which the runtime stages).
// want: host, uint8_t[2K + 1].
struct Selected {
    SelectWs w;
    uint64_t lines = 0, units = 0;
};
// The terms of a gx_select_lines_where call as its flags pass reads them (gx_where.hpp: WhereHead, then the literals in the batch's
// code units), checked against the handle; `none` when the call has no terms.  Needs no device.
struct WhereImage {
    std::vector<uint8_t> bytes;   // empty: no terms
    bool formats = false;         // an integer term reads a group whose format is not LONG (gx_set_number_format)
    bool none() const { return bytes.empty(); }
};
static WhereImage where_image(const gx_handle* h, const gx_where_term* terms, uint32_t n_terms, bool wide, const std::string& name) {
    WhereImage img;
    if (n_terms == 0) return img;
    if (!terms) throw GxError(GX_E_ARG, name + ": terms is NULL");
    if (n_terms > WHERE_MAX_TERMS) throw GxError(GX_E_LIMIT, name + ": more than 64 terms");
    const int32_t K = static_cast<int32_t>(h->T.n_rules);
    const size_t unit = wide ? 2 : 1;
    std::vector<uint32_t> order(n_terms);
    size_t lit_units = 0;
    for (uint32_t t = 0; t < n_terms; ++t) {
        const gx_where_term& m = terms[t];
        order[t] = t;
        if (m.extraction < 0 || m.extraction >= K) throw GxError(GX_E_ARG, name + ": a term's extraction is not in [0, K)");
        if (m.group < 0 || m.group >= gx_num_groups(h, m.extraction)) throw GxError(GX_E_ARG, name + ": a term's group is not one of its extraction's");
        if (m.op >= WHERE_OPS) throw GxError(GX_E_ARG, name + ": a term's op is no GX_WHERE_* value");
        const bool text_op = m.op >= WHERE_EQ && m.op <= WHERE_CONTAINS;
        if (text_op && m.text_units > WHERE_MAX_TEXT) throw GxError(GX_E_LIMIT, name + ": a term's text has more than 255 code units");
        if (text_op && m.text_units && !m.text) throw GxError(GX_E_ARG, name + ": a term's text is NULL");
        if (text_op) lit_units += m.text_units;
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return terms[a].extraction < terms[b].extraction; });
    img.bytes.assign((sizeof(WhereHead) + lit_units * unit + 15) & ~static_cast<size_t>(15), 0);
    WhereHead head{};
    head.n_terms = n_terms;
    head.lit_units = static_cast<uint32_t>(lit_units);
    uint8_t* lits = img.bytes.data() + sizeof(WhereHead);
    size_t at = 0;
    for (uint32_t q = 0; q < n_terms; ++q) {
        const gx_where_term& m = terms[order[q]];
        if (head.n_ext == 0 || head.ext[head.n_ext - 1] != static_cast<uint32_t>(m.extraction)) {
            head.ext[head.n_ext] = static_cast<uint32_t>(m.extraction);
            head.first[head.n_ext++] = static_cast<uint8_t>(q);
        }
        const bool text_op = m.op >= WHERE_EQ && m.op <= WHERE_CONTAINS;
        WhereTerm& d = head.term[q];
        d.group = static_cast<uint16_t>(m.group);
        d.op = static_cast<uint8_t>(m.op);
        d.negate = m.negate ? 1 : 0;
        d.number = m.number;
        if (m.op >= WHERE_INT_EQ) head.fmt[q] = h->number_format_of(m.extraction, m.group);   // (nothing else sees the format)
        if (head.fmt[q]) head.formats = 1u;
        d.lit_at = static_cast<uint16_t>(at);
        d.lit_len = text_op ? static_cast<uint16_t>(m.text_units) : 0;
        if (d.lit_len) memcpy(lits + at * unit, m.text, d.lit_len * unit);
        at += d.lit_len;
    }
    head.first[head.n_ext] = static_cast<uint8_t>(n_terms);
    img.formats = head.formats != 0u;
    memcpy(img.bytes.data(), &head, sizeof(head));
    return img;
}
// A reduction's image on the device, in a buffer of the handle's: the head, a quantile call's QuantHead behind it, then the terms (small
// transfers from pageable memory, which the runtime stages).  terms: nullptr when the call has none.
struct DevImage {
    uint8_t *head, *terms;
};
static DevImage upload_image(GrowBuf& buf, const void* head, size_t head_bytes, const QuantHead* second, const WhereImage& wi, hipStream_t stream) {
    const size_t at_terms = head_bytes + (second ? sizeof(QuantHead) : 0);
    uint8_t* d = static_cast<uint8_t*>(buf.get(at_terms + wi.bytes.size()));
    GX_HIP(hipMemcpyAsync(d, head, head_bytes, hipMemcpyHostToDevice, stream));
    if (second) GX_HIP(hipMemcpyAsync(d + head_bytes, second, sizeof(QuantHead), hipMemcpyHostToDevice, stream));
    if (!wi.none()) GX_HIP(hipMemcpyAsync(d + at_terms, wi.bytes.data(), wi.bytes.size(), hipMemcpyHostToDevice, stream));
    return {d, wi.none() ? nullptr : d + at_terms};
}
static Selected select_pass(gx_handle* h, const BatchView& v, const uint8_t* want, const WhereImage& where, uint64_t* counts, hipStream_t stream) {
    const uint32_t K = static_cast<uint32_t>(h->T.n_rules), bins = 2u * K + 2u;
    const uint64_t n = v.n;
    wait_pending(h->select_event, h->select_pending, stream);
    Selected s;
    s.w = select_workspace(h->select_ws.get(select_workspace_bytes(n, K, true)), n, K, true);
    GX_HIP(hipMemcpyAsync(s.w.want, want, bins - 1u, hipMemcpyHostToDevice, stream));
    if (!where.none()) {
        // (the terms and literals go beside the mask, the same way: a small transfer from pageable memory)
        void* d_img = h->where_image.get(where.bytes.size());
        GX_HIP(hipMemcpyAsync(d_img, where.bytes.data(), where.bytes.size(), hipMemcpyHostToDevice, stream));
        const WhereArgs a{v.data, v.wide ? 1 : 0, v.caps, 2u * static_cast<uint32_t>(h->T.max_groups), d_img, static_cast<uint32_t>(where.bytes.size()),
                          where.formats ? 1u : 0u};
        GX_HIP(launch_where_flags(v.ids, v.fmt, v.row_units, K, n, v.offsets, v.off64 ? 1 : 0, a, counts != nullptr, s.w, stream));
    } else {
        GX_HIP(launch_select_flags(v.ids, v.fmt, v.row_units, K, n, v.offsets, v.off64 ? 1 : 0, s.w, stream));
    }
    uint32_t status = 0;
    GX_HIP(hipMemcpyAsync(&s.lines, s.w.idx_off + n, 8, hipMemcpyDeviceToHost, stream));
    GX_HIP(hipMemcpyAsync(&s.units, s.w.dst_off + n, 8, hipMemcpyDeviceToHost, stream));
    GX_HIP(hipMemcpyAsync(&status, s.w.status, 4, hipMemcpyDeviceToHost, stream));
    if (counts) GX_HIP(hipMemcpyAsync(counts, s.w.counts, static_cast<size_t>(bins) * 8, hipMemcpyDeviceToHost, stream));
    GX_HIP(hipStreamSynchronize(stream));
    if (status) throw GxError(GX_E_LIMIT, "a line of 4 G code units or more cannot be selected");
    return s;
}

int gx_count_outcomes(gx_handle* h, const void* ids, uint64_t n, uint64_t* counts, const gx_batch_opts* opts) {
    return guarded([&]() -> int {
        if (!h || !counts || (n && !ids)) return fail(GX_E_ARG, "gx_count_outcomes: bad argument");
        if (!h->on_device) return fail(GX_E_DEVICE, "handle was created host-only; no device tables (there is no CPU fallback)");
        const gx_batch_opts o = read_opts(opts);
        uint32_t row_units = 1;
        const RowFormat fmt = id_format(h, o, &row_units);
        GX_HIP(hipSetDevice(h->device));
        std::lock_guard<std::mutex> lock(h->mu);
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        DevMem<> d_ids;
        if (!o.device_pointers) {
            const size_t bytes = static_cast<size_t>(n) * row_units * row_unit_bytes(fmt);
            d_ids = dev_alloc(bytes);
            if (bytes) GX_HIP(hipMemcpyAsync(d_ids.get(), ids, bytes, hipMemcpyHostToDevice, stream));
            ids = d_ids.get();
        }
        counts_beside(h, BatchView{ids, fmt, row_units, n, nullptr, false, nullptr, nullptr, false}, counts, stream);
        GX_HIP(hipStreamSynchronize(stream));
        return GX_OK;
    });
}

// gx_select_lines and gx_select_lines_where (where: the latter, whose refusals come before the look at the device)
static int select_lines_call(const char* fn, bool where, gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps,
                             const uint8_t* want, const gx_where_term* terms, uint32_t n_terms, uint32_t* out_index, void* out_bytes, void* out_offsets,
                             void* out_ids, int32_t* out_caps, uint64_t cap_lines, uint64_t out_bytes_cap, uint64_t* n_selected, uint64_t* bytes_selected,
                             const gx_batch_opts* opts) {
    const std::string name = fn;
    return guarded([&]() -> int {
        if (!h || !want || !offsets || !n_selected || !bytes_selected || (n && !ids)) return fail(GX_E_ARG, name + ": bad argument");
        WhereImage image;
        if (where) {
            const gx_batch_opts wo = read_opts(opts);
            uint32_t units = 1;
            const RowFormat wf = id_format(h, wo, &units);
            if (wo.utf8 == 2) return fail(GX_E_ARG, name + ": gx_batch_opts.utf8 = 1 (values are compared in the units the offsets count)");
            image = where_image(h, terms, n_terms, wo.utf16 != 0, name);
            if (!image.none() && wf == ROWS_DENSE && n && !caps) return fail(GX_E_ARG, name + ": terms on dense ids need caps");
        }
        if (!h->on_device) return fail(GX_E_DEVICE, "handle was created host-only; no device tables (there is no CPU fallback)");
        if (n >= (1ull << 32)) return fail(GX_E_LIMIT, name + ": line numbers are 32 bits; split batches of 4 G lines and more");
        const gx_batch_opts o = read_opts(opts);
        uint32_t row_units = 1;
        const RowFormat fmt = id_format(h, o, &row_units);
        const size_t slots = 2 * static_cast<size_t>(h->T.max_groups);
        if (fmt != ROWS_DENSE) { caps = nullptr; out_caps = nullptr; }
        if (out_caps && slots && n && !caps) return fail(GX_E_ARG, name + ": out_caps without caps");
        if (!slots) out_caps = nullptr;
        if (o.no_sync && !o.device_pointers) return fail(GX_E_ARG, name + ": no_sync needs device pointers");
        GX_HIP(hipSetDevice(h->device));
        std::lock_guard<std::mutex> lock(h->mu);
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        const size_t unit = o.utf16 ? 2 : 1;
        const bool host = !o.device_pointers;
        // (the capture rows travel only if they are asked for, or read by terms)
        const StagedLines in = stage_lines(h, bytes, offsets, n, ids, caps, o, fmt, row_units, Travels{true, out_caps || (caps && !image.none())}, stream, name.c_str());
        const BatchView& v = in.v;
        const Selected s = select_pass(h, v, want, image, nullptr, stream);
        *n_selected = s.lines;
        *bytes_selected = s.units * unit;
        const LinesOut lo{out_index, out_bytes, out_offsets, out_ids, out_caps};
        if (!lo.any()) return GX_OK;   // size query
        if (lo.per_line() && s.lines > cap_lines) return fail(GX_E_LIMIT, name + ": cap_lines is smaller than the selection (see *n_selected)");
        if (out_bytes && s.units * unit > out_bytes_cap)
            return fail(GX_E_LIMIT, name + ": out_bytes_cap is smaller than the selected text (see *bytes_selected)");
        const StagedLinesOut out = stage_lines_out(h, v, lo, host, s.lines, s.units);
        if (out.dev.offsets && n == 0) GX_HIP(hipMemsetAsync(out.dev.offsets, 0, v.off64 ? 8 : 4, stream));
        GX_HIP(launch_select_copy(out.dev, v.data, v.offsets, v.off64 ? 1 : 0, v.wide ? 1 : 0, n, s.w, stream));
        if (host) out.deliver(stream);
        // (no_sync: the copy pass still reads the workspace: whoever uses it next waits for this)
        if (o.no_sync) leave_pending(h->select_event, h->select_pending, stream);
        else GX_HIP(hipStreamSynchronize(stream));
        return GX_OK;
    });
}

int gx_select_lines(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps, const uint8_t* want,
                    uint32_t* out_index, void* out_bytes, void* out_offsets, void* out_ids, int32_t* out_caps, uint64_t cap_lines,
                    uint64_t out_bytes_cap, uint64_t* n_selected, uint64_t* bytes_selected, const gx_batch_opts* opts) {
    return select_lines_call("gx_select_lines", false, h, bytes, offsets, n, ids, caps, want, nullptr, 0, out_index, out_bytes, out_offsets, out_ids, out_caps,
                             cap_lines, out_bytes_cap, n_selected, bytes_selected, opts);
}

int gx_select_lines_where(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps, const uint8_t* want,
                          const gx_where_term* terms, uint32_t n_terms, uint32_t* out_index, void* out_bytes, void* out_offsets, void* out_ids,
                          int32_t* out_caps, uint64_t cap_lines, uint64_t out_bytes_cap, uint64_t* n_selected, uint64_t* bytes_selected,
                          const gx_batch_opts* opts) {
    return select_lines_call("gx_select_lines_where", true, h, bytes, offsets, n, ids, caps, want, terms, n_terms, out_index, out_bytes, out_offsets, out_ids,
                             out_caps, cap_lines, out_bytes_cap, n_selected, bytes_selected, opts);
}

// gx_text_select and gx_text_select_where (where: the latter, whose refusals come before the look at the device)
static int text_select_call(const char* fn, bool where, gx_handle* h, const uint8_t* text, uint64_t size, const uint8_t* want, const gx_where_term* terms,
                            uint32_t n_terms, uint8_t* out, uint64_t out_cap, uint64_t* out_size, uint64_t* counts, uint64_t* n_lines,
                            const gx_batch_opts* opts) {
    const std::string name = fn;
    return guarded([&]() -> int {
        if (!h || !want || !out_size || (size && !text)) return fail(GX_E_ARG, name + ": bad argument");
        WhereImage image;
        if (where) {
            if (read_opts(opts).utf8 == 2) return fail(GX_E_ARG, name + ": gx_batch_opts.utf8 = 1 (lines are selected by their bytes)");
            image = where_image(h, terms, n_terms, false, name);
        }
        if (!h->on_device) return fail(GX_E_DEVICE, "handle was created host-only; no device tables (there is no CPU fallback)");
        if (size > 0xFFFFFFFFull) return fail(GX_E_LIMIT, name + ": split texts of 4 GiB and more at a line boundary");
        const gx_batch_opts o = read_opts(opts);
        const size_t slots = 2 * static_cast<size_t>(h->T.max_groups);
        GX_HIP(hipSetDevice(h->device));
        std::lock_guard<std::mutex> lock(h->mu);
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        const StagedText st = stage_text(text, size, o, stream, name.c_str());
        DevMem<uint8_t> d_out;
        if (o.utf8 == 2) return fail(GX_E_ARG, name + ": gx_batch_opts.utf8 = 1 (lines are selected by their bytes)");
        // the lines and the path; then the selection's passes over the ids and offsets they left on the device
        const TextLines tl = text_lines(h, st.src, size, slots, stream, nullptr, 0, o.utf8 != 0);
        const Selected s = select_pass(h, tl.view(), want, image, counts, stream);
        if (promise_broken_since(h, stream)) throw GxError(GX_E_ARG, "internal: " + name + ": a line longer than the split pass reported");
        *out_size = s.units;
        if (n_lines) *n_lines = tl.n;
        if (!out) return GX_OK;
        if (s.units > out_cap) return fail(GX_E_LIMIT, name + ": out_cap is smaller than the selected text (see *out_size)");
        SelectOut sel{};
        sel.bytes = out;
        if (!o.device_pointers) { d_out = dev_alloc<uint8_t>(s.units); sel.bytes = d_out.get(); }
        GX_HIP(launch_select_copy(sel, st.src, tl.b.offsets, 0, 0, tl.n, s.w, stream));
        if (!o.device_pointers && s.units) GX_HIP(hipMemcpyAsync(out, sel.bytes, s.units, hipMemcpyDeviceToHost, stream));
        GX_HIP(hipStreamSynchronize(stream));
        return GX_OK;
    });
}

int gx_text_select(gx_handle* h, const uint8_t* text, uint64_t size, const uint8_t* want, uint8_t* out, uint64_t out_cap, uint64_t* out_size,
                   uint64_t* counts, uint64_t* n_lines, const gx_batch_opts* opts) {
    return text_select_call("gx_text_select", false, h, text, size, want, nullptr, 0, out, out_cap, out_size, counts, n_lines, opts);
}

int gx_text_select_where(gx_handle* h, const uint8_t* text, uint64_t size, const uint8_t* want, const gx_where_term* terms, uint32_t n_terms, uint8_t* out,
                         uint64_t out_cap, uint64_t* out_size, uint64_t* counts, uint64_t* n_lines, const gx_batch_opts* opts) {
    return text_select_call("gx_text_select_where", true, h, text, size, want, terms, n_terms, out, out_cap, out_size, counts, n_lines, opts);
}

// The measures of a gx_capture_stats call as its kernel reads them (gx_stats.hpp: StatsHead, then the edges), checked against the
// handle.  The kernel's measures are ordered by extraction: order[q] is the caller's index of the kernel's measure q.  Needs no device.
struct StatsImage {
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> order;
    uint32_t n_bins = 0;
    bool formats = false;   // a measure reads a group whose format is not LONG (gx_set_number_format)
};
static StatsImage stats_image(const gx_handle* h, const gx_measure* measures, uint32_t n_measures, const std::string& name) {
    StatsImage img;
    if (n_measures == 0) return img;
    if (!measures) throw GxError(GX_E_ARG, name + ": measures is NULL");
    if (n_measures > STATS_MAX_MEASURES) throw GxError(GX_E_LIMIT, name + ": more than 64 measures");
    const int32_t K = static_cast<int32_t>(h->T.n_rules);
    size_t n_edges = 0;
    img.order.resize(n_measures);
    for (uint32_t t = 0; t < n_measures; ++t) {
        const gx_measure& m = measures[t];
        img.order[t] = t;
        if (m.extraction < 0 || m.extraction >= K) throw GxError(GX_E_ARG, name + ": a measure's extraction is not in [0, K)");
        if (m.group < 0 || m.group >= gx_num_groups(h, m.extraction)) throw GxError(GX_E_ARG, name + ": a measure's group is not one of its extraction's");
        if (m.n_edges > STATS_MAX_EDGES) throw GxError(GX_E_LIMIT, name + ": a measure has more than 64 edges");
        if (m.n_edges && !m.edges) throw GxError(GX_E_ARG, name + ": a measure's edges is NULL");
        for (uint32_t j = 1; j < m.n_edges; ++j)
            if (m.edges[j - 1] >= m.edges[j]) throw GxError(GX_E_ARG, name + ": a measure's edges are not strictly ascending");
        n_edges += m.n_edges;
    }
    if (n_edges > STATS_MAX_EDGES_TOTAL) throw GxError(GX_E_LIMIT, name + ": more than 1024 edges in all");
    std::stable_sort(img.order.begin(), img.order.end(), [&](uint32_t a, uint32_t b) { return measures[a].extraction < measures[b].extraction; });
    std::vector<uint32_t> hist_at(n_measures);   // (the bins lie in the caller's order)
    for (uint32_t t = 0; t < n_measures; ++t) {
        hist_at[t] = img.n_bins;
        img.n_bins += measures[t].n_edges + 1u;
    }
    img.bytes.assign((sizeof(StatsHead) + n_edges * 8 + 15) & ~static_cast<size_t>(15), 0);
    StatsHead head{};
    head.n_measures = n_measures;
    head.n_edges = static_cast<uint32_t>(n_edges);
    head.n_bins = img.n_bins;
    uint8_t* edges = img.bytes.data() + sizeof(StatsHead);
    size_t at = 0;
    for (uint32_t q = 0; q < n_measures; ++q) {
        const gx_measure& m = measures[img.order[q]];
        if (head.n_ext == 0 || head.ext[head.n_ext - 1] != static_cast<uint32_t>(m.extraction)) {
            head.ext[head.n_ext] = static_cast<uint32_t>(m.extraction);
            head.first[head.n_ext++] = static_cast<uint8_t>(q);
        }
        StatsMeasure& d = head.m[q];
        d.group = static_cast<uint16_t>(m.group);
        d.n_edges = static_cast<uint8_t>(m.n_edges);   // (<= STATS_MAX_EDGES)
        d.fmt = h->number_format_of(m.extraction, m.group);
        if (d.fmt) img.formats = true;
        d.edge_at = static_cast<uint16_t>(at);
        d.hist_at = static_cast<uint16_t>(hist_at[img.order[q]]);
        if (m.n_edges) memcpy(edges + at * 8, m.edges, static_cast<size_t>(m.n_edges) * 8);
        at += m.n_edges;
    }
    head.first[head.n_ext] = static_cast<uint8_t>(n_measures);
    memcpy(img.bytes.data(), &head, sizeof(head));
    return img;
}

// The reduction on the handle's buffers (under h->mu) and, with counts, the histogram of outcomes beside it (k_select_flags' counting
// form); then ONE synchronisation of the stream, where the host reads the summed words.
static void stats_pass(gx_handle* h, const BatchView& v, const StatsImage& si, const WhereImage& wi, uint32_t n_measures, gx_measure_stats* stats, uint64_t* hist,
                       uint64_t* counts, hipStream_t stream) {
    const uint32_t K = static_cast<uint32_t>(h->T.n_rules);
    const uint64_t n = v.n;
    if (counts) counts_beside(h, v, counts, stream);
    const size_t words = static_cast<size_t>(n_measures) * STATS_WORDS, total = words + si.n_bins;
    std::vector<uint64_t> got(total + 2, 0);   // (the words, the bins, the status word)
    const bool run = n != 0 && n_measures != 0;
    if (run) {
        const DevImage img = upload_image(h->stats_image, si.bytes.data(), si.bytes.size(), nullptr, wi, stream);
        const StatsArgs a{v.data, v.wide ? 1 : 0, v.caps, 2u * static_cast<uint32_t>(h->T.max_groups), img.head, static_cast<uint32_t>(si.bytes.size()),
                          img.terms, static_cast<uint32_t>(wi.bytes.size()), n_measures, si.n_bins,
                          (si.formats || wi.formats) ? 1u : 0u};
        void* ws = h->stats_ws.get(stats_workspace_bytes(n, n_measures, si.n_bins));
        GX_HIP(launch_capture_stats(v.ids, v.fmt, v.row_units, K, n, v.offsets, v.off64 ? 1 : 0, a, ws, stream));
        GX_HIP(hipMemcpyAsync(got.data(), ws, (total + 2) * 8, hipMemcpyDeviceToHost, stream));
    }
    GX_HIP(hipStreamSynchronize(stream));
    if (got[total] & 0xFFFFFFFFull) throw GxError(GX_E_LIMIT, "a line of 4 G code units or more cannot be measured");
    for (uint32_t q = 0; q < n_measures; ++q) {
        gx_measure_stats& s = stats[si.order[q]];
        const uint64_t* w = got.data() + static_cast<size_t>(q) * STATS_WORDS;
        s.numbers = w[STATS_W_NUMBERS];
        s.unset = w[STATS_W_UNSET];
        s.not_numbers = w[STATS_W_NOT_NUMBERS];
        s.lines = s.numbers + s.unset + s.not_numbers;
        s.min = run ? static_cast<int64_t>(w[STATS_W_MIN]) : STATS_INT64_MAX;
        s.max = run ? static_cast<int64_t>(w[STATS_W_MAX]) : STATS_INT64_MIN;
        stats_sum128(w[STATS_W_LO], static_cast<int64_t>(w[STATS_W_HI]), &s.sum_lo, &s.sum_hi);
    }
    if (hist)
        for (uint32_t b = 0; b < si.n_bins; ++b) hist[b] = got[words + b];
}

// what both capture-stats calls refuse before they look at the device
static void stats_refusals(const gx_handle* h, const gx_batch_opts& o, const gx_measure* measures, uint32_t n_measures, const gx_where_term* terms,
                           uint32_t n_terms, bool wide, const gx_measure_stats* stats, const std::string& name, StatsImage* si, WhereImage* wi) {
    if (n_measures && !stats) throw GxError(GX_E_ARG, name + ": stats is NULL");
    *si = stats_image(h, measures, n_measures, name);
    if (o.utf8 == 2) throw GxError(GX_E_ARG, name + ": gx_batch_opts.utf8 = 1 (values are read in the units the offsets count)");
    *wi = where_image(h, terms, n_terms, wide, name);
    if (o.no_sync) throw GxError(GX_E_ARG, name + ": no_sync: the results are host values");
}

int gx_capture_stats(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps, const gx_measure* measures,
                     uint32_t n_measures, const gx_where_term* terms, uint32_t n_terms, gx_measure_stats* stats, uint64_t* hist, const gx_batch_opts* opts) {
    const std::string name = "gx_capture_stats";
    return guarded([&]() -> int {
        if (!h || !offsets || (n && !ids)) return fail(GX_E_ARG, name + ": bad argument");
        const gx_batch_opts o = read_opts(opts);
        uint32_t row_units = 1;
        const RowFormat fmt = id_format(h, o, &row_units);
        StatsImage si;
        WhereImage wi;
        stats_refusals(h, o, measures, n_measures, terms, n_terms, o.utf16 != 0, stats, name, &si, &wi);
        if ((n_measures || !wi.none()) && fmt == ROWS_DENSE && n && !caps) return fail(GX_E_ARG, name + ": measures and terms on dense ids need caps");
        if (!h->on_device) return fail(GX_E_DEVICE, "handle was created host-only; no device tables (there is no CPU fallback)");
        if (n >= (1ull << 32)) return fail(GX_E_LIMIT, name + ": line numbers are 32 bits; split batches of 4 G lines and more");
        if (fmt != ROWS_DENSE) caps = nullptr;
        GX_HIP(hipSetDevice(h->device));
        std::lock_guard<std::mutex> lock(h->mu);
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        const StagedLines in = stage_lines(h, bytes, offsets, n, ids, caps, o, fmt, row_units, Travels{true, caps != nullptr}, stream, name.c_str());
        stats_pass(h, in.v, si, wi, n_measures, stats, hist, nullptr, stream);
        return GX_OK;
    });
}

int gx_text_capture_stats(gx_handle* h, const uint8_t* text, uint64_t size, const gx_measure* measures, uint32_t n_measures, const gx_where_term* terms,
                          uint32_t n_terms, gx_measure_stats* stats, uint64_t* hist, uint64_t* counts, uint64_t* n_lines, const gx_batch_opts* opts) {
    const std::string name = "gx_text_capture_stats";
    return guarded([&]() -> int {
        if (!h || (size && !text)) return fail(GX_E_ARG, name + ": bad argument");
        const gx_batch_opts o = read_opts(opts);
        StatsImage si;
        WhereImage wi;
        stats_refusals(h, o, measures, n_measures, terms, n_terms, false, stats, name, &si, &wi);
        if (size > 0xFFFFFFFFull) return fail(GX_E_LIMIT, name + ": split texts of 4 GiB and more at a line boundary");
        if (!h->on_device) return fail(GX_E_DEVICE, "handle was created host-only; no device tables (there is no CPU fallback)");
        GX_HIP(hipSetDevice(h->device));
        std::lock_guard<std::mutex> lock(h->mu);
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        // the text's lines and the path; then the reduction over the ids, offsets and capture rows they left on the device
        const TextBatch tb = stage_text_lines(h, text, size, o, stream, name.c_str());
        stats_pass(h, tb.v, si, wi, n_measures, stats, hist, counts, stream);
        if (promise_broken_since(h, stream)) throw GxError(GX_E_ARG, "internal: " + name + ": a line longer than the split pass reported");
        if (n_lines) *n_lines = tb.v.n;
        return GX_OK;
    });
}

// The parts of a gx_group_lines call as its kernels read them (gx_group.hpp: GroupHead), checked against the handle.  Needs no device.
struct GroupImage {
    GroupHead head{};
    bool values = false;
};
static GroupImage group_image(const gx_handle* h, const gx_group_part* parts, uint32_t n_parts, uint32_t flags, const std::string& name) {
    GroupImage img;
    if (flags & ~static_cast<uint32_t>(GX_GROUP_WEAK_HASH)) throw GxError(GX_E_ARG, name + ": unknown flag bits");
    img.head.flags = flags;
    if (n_parts == 0) return img;
    if (!parts) throw GxError(GX_E_ARG, name + ": parts is NULL");
    if (n_parts > GROUP_MAX_PARTS) throw GxError(GX_E_LIMIT, name + ": more than 64 parts");
    const int32_t K = static_cast<int32_t>(h->T.n_rules);
    std::vector<uint32_t> order(n_parts);
    for (uint32_t t = 0; t < n_parts; ++t) {
        const gx_group_part& p = parts[t];
        order[t] = t;
        if (p.extraction < 0 || p.extraction >= K) throw GxError(GX_E_ARG, name + ": a part's extraction is not in [0, K)");
        const int32_t groups = gx_num_groups(h, p.extraction);
        if (p.key_group < 0 || p.key_group >= groups) throw GxError(GX_E_ARG, name + ": a part's key_group is not one of its extraction's");
        if (p.value_group < -1 || p.value_group >= groups) throw GxError(GX_E_ARG, name + ": a part's value_group is neither -1 nor one of its extraction's");
        if (p.reserved != 0) throw GxError(GX_E_ARG, name + ": a part's reserved is not 0");
        if (p.value_group >= 0) img.values = true;
    }
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return parts[a].extraction < parts[b].extraction; });
    for (uint32_t q = 0; q < n_parts; ++q) {
        const gx_group_part& p = parts[order[q]];
        if (q && parts[order[q - 1]].extraction == p.extraction) throw GxError(GX_E_ARG, name + ": two parts for one extraction");
        img.head.ext[q] = static_cast<uint32_t>(p.extraction);
        img.head.part[q].key_group = static_cast<uint16_t>(p.key_group);
        img.head.part[q].value_group = p.value_group < 0 ? static_cast<uint16_t>(GROUP_NO_VALUE) : static_cast<uint16_t>(p.value_group);
        if (p.value_group >= 0) img.head.fmt[q] = h->number_format_of(p.extraction, p.value_group);
        if (img.head.fmt[q]) img.head.formats = 1u;
    }
    img.head.n_parts = n_parts;
    img.head.has_values = img.values ? 1u : 0u;
    return img;
}

// what both group calls refuse before they look at the device
static void group_refusals(const gx_handle* h, const gx_batch_opts& o, const gx_group_part* parts, uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms,
                           uint32_t flags, bool wide, const gx_group_out& out, const gx_group_totals* totals, const std::string& name, GroupImage* gi,
                           WhereImage* wi) {
    if (!totals) throw GxError(GX_E_ARG, name + ": totals is NULL");
    *gi = group_image(h, parts, n_parts, flags, name);
    if (out.key_stats && !gi->values) throw GxError(GX_E_ARG, name + ": key_stats without a value_group");
    if (o.utf8 == 2) throw GxError(GX_E_ARG, name + ": gx_batch_opts.utf8 = 1 (values are read in the units the offsets count)");
    *wi = where_image(h, terms, n_terms, wide, name);
    if (o.no_sync) throw GxError(GX_E_ARG, name + ": no_sync: the totals are host values");
    if (out.max_keys > GROUP_MAX_KEYS) throw GxError(GX_E_LIMIT, name + ": max_keys above 2^30");
}

// gx_group_lines' build as group_pass and top_groups_pass run it, on the handle's buffers (under h->mu).  enqueue(): the wait for the
// workspace's last user, the image, then the build, flags and scans.  ask(): the reads of what they left, enqueued last before the
// caller's wait (a read into pageable memory holds the host up until the stream has come that far: what else the caller has to launch
// goes first).  read(), behind that wait: the totals and the refusals that follow from them.  The object stays where it is from ask()
// to the wait: the reads are into its members.
struct GroupBuild {
    GroupArgs a{};
    GroupWs w{};
    uint32_t n_slots = 0;
    uint64_t got[8] = {0, 0, 0, 0, 0, 0, 0, 0}, n_keys = 0, key_units = 0;
    GroupBuild() = default;
    GroupBuild(const GroupBuild&) = delete;
    GroupBuild& operator=(const GroupBuild&) = delete;
    void enqueue(gx_handle* h, const BatchView& v, const GroupImage& gi, const WhereImage& wi, uint64_t max_keys, hipStream_t stream) {
        wait_pending(h->group_event, h->group_pending, stream);
        n_slots = group_slots(max_keys);
        const DevImage img = upload_image(h->group_image, &gi.head, sizeof(GroupHead), nullptr, wi, stream);
        a = GroupArgs{v.data, v.wide ? 1 : 0, v.caps, 2u * static_cast<uint32_t>(h->T.max_groups), img.head, img.terms,
                      static_cast<uint32_t>(wi.bytes.size()), gi.values ? 1u : 0u, (gi.head.formats || wi.formats) ? 1u : 0u};
        w = group_workspace(h->group_table.get(group_table_bytes(n_slots, gi.values)), h->group_lines.get(group_lines_bytes(v.n)), v.n, n_slots, gi.values);
        GX_HIP(launch_group_build(v.ids, v.fmt, v.row_units, static_cast<uint32_t>(h->T.n_rules), v.n, v.offsets, v.off64 ? 1 : 0, a, w, stream));
    }
    void ask(uint64_t n, hipStream_t stream) {
        GX_HIP(hipMemcpyAsync(got, w.totals, sizeof(got), hipMemcpyDeviceToHost, stream));
        GX_HIP(hipMemcpyAsync(&n_keys, w.idx_off + n, 8, hipMemcpyDeviceToHost, stream));
        GX_HIP(hipMemcpyAsync(&key_units, w.dst_off + n, 8, hipMemcpyDeviceToHost, stream));
    }
    int read(gx_group_totals* totals, const std::string& name) const {
        if (got[2] & 1u) throw GxError(GX_E_LIMIT, "a line of 4 G code units or more cannot be grouped");
        totals->lines = got[0];
        totals->unset = got[1];
        totals->keyed = got[0] - got[1];
        totals->n_keys = n_keys;
        totals->key_units = key_units;
        if (got[2] & 2u) {
            totals->exact = 0;
            totals->n_keys = static_cast<uint64_t>(n_slots) + 1u;
            return fail(GX_E_LIMIT, name + ": the table of " + std::to_string(n_slots) + " slots is full; the number of lines is always a sufficient max_keys");
        }
        return GX_OK;
    }
};

// What every step of a group_pass call reads: the call's arguments and its build.
struct GroupCtx {
    gx_handle* h;
    const BatchView& v;
    const WhereImage& wi;
    bool values, out64, host_out;   // values: a part has a value group
    uint64_t max_keys;
    const gx_group_totals* totals;
    hipStream_t stream;
    const std::string& name;
    GroupBuild b;
    uint32_t K() const { return static_cast<uint32_t>(h->T.n_rules); }
};

// What a call built on gx_group_lines adds to group_pass: its arguments (GroupQuant, ByKeyCall, PairsCall, SeriesCall, SessionsCall, SpansCall, WindowsCall) and, beside each,
// what it keeps while the pass runs (…Run; call == nullptr: not that call), whose steps group_pass takes in this order:
//   start()    the call's own totals as they are when nothing has run
//   nothing()  no lines or no parts: the results that no kernel writes
//   enqueue()  behind the build and before the ONE wait: the call's own passes and the reads of what they leave
//   read()     behind the wait: the totals, the checks that they add up, the refusal of a full table
//   fits()     the refusals of capacities that are smaller than the result
//   emit()     behind launch_group_emit: the call's outputs, those of a host caller by way of the pass' twins
// A step that a call does not need is not there.

// gq (gx_group_quantiles; nullptr or n_q == 0: gx_group_lines as it is): before the read of the totals also the candidates' pairs, their
// number and the OR and AND of their value keys (launch_gq_collect), read in the same wait; behind the emit the sort by the digit
// plan made from them and the pick.
struct GroupQuant {
    const gx_quantile* quantiles = nullptr;
    uint32_t n_quantiles = 0;
    gx_quantile_out* rows = nullptr;   // the caller's, device or host as the other per-key arrays; nullptr: not wanted
    TopHead ti{};                 // (gq_refusals) the parts that have a value group
    QuantHead qh{};
};
static_assert(sizeof(gx_quantile_out) == sizeof(QuantOut), "the rows are copied as they are");
struct GroupQuantRun {
    const GroupQuant* call;
    gx_quantile_out* rows;   // where the rows go; nullptr: none are wanted
    bool sort;               // the candidates are collected: only where rows are wanted and a part has a value (else every population is empty)
    GqWs qw{};
    GqDev qd{};
    uint8_t* d_qh = nullptr;   // the QuantHead on the device
    explicit GroupQuantRun(const GroupQuant* gq) : call(gq), rows(gq && gq->qh.n_q ? gq->rows : nullptr), sort(rows && gq->ti.n_parts != 0) {}
    void enqueue(const GroupCtx& c) {
        const BatchView& v = c.v;
        const DevImage img = upload_image(c.h->gq_image, &call->ti, sizeof(TopHead), &call->qh, c.wi, c.stream);
        d_qh = img.head + sizeof(TopHead);
        const TopArgs ta{v.data, v.wide ? 1 : 0, v.caps, 2u * static_cast<uint32_t>(c.h->T.max_groups), img.head, img.terms,
                         static_cast<uint32_t>(c.wi.bytes.size()), 0u, 0u, c.b.a.formats};
        qw = gq_workspace(c.h->gq_ws.get(gq_workspace_bytes(v.n)), v.n);
        GX_HIP(launch_gq_collect(v.ids, v.fmt, v.row_units, c.K(), v.n, v.offsets, v.off64 ? 1 : 0, ta, c.b.w.slot_of, qw, c.stream));
        GX_HIP(hipMemcpyAsync(&qd, qw.head, sizeof(GqDev), hipMemcpyDeviceToHost, c.stream));
    }
    void emit(const GroupCtx& c, HostTwins& twins) const {
        const uint32_t n_q = call->qh.n_q;
        const size_t rows_bytes = static_cast<size_t>(c.b.n_keys) * n_q * sizeof(QuantOut);
        if (!rows_bytes) return;
        void* d_rows = twins.of(rows, rows_bytes);
        if (sort && qd.candidates != 0) {
            const GqPlan plan = gq_plan(qd.value_or ^ qd.value_and, c.b.n_keys, gq_sorts_all_digits());
            GX_HIP(launch_gq_sort_pick(qw, qd.candidates, plan, c.b.w.keynum, c.b.w.n_slots, d_qh, n_q, c.b.n_keys, d_rows, c.stream));
        } else {
            GX_HIP(hipMemsetAsync(d_rows, 0, rows_bytes, c.stream));   // no key has a number
        }
    }
};
// bk (gx_lines_by_key; nullptr: gx_group_lines as it is): before the read of the totals also the kept flags, their scan and the kept
// lines, units and keys (launch_by_key_kept), read in the same wait; behind the emit, which numbers the slots, the compaction, the sort
// by key number, the bounds (launch_by_key_sort) and the copy (launch_partition_copy).
struct ByKeyCall {
    uint64_t min_lines = 0, max_lines = 0;
    bool all_digits = false;
    gx_by_key_out out{};
    gx_by_key_totals* totals = nullptr;   // (its group member is the gx_group_totals the pass fills)
    bool per_line() const { return out.out_index || out.out_offsets || out.out_ids || out.out_caps; }
    bool any() const { return per_line() || out.out_bytes || out.key_out_lines || out.key_out_units; }
};
struct ByKeyRun {
    const ByKeyCall* call;
    ByKeyWs bw{};
    ByKeyDev bd{};
    StagedLinesOut lines;   // the kept lines' outputs (their twins are its own, and live as long as this object)
    explicit operator bool() const { return call != nullptr; }
    void start() const { *call->totals = gx_by_key_totals{}; }
    void nothing(const GroupCtx& c) const {   // no kept lines: the one entry of the offsets and of the two prefixes
        fill_out(call->out.out_offsets, 0, c.v.off64 ? 8 : 4, c.host_out, c.stream);
        fill_out(call->out.key_out_lines, 0, 8, c.host_out, c.stream);
        fill_out(call->out.key_out_units, 0, 8, c.host_out, c.stream);
    }
    // the kept lines, their units and their keys: from the slots' line counts, which the build has left complete
    void enqueue(const GroupCtx& c) {
        const uint64_t n = c.v.n;
        bw = by_key_workspace(c.h->by_key_ws.get(by_key_workspace_bytes(n)), n);
        GX_HIP(launch_by_key_kept(n, c.v.offsets, c.v.off64 ? 1 : 0, c.b.w, call->min_lines, call->max_lines, bw, c.stream));
        GX_HIP(hipMemcpyAsync(&bd, bw.head, sizeof(ByKeyDev), hipMemcpyDeviceToHost, c.stream));
    }
    void read(const GroupCtx& c) const {
        if (bd.lines_out > c.v.n || bd.keys_kept > c.b.n_keys) throw GxError(GX_E_ARG, "internal: " + c.name + ": more kept lines or keys than there are");
        call->totals->keys_kept = bd.keys_kept;
        call->totals->lines_out = bd.lines_out;
        call->totals->units_out = bd.units_out;
    }
    int fits(const GroupCtx& c) const {
        const gx_by_key_out& b = call->out;
        const std::string& name = c.name;
        const size_t unit = c.v.wide ? 2 : 1;
        if (call->per_line() && bd.lines_out > b.cap_lines) return fail(GX_E_LIMIT, name + ": cap_lines is smaller than the result (see totals->lines_out)");
        if (b.out_bytes && bd.units_out * unit > b.out_bytes_cap) return fail(GX_E_LIMIT, name + ": the kept text is larger than the capacity (see totals->units_out)");
        if (b.out_offsets && !c.v.off64 && bd.units_out > 0xFFFFFFFFull) return fail(GX_E_LIMIT, name + ": 4 G code units and more need offsets64");
        if ((b.key_out_lines || b.key_out_units) && c.b.n_keys > c.max_keys)
            return fail(GX_E_LIMIT, name + ": " + std::to_string(c.b.n_keys) + " keys, max_keys " + std::to_string(c.max_keys));
        return GX_OK;
    }
    // the kept lines by (key number, line) as a new batch, and the keys' bounds in it
    void emit(const GroupCtx& c, HostTwins& twins) {
        const gx_by_key_out& b = call->out;
        const BatchView& v = c.v;
        const uint64_t n = v.n, m = bd.lines_out, n_keys = c.b.n_keys;
        lines = stage_lines_out(c.h, v, LinesOut{b.out_index, b.out_bytes, b.out_offsets, b.out_ids, b.out_caps}, c.host_out, m, bd.units_out);
        uint64_t* kol = twins.of(b.key_out_lines, (n_keys + 1) * 8);
        uint64_t* kou = twins.of(b.key_out_units, (n_keys + 1) * 8);
        if (m == 0) {
            if (lines.dev.offsets) GX_HIP(hipMemsetAsync(lines.dev.offsets, 0, v.off64 ? 8 : 4, c.stream));
            if (kol) GX_HIP(hipMemsetAsync(kol, 0, (n_keys + 1) * 8, c.stream));
            if (kou) GX_HIP(hipMemsetAsync(kou, 0, (n_keys + 1) * 8, c.stream));
        } else {
            PartWs pw{};   // (the copy pass reads the permutation and the output offsets alone)
            GX_HIP(launch_by_key_sort(n, m, n_keys, by_key_passes(n_keys, call->all_digits), c.b.w, bw, kol, kou, &pw.perm_sorted, c.stream));
            pw.dst_off = bw.dst_off;
            GX_HIP(launch_partition_copy(lines.dev, v.data, v.offsets, v.off64 ? 1 : 0, v.wide ? 1 : 0, n, m, pw, c.stream));
        }
    }
};
// pc (gx_group_pairs; nullptr: gx_group_lines as it is): behind the build the pair table's build, flags and scans (launch_pairs_build),
// whose totals, pairs and units are read in the same wait; behind the emit, which numbers the key slots, the pair emit.
struct PairsCall {
    const int32_t* second_groups = nullptr;
    const gx_pairs_out* asked = nullptr;   // the caller's; nullptr: the keys alone, no pair table
    gx_pairs_totals* totals = nullptr;     // (its group member is the gx_group_totals the pass fills)
    PairsHead head{};                      // (pairs_refusals) the second group per entry of GroupHead::ext[]
    bool any_second = false;
    gx_pairs_out out{};
    bool per_pair() const { return out.pair_offsets || out.pair_key || out.pair_first_line || out.pair_lines; }
    bool any() const { return per_pair() || out.pair_units || out.key_pairs || out.line_pair; }
};
struct PairsRun {
    const PairsCall* call;
    PairsWs pw{};
    PairsDev pd{};
    uint64_t n_pairs = 0, pair_units = 0;
    uint8_t* d_img = nullptr;   // the PairsHead on the device
    explicit operator bool() const { return call != nullptr; }
    void start() const {
        *call->totals = gx_pairs_totals{};
        call->totals->pairs_exact = 1;
    }
    void nothing(const GroupCtx& c) const {   // no pairs: the offsets' one entry and every line's "none"
        fill_out(call->out.pair_offsets, 0, c.out64 ? 8 : 4, c.host_out, c.stream);
        fill_out(call->out.line_pair, 0xFF, c.v.n * 4, c.host_out, c.stream);
    }
    // a second table keyed by (key slot, second text), behind the build that has left slot_of[] complete
    void enqueue(const GroupCtx& c) {
        const BatchView& v = c.v;
        const uint32_t p_slots = group_slots(call->out.max_pairs);
        d_img = static_cast<uint8_t*>(c.h->pairs_image.get(sizeof(PairsHead)));
        GX_HIP(hipMemcpyAsync(d_img, &call->head, sizeof(PairsHead), hipMemcpyHostToDevice, c.stream));
        pw = pairs_workspace(c.h->pairs_table.get(pairs_table_bytes(p_slots, c.b.n_slots)), c.h->pairs_lines.get(pairs_lines_bytes(v.n)), v.n, p_slots, c.b.n_slots);
        GX_HIP(launch_pairs_build(v.ids, v.fmt, v.row_units, c.K(), v.n, v.offsets, v.off64 ? 1 : 0, c.b.a, d_img, c.b.w, pw, c.stream));
        GX_HIP(hipMemcpyAsync(&pd, pw.totals, sizeof(PairsDev), hipMemcpyDeviceToHost, c.stream));
        GX_HIP(hipMemcpyAsync(&n_pairs, pw.idx_off + v.n, 8, hipMemcpyDeviceToHost, c.stream));
        GX_HIP(hipMemcpyAsync(&pair_units, pw.dst_off + v.n, 8, hipMemcpyDeviceToHost, c.stream));
    }
    int read(const GroupCtx& c) const {
        gx_pairs_totals& t = *call->totals;
        if (pd.paired + pd.unpaired != c.totals->keyed) throw GxError(GX_E_ARG, "internal: " + c.name + ": paired and unpaired lines do not add up to the keyed lines");
        t.paired = pd.paired;
        t.unpaired = pd.unpaired;
        t.n_pairs = n_pairs;
        t.pair_units = pair_units;
        if (pd.status & 2u) {
            t.pairs_exact = 0;
            t.n_pairs = static_cast<uint64_t>(pw.n_slots) + 1u;
            return fail(GX_E_LIMIT, c.name + ": the pair table of " + std::to_string(pw.n_slots) + " slots is full; the number of lines is always a sufficient max_pairs");
        }
        return GX_OK;
    }
    int fits(const GroupCtx& c) const {
        const gx_pairs_out& b = call->out;
        const std::string& name = c.name;
        if (call->per_pair() && n_pairs > b.max_pairs) return fail(GX_E_LIMIT, name + ": " + std::to_string(n_pairs) + " pairs, max_pairs " + std::to_string(b.max_pairs));
        if (b.pair_units && pair_units > b.pair_units_cap)
            return fail(GX_E_LIMIT, name + ": " + std::to_string(pair_units) + " pair units, pair_units_cap " + std::to_string(b.pair_units_cap));
        if (b.pair_offsets && !c.out64 && pair_units > 0xFFFFFFFFull) return fail(GX_E_LIMIT, name + ": 4 G pair units and more need offsets64");
        if (b.key_pairs && c.b.n_keys > c.max_keys) return fail(GX_E_LIMIT, name + ": " + std::to_string(c.b.n_keys) + " keys, max_keys " + std::to_string(c.max_keys));
        return GX_OK;
    }
    // the pairs' rows, their seconds, the keys' pairs and the lines' pair numbers
    void emit(const GroupCtx& c, HostTwins& twins) const {
        const gx_pairs_out& b = call->out;
        const BatchView& v = c.v;
        const size_t unit = v.wide ? 2 : 1, off_w = c.out64 ? 8 : 4;
        const uint64_t n = v.n, n_keys = c.b.n_keys;
        const PairsOut po{twins.of(b.pair_units, pair_units * unit), twins.of(b.pair_offsets, (n_pairs + 1) * off_w), twins.of(b.pair_key, n_pairs * 4),
                          twins.of(b.pair_first_line, n_pairs * 4), twins.of(b.pair_lines, n_pairs * 8), twins.of(b.key_pairs, n_keys * 8),
                          twins.of(b.line_pair, n * 4), c.out64 ? 1 : 0};
        GX_HIP(launch_pairs_emit(v.ids, v.fmt, v.row_units, c.K(), n, v.offsets, v.off64 ? 1 : 0, c.b.a, d_img, c.b.w, pw, po, n_pairs, pair_units, n_keys, c.stream));
    }
};
// sc (gx_group_series; nullptr: gx_group_lines as it is): behind the build the bucket table's and the cell table's build, flags and scans
// (launch_series_build), whose totals, buckets and cells are read in the same wait -- both sorts' digits follow from numbers known
// there; behind the emit, which numbers the key slots, the two sorts and the series' emits.
struct SeriesCall {
    const int32_t* number_groups = nullptr;
    int64_t origin = 0, width = 0;
    bool all_digits = false;
    const gx_series_out* asked = nullptr;   // the caller's; nullptr: the keys alone, no series tables
    gx_series_totals* totals = nullptr;     // (its group member is the gx_group_totals the pass fills)
    SeriesHead head{};                      // (series_refusals) the number group per entry of GroupHead::ext[]
    bool any_number = false;
    gx_series_out out{};
    bool per_cell() const { return out.cell_key || out.cell_bucket || out.cell_first_line || out.cell_lines || out.cell_stats; }
    bool any() const { return per_cell() || out.bucket_number || out.key_cell_begin || out.line_cell; }
};
struct SeriesRun {
    const SeriesCall* call;
    SeriesWs sw{};
    SeriesDev sd{};
    uint64_t n_buckets = 0, n_cells = 0, min_word = 0, max_word = 0;
    explicit operator bool() const { return call != nullptr; }
    void start() const {
        *call->totals = gx_series_totals{};
        call->totals->cells_exact = 1;
    }
    void nothing(const GroupCtx& c) const {   // no cells: the bounds' one entry and every line's "none"
        fill_out(call->out.key_cell_begin, 0, 8, c.host_out, c.stream);
        fill_out(call->out.line_cell, 0xFF, c.v.n * 4, c.host_out, c.stream);
    }
    // a table of the buckets and a table of (key slot, bucket slot), behind the build that has left slot_of[]
    void enqueue(const GroupCtx& c) {
        const BatchView& v = c.v;
        const uint32_t s_slots = group_slots(call->out.max_cells);
        const size_t at_table = (sizeof(SeriesHead) + 15) & ~static_cast<size_t>(15);
        uint8_t* d_img = static_cast<uint8_t*>(c.h->series_table.get(at_table + series_table_bytes(s_slots, c.values)));
        GX_HIP(hipMemcpyAsync(d_img, &call->head, sizeof(SeriesHead), hipMemcpyHostToDevice, c.stream));
        sw = series_workspace(d_img + at_table, c.h->series_lines.get(series_lines_bytes(v.n)), s_slots, c.values);
        GX_HIP(launch_series_build(v.ids, v.fmt, v.row_units, c.K(), v.n, v.offsets, v.off64 ? 1 : 0, c.b.a, d_img, c.b.a.formats != 0 || call->head.formats != 0, c.b.w, sw,
                                   c.stream));
        GX_HIP(hipMemcpyAsync(&sd, sw.totals, sizeof(SeriesDev), hipMemcpyDeviceToHost, c.stream));
        GX_HIP(hipMemcpyAsync(&n_buckets, sw.bbefore + s_slots, 8, hipMemcpyDeviceToHost, c.stream));
        GX_HIP(hipMemcpyAsync(&n_cells, sw.cbefore + s_slots, 8, hipMemcpyDeviceToHost, c.stream));
    }
    int read(const GroupCtx& c) {
        gx_series_totals& t = *call->totals;
        t.celled = sd.celled;
        t.number_unset = sd.number_unset;
        t.not_numbers = sd.not_numbers;
        t.out_of_range = sd.out_of_range;
        t.n_cells = n_cells;
        t.n_buckets = n_buckets;
        min_word = ~sd.min_inv;
        max_word = sd.max_word;
        if (n_buckets) {
            t.first_bucket = bucket_number(min_word);
            t.last_bucket = bucket_number(max_word);
        }
        if (sd.status & 2u) {
            t.cells_exact = 0;
            t.n_cells = static_cast<uint64_t>(sw.n_slots) + 1u;
            return fail(GX_E_LIMIT, c.name + ": a series table of " + std::to_string(sw.n_slots) + " slots is full; the number of lines is always a sufficient max_cells");
        }
        if (sd.celled + sd.number_unset + sd.not_numbers + sd.out_of_range != c.totals->keyed)
            throw GxError(GX_E_ARG, "internal: " + c.name + ": the classes of the keyed lines do not add up to them");
        if (n_buckets > n_cells || n_cells > sd.celled) throw GxError(GX_E_ARG, "internal: " + c.name + ": more buckets than cells, or more cells than celled lines");
        return GX_OK;
    }
    int fits(const GroupCtx& c) const {
        const gx_series_out& b = call->out;
        const std::string& name = c.name;
        if (call->per_cell() && n_cells > b.max_cells) return fail(GX_E_LIMIT, name + ": " + std::to_string(n_cells) + " cells, max_cells " + std::to_string(b.max_cells));
        if (b.bucket_number && n_buckets > b.max_buckets)
            return fail(GX_E_LIMIT, name + ": " + std::to_string(n_buckets) + " buckets, max_buckets " + std::to_string(b.max_buckets));
        if (b.key_cell_begin && c.b.n_keys > c.max_keys) return fail(GX_E_LIMIT, name + ": " + std::to_string(c.b.n_keys) + " keys, max_keys " + std::to_string(c.max_keys));
        return GX_OK;
    }
    // the axis, the cells' rows ordered by (key number, bucket), the keys' bounds and the lines' cells
    void emit(const GroupCtx& c, HostTwins& twins) const {
        const gx_series_out& b = call->out;
        const uint64_t n = c.v.n, n_keys = c.b.n_keys;
        const SeriesOut so{twins.of(b.bucket_number, n_buckets * 8), twins.of(b.cell_key, n_cells * 4), twins.of(b.cell_bucket, n_cells * 4),
                           twins.of(b.cell_first_line, n_cells * 4), twins.of(b.cell_lines, n_cells * 8),
                           twins.of(reinterpret_cast<uint64_t*>(b.cell_stats), n_cells * 64), twins.of(b.key_cell_begin, (n_keys + 1) * 8),
                           twins.of(b.line_cell, n * 4)};
        if (n_cells == 0) {   // keyed lines, and none of them celled: every key's run is empty
            if (so.key_cell_begin) GX_HIP(hipMemsetAsync(so.key_cell_begin, 0, (n_keys + 1) * 8, c.stream));
            if (so.line_cell) GX_HIP(hipMemsetAsync(so.line_cell, 0xFF, n * 4, c.stream));
        } else {
            const uint32_t b_digits = call->all_digits ? BUCKET_MAX_DIGITS : bucket_digits(min_word, max_word);
            const uint32_t c_digits = call->all_digits ? BUCKET_MAX_DIGITS : series_digits(n_keys, n_buckets);
            const SeriesSortWs ssw = series_sort_workspace(c.h->series_sort.get(series_sort_workspace_bytes(n_cells)), n_cells);
            GX_HIP(launch_series_emit(n, n_keys, n_buckets, n_cells, b_digits, c_digits, c.b.w, sw, ssw, so, c.stream));
        }
    }
};
// ss (gx_group_sessions; nullptr: gx_group_lines as it is): behind the build the keys pass and its scan (launch_sessions_keys), whose
// classes, entries and time words' OR / AND / range are read in the group's wait.  n_sessions exists only behind the two sorts, so
// read() enqueues them with the heads, their scan and the longest session (launch_sessions_sort) and takes the call's ONE further wait --
// before launch_group_emit: a key's number is known from the build, and a capacity can be refused before any output is written.
struct SessionsCall {
    const int32_t* number_groups = nullptr;
    int64_t max_gap = 0;
    bool all_digits = false;
    const gx_sessions_out* asked = nullptr;   // the caller's; nullptr: the keys alone, no session passes
    gx_sessions_totals* totals = nullptr;     // (its group member is the gx_group_totals the pass fills)
    SessionsHead head{};                      // (sessions_refusals) the number group per entry of GroupHead::ext[]
    bool any_number = false;
    gx_sessions_out out{};
    bool per_session() const {
        return out.session_key || out.session_begin || out.session_end || out.session_first_line || out.session_lines || out.session_stats ||
               out.session_entry_begin;
    }
    bool any() const { return per_session() || out.key_session_begin || out.entry_line || out.line_session; }
};
struct SessionsRun {
    const SessionsCall* call;
    SessionsWs sw{};
    SessionsSortWs ssw{};
    SessionsDev sd{};
    SessionsDev2 sd2{};
    uint32_t time_buf = 0, key_buf = 0;
    explicit operator bool() const { return call != nullptr; }
    void start() const { *call->totals = gx_sessions_totals{}; }
    void nothing(const GroupCtx& c) const {   // no sessions: the bounds' one entry and every line's "none"
        fill_out(call->out.session_entry_begin, 0, 8, c.host_out, c.stream);
        fill_out(call->out.key_session_begin, 0, 8, c.host_out, c.stream);
        fill_out(call->out.line_session, 0xFF, c.v.n * 4, c.host_out, c.stream);
    }
    void enqueue(const GroupCtx& c) {
        const BatchView& v = c.v;
        sw = sessions_workspace(c.h->sessions_lines.get(sessions_workspace_bytes(v.n, c.values)), v.n, c.values);
        GX_HIP(hipMemcpyAsync(sw.image, &call->head, sizeof(SessionsHead), hipMemcpyHostToDevice, c.stream));
        GX_HIP(launch_sessions_keys(v.ids, v.fmt, v.row_units, c.K(), v.n, v.offsets, v.off64 ? 1 : 0, c.b.a, c.b.a.formats != 0 || call->head.formats != 0, c.b.w, sw,
                                    c.stream));
        GX_HIP(hipMemcpyAsync(&sd, sw.dev, sizeof(SessionsDev), hipMemcpyDeviceToHost, c.stream));
    }
    int read(const GroupCtx& c) {
        gx_sessions_totals& t = *call->totals;
        t.entries = sd.entries;
        t.number_unset = sd.number_unset;
        t.not_numbers = sd.not_numbers;
        if (sd.entries + sd.number_unset + sd.not_numbers != c.totals->keyed)
            throw GxError(GX_E_ARG, "internal: " + c.name + ": the classes of the keyed lines do not add up to them");
        if (sd.entries == 0) return GX_OK;
        t.first_time = top_value(~sd.min_inv, false);
        t.last_time = top_value(sd.max_word, false);
        if (sd.entries > SESSIONS_MAX) return fail(GX_E_LIMIT, c.name + ": " + std::to_string(sd.entries) + " entries; split batches of more than 2^30");
        const uint64_t m = sd.entries;
        const SortPlan plan = sessions_time_plan(sd.time_or, ~sd.and_inv, m, call->all_digits);
        const bool stats = call->out.session_stats != nullptr;
        ssw = sessions_sort_workspace(c.h->sessions_sort.get(sessions_sort_workspace_bytes(m, stats)), m, stats);
        GX_HIP(launch_sessions_sort(c.v.n, m, plan, sessions_key_digits(c.b.n_keys, call->all_digits), call->max_gap, c.b.w, sw, ssw, &time_buf, &key_buf, c.stream));
        GX_HIP(hipMemcpyAsync(&sd2, ssw.dev2, sizeof(SessionsDev2), hipMemcpyDeviceToHost, c.stream));
        GX_HIP(hipStreamSynchronize(c.stream));
        if (sd2.n_sessions == 0 || sd2.n_sessions > m) throw GxError(GX_E_ARG, "internal: " + c.name + ": entries without a session, or more sessions than entries");
        t.n_sessions = sd2.n_sessions;
        t.longest_lines = sd2.longest_lines;
        t.longest_duration = sd2.longest_duration;
        return GX_OK;
    }
    int fits(const GroupCtx& c) const {
        const gx_sessions_out& b = call->out;
        const std::string& name = c.name;
        if (call->per_session() && sd2.n_sessions > b.max_sessions)
            return fail(GX_E_LIMIT, name + ": " + std::to_string(sd2.n_sessions) + " sessions, max_sessions " + std::to_string(b.max_sessions));
        if (b.entry_line && sd.entries > b.max_entries)
            return fail(GX_E_LIMIT, name + ": " + std::to_string(sd.entries) + " entries, max_entries " + std::to_string(b.max_entries));
        if (b.key_session_begin && c.b.n_keys > c.max_keys)
            return fail(GX_E_LIMIT, name + ": " + std::to_string(c.b.n_keys) + " keys, max_keys " + std::to_string(c.max_keys));
        return GX_OK;
    }
    // the sessions' rows ordered by (key number, begin), the keys' bounds, the entries' lines and the lines' sessions
    void emit(const GroupCtx& c, HostTwins& twins) const {
        const gx_sessions_out& b = call->out;
        const uint64_t n = c.v.n, n_keys = c.b.n_keys, ns = sd2.n_sessions, m = sd.entries;
        const SessionsOut so{twins.of(b.session_key, ns * 4), twins.of(b.session_begin, ns * 8), twins.of(b.session_end, ns * 8),
                             twins.of(b.session_first_line, ns * 4), twins.of(b.session_lines, ns * 8),
                             twins.of(reinterpret_cast<uint64_t*>(b.session_stats), ns * 64), twins.of(b.session_entry_begin, (ns + 1) * 8),
                             twins.of(b.key_session_begin, (n_keys + 1) * 8), twins.of(b.entry_line, m * 4), twins.of(b.line_session, n * 4)};
        if (m == 0) {   // keyed lines, and none of them an entry: every key's run is empty
            if (so.session_entry_begin) GX_HIP(hipMemsetAsync(so.session_entry_begin, 0, 8, c.stream));
            if (so.key_session_begin) GX_HIP(hipMemsetAsync(so.key_session_begin, 0, (n_keys + 1) * 8, c.stream));
            if (so.line_session) GX_HIP(hipMemsetAsync(so.line_session, 0xFF, n * 4, c.stream));
        } else {
            GX_HIP(launch_sessions_emit(n, m, ns, n_keys, sw, ssw, time_buf, key_buf, so, c.stream));
        }
    }
};
// sp (gx_group_spans; nullptr: gx_group_lines as it is): behind the build the entries pass and its scan (launch_spans_entries), whose
// entries are read in the group's wait.  n_spans exists only behind the sort, so read() enqueues it with the heads and their scans
// (launch_spans_pair) and takes the call's ONE further wait -- before launch_group_emit: a key's number is known from the build, and a
// capacity can be refused before any output is written.
struct SpansCall {
    const int32_t* number_groups = nullptr;
    const uint32_t* roles = nullptr;
    bool all_digits = false;
    const gx_spans_out* asked = nullptr;   // the caller's; nullptr: the keys alone, no span passes
    gx_spans_totals* totals = nullptr;     // (its group member is the gx_group_totals the pass fills)
    SpansHead head{};                      // (spans_refusals) the number group and the role per entry of GroupHead::ext[]
    gx_spans_out out{};
    bool per_span() const {
        return out.span_key || out.span_begin_line || out.span_end_line || out.span_begin || out.span_end || out.span_duration || out.span_class;
    }
    bool per_key() const { return out.key_span_begin || out.key_span_stats || out.key_open_line; }
    bool any() const { return per_span() || per_key() || out.line_span || out.line_state; }
};
struct SpansRun {
    const SpansCall* call;
    SpansWs sw{};
    SpansPairWs pw{};
    SpansDev sd{};
    uint64_t m = 0, n_spans = 0, sums[4] = {0, 0, 0, 0};
    uint32_t buf = 0;
    explicit operator bool() const { return call != nullptr; }
    void start() const { *call->totals = gx_spans_totals{}; }
    void nothing(const GroupCtx& c) const {   // no spans: the bounds' one entry, every line's "none" and state 0
        fill_out(call->out.key_span_begin, 0, 8, c.host_out, c.stream);
        fill_out(call->out.line_span, 0xFF, c.v.n * 4, c.host_out, c.stream);
        fill_out(call->out.line_state, 0, c.v.n, c.host_out, c.stream);
    }
    void enqueue(const GroupCtx& c) {
        const BatchView& v = c.v;
        sw = spans_workspace(c.h->spans_lines.get(spans_workspace_bytes(v.n)), v.n);
        GX_HIP(hipMemcpyAsync(sw.image, &call->head, sizeof(SpansHead), hipMemcpyHostToDevice, c.stream));
        GX_HIP(launch_spans_entries(v.ids, v.fmt, v.row_units, c.K(), v.n, v.offsets, v.off64 ? 1 : 0, c.b.a, call->head.formats != 0, c.b.w, sw, c.stream));
        GX_HIP(hipMemcpyAsync(&m, sw.before + v.n, 8, hipMemcpyDeviceToHost, c.stream));
    }
    int read(const GroupCtx& c) {
        gx_spans_totals& t = *call->totals;
        if (m != c.totals->keyed) throw GxError(GX_E_ARG, "internal: " + c.name + ": the entries are not the keyed lines");
        if (m == 0) return GX_OK;
        if (m > SPANS_MAX) return fail(GX_E_LIMIT, c.name + ": " + std::to_string(m) + " entries; split batches of more than 2^30");
        const uint64_t n_keys = c.b.n_keys;
        pw = spans_pair_workspace(c.h->spans_pair.get(spans_pair_workspace_bytes(m, n_keys)), m, n_keys);
        GX_HIP(launch_spans_pair(c.v.n, m, n_keys, spans_key_digits(n_keys, call->all_digits), c.b.w, sw, pw, &buf, c.stream));
        GX_HIP(hipMemcpyAsync(&sd, pw.dev, sizeof(SpansDev), hipMemcpyDeviceToHost, c.stream));
        GX_HIP(hipMemcpyAsync(&n_spans, pw.sbefore + m, 8, hipMemcpyDeviceToHost, c.stream));
        for (int q = 0; q < 4; ++q) GX_HIP(hipMemcpyAsync(&sums[q], pw.pre[q] + m, 8, hipMemcpyDeviceToHost, c.stream));
        GX_HIP(hipStreamSynchronize(c.stream));
        if (sd.state[SPAN_S_BEGIN] != n_spans || sd.state[SPAN_S_END] != n_spans || n_spans > m / 2)
            throw GxError(GX_E_ARG, "internal: " + c.name + ": the spans' begins and ends do not add up to the spans");
        t.n_spans = n_spans;
        t.superseded = sd.state[SPAN_S_SUPERSEDED];
        t.left_open = sd.state[SPAN_S_OPEN];
        t.orphan_ends = sd.state[SPAN_S_ORPHAN];
        t.begins = n_spans + t.superseded + t.left_open;
        t.ends = n_spans + t.orphan_ends;
        if (t.begins + t.ends != m) throw GxError(GX_E_ARG, "internal: " + c.name + ": the states of the entries do not add up to them");
        t.out_of_range = sums[1] >> 32;
        uint64_t w[GROUP_STATS_WORDS];
        w[GROUP_S_NUMBERS] = sums[0] & 0xFFFFFFFFull;
        w[GROUP_S_UNSET] = sums[0] >> 32;
        w[GROUP_S_NOT_NUMBERS] = sums[1] & 0xFFFFFFFFull;
        w[GROUP_S_MIN] = sd.min_word;
        w[GROUP_S_MAX] = sd.max_word;
        w[GROUP_S_LO] = sums[2];
        w[GROUP_S_HI] = sums[3];
        w[GROUP_S_SPARE] = 0;
        static_assert(sizeof(gx_measure_stats) == 64, "group_stats_out writes its eight words");
        uint64_t st[8];
        group_stats_out(w, st);
        std::memcpy(&t.durations, st, sizeof(st));
        return GX_OK;
    }
    int fits(const GroupCtx& c) const {
        const gx_spans_out& b = call->out;
        const std::string& name = c.name;
        if (call->per_span() && n_spans > b.max_spans) return fail(GX_E_LIMIT, name + ": " + std::to_string(n_spans) + " spans, max_spans " + std::to_string(b.max_spans));
        if (call->per_key() && c.b.n_keys > c.max_keys) return fail(GX_E_LIMIT, name + ": " + std::to_string(c.b.n_keys) + " keys, max_keys " + std::to_string(c.max_keys));
        return GX_OK;
    }
    // the spans' rows ordered by (key number, end line), the keys' bounds, open lines and stats, the lines' spans and states
    void emit(const GroupCtx& c, HostTwins& twins) const {
        const gx_spans_out& b = call->out;
        const uint64_t n = c.v.n, n_keys = c.b.n_keys, ns = n_spans;
        const SpansOut so{twins.of(b.span_key, ns * 4), twins.of(b.span_begin_line, ns * 4), twins.of(b.span_end_line, ns * 4), twins.of(b.span_begin, ns * 8),
                          twins.of(b.span_end, ns * 8), twins.of(b.span_duration, ns * 8), twins.of(b.span_class, ns), twins.of(b.key_span_begin, (n_keys + 1) * 8),
                          twins.of(reinterpret_cast<uint64_t*>(b.key_span_stats), n_keys * 64), twins.of(b.key_open_line, n_keys * 4), twins.of(b.line_span, n * 4),
                          twins.of(b.line_state, n)};
        if (m == 0) {   // counted lines, and none of them keyed: no key, no entry
            if (so.key_span_begin) GX_HIP(hipMemsetAsync(so.key_span_begin, 0, (n_keys + 1) * 8, c.stream));
            if (so.line_span) GX_HIP(hipMemsetAsync(so.line_span, 0xFF, n * 4, c.stream));
            if (so.line_state) GX_HIP(hipMemsetAsync(so.line_state, 0, n, c.stream));
        } else {
            GX_HIP(launch_spans_emit(n, m, ns, n_keys, sw, pw, buf, so, c.stream));
        }
    }
};
// wc (gx_group_windows; nullptr: gx_group_lines as it is): behind the build gx_group_sessions' keys pass and its scan
// (launch_sessions_keys, on the handle's same per-line workspace), read in the group's wait.  The trips exist only behind the two sorts
// and the window pass, so read() enqueues them (launch_windows_pass) and takes the call's ONE further wait -- before launch_group_emit: a
// capacity can be refused before any output is written.
struct WindowsCall {
    const int32_t* number_groups = nullptr;
    int64_t window = 0;
    uint32_t threshold = 0;
    bool all_digits = false;
    const gx_windows_out* asked = nullptr;   // the caller's; nullptr: the keys alone, no window passes
    gx_windows_totals* totals = nullptr;     // (its group member is the gx_group_totals the pass fills)
    SessionsHead head{};                     // (windows_refusals) the number group per entry of GroupHead::ext[]
    bool any_number = false;
    gx_windows_out out{};
    bool per_entry() const { return out.entry_line || out.entry_key || out.entry_time || out.entry_window_lines || out.entry_window_sum; }
    bool per_trip() const { return out.trip_key || out.trip_line || out.trip_time || out.trip_entry; }
    bool per_key() const { return out.key_entry_begin || out.key_peak_lines || out.key_peak_line || out.key_trip_begin; }
    bool any() const { return per_entry() || per_trip() || per_key() || out.line_window_lines; }
};
static gx_windows_totals windows_totals_of_nothing() {
    gx_windows_totals t{};
    t.peak_line = t.peak_key = GROUP_NONE;
    return t;
}
struct WindowsRun {
    const WindowsCall* call;
    SessionsWs sw{};
    WindowsWs ww{};
    SessionsDev sd{};
    WindowsDev2 wd{};
    uint32_t time_buf = 0, key_buf = 0;
    explicit operator bool() const { return call != nullptr; }
    void start() const { *call->totals = windows_totals_of_nothing(); }
    void nothing(const GroupCtx& c) const {   // no entries: the bounds' one entry and every line's 0
        fill_out(call->out.key_entry_begin, 0, 8, c.host_out, c.stream);
        fill_out(call->out.key_trip_begin, 0, 8, c.host_out, c.stream);
        fill_out(call->out.line_window_lines, 0, c.v.n * 4, c.host_out, c.stream);
    }
    void enqueue(const GroupCtx& c) {
        const BatchView& v = c.v;
        sw = sessions_workspace(c.h->sessions_lines.get(sessions_workspace_bytes(v.n, c.values)), v.n, c.values);
        GX_HIP(hipMemcpyAsync(sw.image, &call->head, sizeof(SessionsHead), hipMemcpyHostToDevice, c.stream));
        GX_HIP(launch_sessions_keys(v.ids, v.fmt, v.row_units, c.K(), v.n, v.offsets, v.off64 ? 1 : 0, c.b.a, c.b.a.formats != 0 || call->head.formats != 0, c.b.w, sw,
                                    c.stream));
        GX_HIP(hipMemcpyAsync(&sd, sw.dev, sizeof(SessionsDev), hipMemcpyDeviceToHost, c.stream));
    }
    int read(const GroupCtx& c) {
        gx_windows_totals& t = *call->totals;
        t.entries = sd.entries;
        t.number_unset = sd.number_unset;
        t.not_numbers = sd.not_numbers;
        if (sd.entries + sd.number_unset + sd.not_numbers != c.totals->keyed)
            throw GxError(GX_E_ARG, "internal: " + c.name + ": the classes of the keyed lines do not add up to them");
        if (sd.entries == 0) return GX_OK;
        t.first_time = top_value(~sd.min_inv, false);
        t.last_time = top_value(sd.max_word, false);
        if (sd.entries > WINDOWS_MAX) return fail(GX_E_LIMIT, c.name + ": " + std::to_string(sd.entries) + " entries; split batches of more than 2^30");
        const uint64_t m = sd.entries, n_keys = c.b.n_keys;
        const SortPlan plan = sessions_time_plan(sd.time_or, ~sd.and_inv, m, call->all_digits);
        const bool sums = call->out.entry_window_sum != nullptr;
        ww = windows_workspace(c.h->windows_ws.get(windows_workspace_bytes(m, n_keys, sums)), m, n_keys, sums);
        GX_HIP(launch_windows_pass(c.v.n, m, n_keys, plan, sessions_key_digits(n_keys, call->all_digits), call->window, call->threshold, c.b.w, sw, ww, &time_buf,
                                   &key_buf, c.stream));
        GX_HIP(hipMemcpyAsync(&wd, ww.dev2, sizeof(WindowsDev2), hipMemcpyDeviceToHost, c.stream));
        GX_HIP(hipStreamSynchronize(c.stream));
        const uint32_t peak = window_peak_lines(wd.peak_word);
        if (wd.n_trips > m || wd.tripped_keys > wd.n_trips || wd.tripped_keys > n_keys || peak == 0 || peak > m || wd.peak_key >= n_keys)
            throw GxError(GX_E_ARG, "internal: " + c.name + ": more trips than entries, more tripped keys than trips or keys, or entries without a peak");
        t.n_trips = wd.n_trips;
        t.tripped_keys = wd.tripped_keys;
        t.peak_lines = peak;
        t.peak_line = wd.peak_line;
        t.peak_key = wd.peak_key;
        return GX_OK;
    }
    int fits(const GroupCtx& c) const {
        const gx_windows_out& b = call->out;
        const std::string& name = c.name;
        if (call->per_entry() && sd.entries > b.max_entries)
            return fail(GX_E_LIMIT, name + ": " + std::to_string(sd.entries) + " entries, max_entries " + std::to_string(b.max_entries));
        if (call->per_trip() && wd.n_trips > b.max_trips)
            return fail(GX_E_LIMIT, name + ": " + std::to_string(wd.n_trips) + " trips, max_trips " + std::to_string(b.max_trips));
        if (call->per_key() && c.b.n_keys > c.max_keys)
            return fail(GX_E_LIMIT, name + ": " + std::to_string(c.b.n_keys) + " keys, max_keys " + std::to_string(c.max_keys));
        return GX_OK;
    }
    // the entries' rows and the trips' ordered by (key number, time, line), the keys' bounds and peaks, the lines' window_lines
    void emit(const GroupCtx& c, HostTwins& twins) const {
        const gx_windows_out& b = call->out;
        const uint64_t n = c.v.n, n_keys = c.b.n_keys, m = sd.entries, nt = wd.n_trips;
        const WindowsOut wo{twins.of(b.entry_line, m * 4), twins.of(b.entry_key, m * 4), twins.of(b.entry_time, m * 8), twins.of(b.entry_window_lines, m * 4),
                            twins.of(reinterpret_cast<uint64_t*>(b.entry_window_sum), m * 32), twins.of(b.key_entry_begin, (n_keys + 1) * 8),
                            twins.of(b.key_peak_lines, n_keys * 4), twins.of(b.key_peak_line, n_keys * 4), twins.of(b.line_window_lines, n * 4),
                            twins.of(b.trip_key, nt * 4), twins.of(b.trip_line, nt * 4), twins.of(b.trip_time, nt * 8), twins.of(b.trip_entry, nt * 4),
                            twins.of(b.key_trip_begin, (n_keys + 1) * 8)};
        if (m == 0) {   // keyed lines, and none of them an entry: every key's runs are empty and it has no peak
            if (wo.key_entry_begin) GX_HIP(hipMemsetAsync(wo.key_entry_begin, 0, (n_keys + 1) * 8, c.stream));
            if (wo.key_trip_begin) GX_HIP(hipMemsetAsync(wo.key_trip_begin, 0, (n_keys + 1) * 8, c.stream));
            if (wo.key_peak_lines && n_keys) GX_HIP(hipMemsetAsync(wo.key_peak_lines, 0, n_keys * 4, c.stream));
            if (wo.key_peak_line && n_keys) GX_HIP(hipMemsetAsync(wo.key_peak_line, 0xFF, n_keys * 4, c.stream));
            if (wo.line_window_lines) GX_HIP(hipMemsetAsync(wo.line_window_lines, 0, n * 4, c.stream));
        } else {
            GX_HIP(launch_windows_emit(n, m, nt, n_keys, sw, ww, time_buf, key_buf, wo, c.stream));
        }
    }
};
// gx_top_groups: what the call adds to gx_group_lines' arguments (top_groups_pass takes group_pass' place)
struct TopGroupsCall {
    uint32_t rank_by = 0, n_wanted = 0, smallest = 0;
    gx_top_groups_out out{};
    gx_top_groups_totals* totals = nullptr;
};
// What the calls built on gx_group_lines add to it, each absent by default.
struct GroupExtras {
    std::optional<GroupQuant> quant;
    std::optional<TopGroupsCall> top;
    std::optional<ByKeyCall> by_key;
    std::optional<PairsCall> pairs;
    std::optional<SeriesCall> series;
    std::optional<SessionsCall> sessions;
    std::optional<SpansCall> spans;
    std::optional<WindowsCall> windows;
};
// The passes on the handle's buffers (under h->mu): build, flags and scans; ONE synchronisation of the stream, where the host reads the
// totals and checks the capacities; then the emit.  out: the caller's, device or host
// (host_out: staged, and a second wait delivers them).  counts: also the histogram of outcomes (gx_text_group_lines).
// x: what the call adds to gx_group_lines, each in the steps that stand beside its arguments above.
static int group_pass(gx_handle* h, const BatchView& v, const GroupImage& gi, const WhereImage& wi, const gx_group_out& out, bool out64, bool host_out,
                      gx_group_totals* totals, uint64_t* counts, hipStream_t stream, const std::string& name, const GroupExtras& x) {
    GroupQuantRun gq(x.quant ? &*x.quant : nullptr);
    ByKeyRun bk{x.by_key ? &*x.by_key : nullptr};
    PairsRun pc{x.pairs && x.pairs->asked ? &*x.pairs : nullptr};
    SeriesRun sc{x.series && x.series->asked ? &*x.series : nullptr};
    SessionsRun ss{x.sessions && x.sessions->asked ? &*x.sessions : nullptr};
    SpansRun sp{x.spans && x.spans->asked ? &*x.spans : nullptr};
    WindowsRun wc{x.windows && x.windows->asked ? &*x.windows : nullptr};
    GroupCtx c{h, v, wi, gi.values, out64, host_out, out.max_keys, totals, stream, name};
    const uint64_t n = v.n;
    if (bk) bk.start();
    if (pc) pc.start();
    if (sc) sc.start();
    if (ss) ss.start();
    if (sp) sp.start();
    if (wc) wc.start();
    if (counts) counts_beside(h, v, counts, stream);
    *totals = gx_group_totals{};
    totals->exact = 1;
    const bool bk_out = bk && bk.call->any(), pc_out = pc && pc.call->any(), sc_out = sc && sc.call->any(), ss_out = ss && ss.call->any(),
               sp_out = sp && sp.call->any(), wc_out = wc && wc.call->any();
    const bool any_out = out.key_units || out.key_offsets || out.key_first_line || out.key_lines || out.key_stats || out.line_key || gq.rows || bk_out || pc_out ||
                         sc_out || ss_out || sp_out || wc_out;
    if (n == 0 || gi.head.n_parts == 0) {
        GX_HIP(hipStreamSynchronize(stream));
        // no keys: the offsets' one entry and every line's "none"
        fill_out(out.key_offsets, 0, out64 ? 8 : 4, host_out, stream);
        fill_out(out.line_key, 0xFF, n * 4, host_out, stream);
        if (bk_out) bk.nothing(c);
        if (pc_out) pc.nothing(c);
        if (sc_out) sc.nothing(c);
        if (ss_out) ss.nothing(c);
        if (sp_out) sp.nothing(c);
        if (wc_out) wc.nothing(c);
        return GX_OK;
    }
    GroupBuild& b = c.b;
    b.enqueue(h, v, gi, wi, out.max_keys, stream);
    if (gq.sort) gq.enqueue(c);
    if (bk) bk.enqueue(c);
    if (pc) pc.enqueue(c);
    if (sc) sc.enqueue(c);
    if (ss) ss.enqueue(c);
    if (sp) sp.enqueue(c);
    if (wc) wc.enqueue(c);
    b.ask(n, stream);
    GX_HIP(hipStreamSynchronize(stream));
    int rc = b.read(totals, name);
    if (rc != GX_OK) return rc;
    if (bk) bk.read(c);
    if (pc && (rc = pc.read(c)) != GX_OK) return rc;
    if (sc && (rc = sc.read(c)) != GX_OK) return rc;
    if (ss && (rc = ss.read(c)) != GX_OK) return rc;
    if (sp && (rc = sp.read(c)) != GX_OK) return rc;
    if (wc && (rc = wc.read(c)) != GX_OK) return rc;
    if (!any_out) return GX_OK;
    const uint64_t n_keys = b.n_keys, key_units = b.key_units;
    const bool per_key = out.key_offsets || out.key_first_line || out.key_lines || out.key_stats || gq.rows;
    if (per_key && n_keys > out.max_keys) return fail(GX_E_LIMIT, name + ": " + std::to_string(n_keys) + " keys, max_keys " + std::to_string(out.max_keys));
    if (out.key_units && key_units > out.key_units_cap)
        return fail(GX_E_LIMIT, name + ": " + std::to_string(key_units) + " key units, key_units_cap " + std::to_string(out.key_units_cap));
    if (out.key_offsets && !out64 && key_units > 0xFFFFFFFFull) return fail(GX_E_LIMIT, name + ": 4 G key units and more need offsets64");
    if (bk_out && (rc = bk.fits(c)) != GX_OK) return rc;
    if (pc_out && (rc = pc.fits(c)) != GX_OK) return rc;
    if (sc_out && (rc = sc.fits(c)) != GX_OK) return rc;
    if (ss_out && (rc = ss.fits(c)) != GX_OK) return rc;
    if (sp_out && (rc = sp.fits(c)) != GX_OK) return rc;
    if (wc_out && (rc = wc.fits(c)) != GX_OK) return rc;
    const size_t unit = v.wide ? 2 : 1, off_w = out64 ? 8 : 4;
    HostTwins twins(host_out);
    const GroupOut o{twins.of(out.key_units, key_units * unit), twins.of(out.key_offsets, (n_keys + 1) * off_w), twins.of(out.key_first_line, n_keys * 4),
                     twins.of(out.key_lines, n_keys * 8), twins.of(reinterpret_cast<uint64_t*>(out.key_stats), n_keys * 64), twins.of(out.line_key, n * 4),
                     out64 ? 1 : 0};
    GX_HIP(launch_group_emit(v.ids, v.fmt, v.row_units, c.K(), n, v.offsets, v.off64 ? 1 : 0, b.a, b.w, o, n_keys, key_units, stream));
    if (bk_out) bk.emit(c, twins);
    if (pc_out) pc.emit(c, twins);
    if (sc_out) sc.emit(c, twins);
    if (ss_out) ss.emit(c, twins);
    if (sp_out) sp.emit(c, twins);
    if (wc_out) wc.emit(c, twins);
    if (gq.rows) gq.emit(c, twins);
    if (host_out) {
        twins.deliver(stream);
        if (bk_out) bk.lines.deliver(stream);
        GX_HIP(hipStreamSynchronize(stream));
    } else {
        leave_pending(h->group_event, h->group_pending, stream);
    }
    return GX_OK;
}

// what gx_group_pairs adds to the refusals of gx_group_lines, behind them and before the look at the device: the second groups, checked
// against the handle and laid out by GroupHead::ext[] (gi: group_refusals')
static void pairs_refusals(const gx_handle* h, const GroupImage& gi, const gx_group_part* parts, uint32_t n_parts, const std::string& name, PairsCall* pc) {
    for (uint32_t q = 0; q < GROUP_MAX_PARTS; ++q) pc->head.second[q] = PAIRS_NO_SECOND;
    if (pc->asked) pc->out = *pc->asked;
    if (n_parts && !pc->second_groups) throw GxError(GX_E_ARG, name + ": second_groups is NULL");
    for (uint32_t t = 0; t < n_parts; ++t) {
        const int32_t sg = pc->second_groups[t];
        if (sg < -1 || sg >= gx_num_groups(h, parts[t].extraction)) throw GxError(GX_E_ARG, name + ": a part's second group is neither -1 nor one of its extraction's");
        if (sg < 0) continue;
        pc->any_second = true;
        for (uint32_t q = 0; q < gi.head.n_parts; ++q)
            if (gi.head.ext[q] == static_cast<uint32_t>(parts[t].extraction)) pc->head.second[q] = sg;
    }
    if (n_parts && !pc->any_second && pc->any()) throw GxError(GX_E_ARG, name + ": pair outputs while every part's second group is -1");
    if (pc->out.max_pairs > PAIRS_MAX_PAIRS) throw GxError(GX_E_LIMIT, name + ": max_pairs above 2^30");
}

// what gx_group_series adds to the refusals of gx_group_lines, behind them and before the look at the device: the number groups, checked
// against the handle and laid out with their formats by GroupHead::ext[] (gi: group_refusals'), then the width and the outputs
static void series_refusals(const gx_handle* h, const GroupImage& gi, const gx_group_part* parts, uint32_t n_parts, const std::string& name, SeriesCall* sc) {
    for (uint32_t q = 0; q < GROUP_MAX_PARTS; ++q) sc->head.number[q] = SERIES_NO_NUMBER;
    sc->head.origin = sc->origin;
    sc->head.width = static_cast<uint64_t>(sc->width < 1 ? 1 : sc->width);
    sc->head.flags = gi.head.flags | (sc->all_digits ? BUCKET_ALL_DIGITS : 0u);
    if (sc->asked) sc->out = *sc->asked;
    if (n_parts && !sc->number_groups) throw GxError(GX_E_ARG, name + ": number_groups is NULL");
    for (uint32_t t = 0; t < n_parts; ++t) {
        const int32_t ng = sc->number_groups[t];
        if (ng < -1 || ng >= gx_num_groups(h, parts[t].extraction)) throw GxError(GX_E_ARG, name + ": a part's number group is neither -1 nor one of its extraction's");
        if (ng < 0) continue;
        sc->any_number = true;
        for (uint32_t q = 0; q < gi.head.n_parts; ++q) {
            if (gi.head.ext[q] != static_cast<uint32_t>(parts[t].extraction)) continue;
            sc->head.number[q] = ng;
            sc->head.nfmt[q] = h->number_format_of(parts[t].extraction, ng);
            if (sc->head.nfmt[q]) sc->head.formats = 1u;
        }
    }
    if (sc->width < 1) throw GxError(GX_E_ARG, name + ": width below 1");
    if (sc->out.cell_stats && !gi.values) throw GxError(GX_E_ARG, name + ": cell_stats without a value_group");
    if (n_parts && !sc->any_number && sc->any()) throw GxError(GX_E_ARG, name + ": series outputs while every part's number group is -1");
    if (sc->out.max_cells > SERIES_MAX_CELLS) throw GxError(GX_E_LIMIT, name + ": max_cells above 2^30");
}

// the number groups of gx_group_sessions and gx_group_windows: checked against the handle and laid out with their formats by
// GroupHead::ext[] (gi: group_refusals')
static void sessions_number_groups(const gx_handle* h, const GroupImage& gi, const gx_group_part* parts, uint32_t n_parts, const int32_t* number_groups,
                                   const std::string& name, SessionsHead* head, bool* any_number) {
    for (uint32_t q = 0; q < GROUP_MAX_PARTS; ++q) head->number[q] = SESSIONS_NO_NUMBER;
    if (n_parts && !number_groups) throw GxError(GX_E_ARG, name + ": number_groups is NULL");
    for (uint32_t t = 0; t < n_parts; ++t) {
        const int32_t ng = number_groups[t];
        if (ng < -1 || ng >= gx_num_groups(h, parts[t].extraction)) throw GxError(GX_E_ARG, name + ": a part's number group is neither -1 nor one of its extraction's");
        if (ng < 0) continue;
        *any_number = true;
        for (uint32_t q = 0; q < gi.head.n_parts; ++q) {
            if (gi.head.ext[q] != static_cast<uint32_t>(parts[t].extraction)) continue;
            head->number[q] = ng;
            head->nfmt[q] = h->number_format_of(parts[t].extraction, ng);
            if (head->nfmt[q]) head->formats = 1u;
        }
    }
}
// what gx_group_sessions adds to the refusals of gx_group_lines, behind them and before the look at the device: the number groups, then
// the gap and the outputs
static void sessions_refusals(const gx_handle* h, const GroupImage& gi, const gx_group_part* parts, uint32_t n_parts, const std::string& name, SessionsCall* ss) {
    if (ss->asked) ss->out = *ss->asked;
    sessions_number_groups(h, gi, parts, n_parts, ss->number_groups, name, &ss->head, &ss->any_number);
    if (ss->max_gap < 0) throw GxError(GX_E_ARG, name + ": max_gap below 0");
    if (ss->out.session_stats && !gi.values) throw GxError(GX_E_ARG, name + ": session_stats without a value_group");
    if (n_parts && !ss->any_number && ss->any()) throw GxError(GX_E_ARG, name + ": session outputs while every part's number group is -1");
    if (ss->out.max_sessions > SESSIONS_MAX) throw GxError(GX_E_LIMIT, name + ": max_sessions above 2^30");
}

// what gx_group_windows adds to the refusals of gx_group_lines, behind them and before the look at the device: gx_group_sessions' number
// groups, then the window, the sums, the trips and the outputs
static void windows_refusals(const gx_handle* h, const GroupImage& gi, const gx_group_part* parts, uint32_t n_parts, const std::string& name, WindowsCall* wc) {
    if (wc->asked) wc->out = *wc->asked;
    sessions_number_groups(h, gi, parts, n_parts, wc->number_groups, name, &wc->head, &wc->any_number);
    if (wc->window < 0) throw GxError(GX_E_ARG, name + ": window below 0");
    if (wc->out.entry_window_sum && !gi.values) throw GxError(GX_E_ARG, name + ": entry_window_sum without a value_group");
    if (wc->threshold == 0 && (wc->per_trip() || wc->out.key_trip_begin)) throw GxError(GX_E_ARG, name + ": trip outputs with threshold 0");
    if (n_parts && !wc->any_number && wc->any()) throw GxError(GX_E_ARG, name + ": window outputs while every part's number group is -1");
    if (wc->out.max_entries > WINDOWS_MAX) throw GxError(GX_E_LIMIT, name + ": max_entries above 2^30");
    if (wc->out.max_trips > WINDOWS_MAX) throw GxError(GX_E_LIMIT, name + ": max_trips above 2^30");
}

// what gx_group_spans adds to the refusals of gx_group_lines, behind them and before the look at the device: the number groups, checked
// against the handle and laid out with their formats by GroupHead::ext[] (gi: group_refusals'), then the roles likewise
static void spans_refusals(const gx_handle* h, const GroupImage& gi, const gx_group_part* parts, uint32_t n_parts, const std::string& name, SpansCall* sp) {
    for (uint32_t q = 0; q < GROUP_MAX_PARTS; ++q) sp->head.number[q] = SPANS_NO_NUMBER;
    if (sp->asked) sp->out = *sp->asked;
    if (n_parts && !sp->number_groups) throw GxError(GX_E_ARG, name + ": number_groups is NULL");
    for (uint32_t t = 0; t < n_parts; ++t) {
        const int32_t ng = sp->number_groups[t];
        if (ng < -1 || ng >= gx_num_groups(h, parts[t].extraction)) throw GxError(GX_E_ARG, name + ": a part's number group is neither -1 nor one of its extraction's");
        if (ng < 0) continue;
        for (uint32_t q = 0; q < gi.head.n_parts; ++q) {
            if (gi.head.ext[q] != static_cast<uint32_t>(parts[t].extraction)) continue;
            sp->head.number[q] = ng;
            sp->head.nfmt[q] = h->number_format_of(parts[t].extraction, ng);
            if (sp->head.nfmt[q]) sp->head.formats = 1u;
        }
    }
    if (n_parts && !sp->roles) throw GxError(GX_E_ARG, name + ": roles is NULL");
    for (uint32_t t = 0; t < n_parts; ++t) {
        const uint32_t role = sp->roles[t];
        if (role != GX_SPAN_BEGIN && role != GX_SPAN_END) throw GxError(GX_E_ARG, name + ": a part's role is neither GX_SPAN_BEGIN nor GX_SPAN_END");
        for (uint32_t q = 0; q < gi.head.n_parts; ++q)
            if (gi.head.ext[q] == static_cast<uint32_t>(parts[t].extraction)) sp->head.role[q] = static_cast<uint8_t>(role);
    }
    if (sp->out.max_spans > SPANS_MAX) throw GxError(GX_E_LIMIT, name + ": max_spans above 2^30");
}

// what gx_lines_by_key adds to the refusals of gx_group_lines, behind them and before the look at the device
static bool ranges_meet(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
    if (!a || !b || !a_bytes || !b_bytes) return false;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    // (a capacity may be "large enough": an end beyond the address space is the address space's)
    const uintptr_t a1 = a_bytes > UINTPTR_MAX - a0 ? UINTPTR_MAX : a0 + static_cast<uintptr_t>(a_bytes);
    const uintptr_t b1 = b_bytes > UINTPTR_MAX - b0 ? UINTPTR_MAX : b0 + static_cast<uintptr_t>(b_bytes);
    return a0 < b1 && b0 < a1;
}
static void by_key_refusals(const ByKeyCall& bk, const std::string& name) {
    if (bk.max_lines != 0 && bk.min_lines > bk.max_lines) throw GxError(GX_E_ARG, name + ": min_lines is above max_lines");
}
// outputs (pointer, capacity in bytes) against inputs (pointer, bytes known before the device is looked at)
static void by_key_overlaps(const std::pair<const void*, uint64_t>* outs, size_t n_outs, const std::pair<const void*, uint64_t>* ins, size_t n_ins,
                            const std::string& name) {
    for (size_t a = 0; a < n_outs; ++a)
        for (size_t b = 0; b < n_ins; ++b)
            if (ranges_meet(outs[a].first, outs[a].second, ins[b].first, ins[b].second)) throw GxError(GX_E_ARG, name + ": an output overlaps an input");
}

// what gx_top_groups adds to the refusals of gx_group_lines, behind them and before the look at the device
static void tg_refusals(const GroupImage& gi, const TopGroupsCall& tg, const std::string& name) {
    if (tg.rank_by >= TG_RANK_KINDS) throw GxError(GX_E_ARG, name + ": rank_by is not one of GX_RANK_LINES .. GX_RANK_MIN");
    if (tg.rank_by != TG_RANK_LINES && !gi.values) throw GxError(GX_E_ARG, name + ": ranking by numbers, sum, max or min needs a part with a value_group");
    if (tg.n_wanted > TG_MAX) throw GxError(GX_E_LIMIT, name + ": n_wanted above GX_TOP_GROUPS_MAX");
}

// gx_top_groups' passes on the handle's buffers (under h->mu): gx_group_lines' build, flags and scans, and the FIRST wait, where the
// host reads gx_group_lines' totals (the keys, the status); then the keys pass, the select, the order and the scan of the chosen keys'
// lengths, and the SECOND wait, where the host reads the candidates, the select's state, the ties and the chosen keys' units and checks
// the capacities; then the emit over the chosen keys.  Host outputs are staged and a third wait delivers them; with device pointers the
// emit is left running under group_event.
static int top_groups_pass(gx_handle* h, const BatchView& v, const GroupImage& gi, const WhereImage& wi, uint64_t max_keys, const TopGroupsCall& tg, bool out64,
                           bool host_out, uint64_t* counts, hipStream_t stream, const std::string& name) {
    const uint32_t K = static_cast<uint32_t>(h->T.n_rules);
    const uint64_t n = v.n;
    if (counts) counts_beside(h, v, counts, stream);
    gx_top_groups_totals* totals = tg.totals;
    *totals = gx_top_groups_totals{};
    totals->group.exact = 1;
    const gx_top_groups_out& out = tg.out;
    const bool any_out = out.key_units || out.key_offsets || out.key_number || out.key_first_line || out.key_lines || out.key_stats || out.line_rank;
    // no keys: the offsets' one entry and every line's "none"
    auto deliver_nothing = [&]() -> int {
        fill_out(out.key_offsets, 0, out64 ? 8 : 4, host_out, stream);
        fill_out(out.line_rank, 0xFF, n * 4, host_out, stream);
        return GX_OK;
    };
    if (n == 0 || gi.head.n_parts == 0) {
        GX_HIP(hipStreamSynchronize(stream));
        return deliver_nothing();
    }
    // the first wait: gx_group_lines' totals
    GroupBuild b;
    b.enqueue(h, v, gi, wi, max_keys, stream);
    b.ask(n, stream);
    GX_HIP(hipStreamSynchronize(stream));
    const int rc = b.read(&totals->group, name);
    if (rc != GX_OK) return rc;
    const GroupArgs& a = b.a;
    const GroupWs& w = b.w;
    const uint32_t n_slots = b.n_slots;
    const uint64_t n_keys = b.n_keys;
    if (n_keys == 0) return deliver_nothing();
    if (n_keys > n) throw GxError(GX_E_ARG, "internal: " + name + ": more keys than lines");
    // the keys pass, the select, the order; the second wait: what the select found
    const TopGroupsWs tw = top_groups_workspace(h->tg_ws.get(top_groups_workspace_bytes(n, n_slots, n_keys)), n, n_slots, n_keys);
    GX_HIP(launch_top_groups_select(n, a, w, n_keys, tg.rank_by, tg.smallest, tg.n_wanted, tw, stream));
    TgDev head{};
    uint64_t both = 0, units_top = 0;
    GX_HIP(hipMemcpyAsync(&head, tw.head, offsetof(TgDev, hist), hipMemcpyDeviceToHost, stream));
    if (tg.n_wanted) {
        GX_HIP(hipMemcpyAsync(&both, tw.before + n_keys, 8, hipMemcpyDeviceToHost, stream));
        GX_HIP(hipMemcpyAsync(&units_top, tw.dst_off + tg.n_wanted, 8, hipMemcpyDeviceToHost, stream));
    }
    GX_HIP(hipStreamSynchronize(stream));
    const uint32_t n_top = tg.n_wanted ? head.sel.n_top : 0u;
    if (n_top > tg.n_wanted || n_top > head.candidates) throw GxError(GX_E_ARG, "internal: " + name + ": the select chose more keys than it may");
    totals->candidates = head.candidates;
    totals->n_top = n_top;
    totals->units_top = units_top;
    if (n_top) {
        tg_value(head.sel.prefix, tg.smallest != 0u, &totals->last_hi, &totals->last_lo);
        totals->ties_left = (both >> 32) - head.sel.remaining;
    }
    if (!any_out) return GX_OK;
    const bool per_key = out.key_offsets || out.key_number || out.key_first_line || out.key_lines || out.key_stats;
    if (per_key && n_top > out.cap_keys) return fail(GX_E_LIMIT, name + ": " + std::to_string(n_top) + " keys, cap_keys " + std::to_string(out.cap_keys));
    if (out.key_units && units_top > out.key_units_cap)
        return fail(GX_E_LIMIT, name + ": " + std::to_string(units_top) + " key units, key_units_cap " + std::to_string(out.key_units_cap));
    if (out.key_offsets && !out64 && units_top > 0xFFFFFFFFull) return fail(GX_E_LIMIT, name + ": 4 G key units and more need offsets64");
    const size_t unit = v.wide ? 2 : 1, off_w = out64 ? 8 : 4;
    HostTwins twins(host_out);
    const TopGroupsOut o{twins.of(out.key_units, units_top * unit), twins.of(out.key_offsets, (n_top + 1) * off_w), twins.of(out.key_number, n_top * 4),
                         twins.of(out.key_first_line, n_top * 4), twins.of(out.key_lines, n_top * 8), twins.of(reinterpret_cast<uint64_t*>(out.key_stats), n_top * 64),
                         twins.of(out.line_rank, n * 4), out64 ? 1 : 0};
    GX_HIP(launch_top_groups_emit(v.ids, v.fmt, v.row_units, K, n, v.offsets, v.off64 ? 1 : 0, a, w, tw, o, n_top, units_top, stream));
    if (host_out) {
        twins.deliver(stream);
        GX_HIP(hipStreamSynchronize(stream));
    } else {
        leave_pending(h->group_event, h->group_pending, stream);
    }
    return GX_OK;
}

// what gx_group_quantiles adds to the refusals of gx_group_lines, behind them and before the look at the device: the quantiles
// (gx_capture_quantiles' rule), and the parts that have a value group as the keys pass reads them
static void gq_refusals(const GroupImage& gi, const std::string& name, GroupQuant* gq) {
    const gx_quantile* quantiles = gq->quantiles;
    const uint32_t n_quantiles = gq->n_quantiles;
    if (n_quantiles && !quantiles) throw GxError(GX_E_ARG, name + ": quantiles is NULL");
    if (n_quantiles > GX_QUANTILE_MAX) throw GxError(GX_E_LIMIT, name + ": n_quantiles above GX_QUANTILE_MAX");
    gq->qh.n_q = n_quantiles;
    for (uint32_t q = 0; q < n_quantiles; ++q) {
        if (quantiles[q].den == 0) throw GxError(GX_E_ARG, name + ": a quantile's den is 0");
        if (quantiles[q].num > quantiles[q].den) throw GxError(GX_E_ARG, name + ": a quantile's num is above its den");
        gq->qh.ask[q] = QuantAsk{quantiles[q].num, quantiles[q].den};
    }
    for (uint32_t e = 0; e < gi.head.n_parts; ++e) {   // (ascending by extraction already)
        if (gi.head.part[e].value_group == GROUP_NO_VALUE) continue;
        gq->ti.ext[gq->ti.n_parts] = gi.head.ext[e];
        gq->ti.fmt[gq->ti.n_parts] = gi.head.fmt[e];
        gq->ti.group[gq->ti.n_parts++] = gi.head.part[e].value_group;
    }
}

// what the extras add to the refusals of gx_group_lines, behind them (gi: group_refusals') and before the look at the device
static void extras_refusals(const gx_handle* h, const GroupImage& gi, const gx_group_part* parts, uint32_t n_parts, const std::string& name, GroupExtras* x) {
    if (x->quant) gq_refusals(gi, name, &*x->quant);
    if (x->top) tg_refusals(gi, *x->top, name);
    if (x->pairs) pairs_refusals(h, gi, parts, n_parts, name, &*x->pairs);
    if (x->series) series_refusals(h, gi, parts, n_parts, name, &*x->series);
    if (x->sessions) sessions_refusals(h, gi, parts, n_parts, name, &*x->sessions);
    if (x->spans) spans_refusals(h, gi, parts, n_parts, name, &*x->spans);
    if (x->windows) windows_refusals(h, gi, parts, n_parts, name, &*x->windows);
    if (x->by_key) by_key_refusals(*x->by_key, name);
}

// gx_group_lines and, with extras, the calls built on it
static int group_lines_call(const std::string& name, gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps,
                            const gx_group_part* parts, uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms, uint32_t flags, const gx_group_out* out,
                            gx_group_totals* totals, const gx_batch_opts* opts, GroupExtras x = {}) {
    return guarded([&]() -> int {
        if (!h || !offsets || (n && !ids)) return fail(GX_E_ARG, name + ": bad argument");
        const gx_batch_opts o = read_opts(opts);
        uint32_t row_units = 1;
        const RowFormat fmt = id_format(h, o, &row_units);
        const gx_group_out none{};
        const gx_group_out& go = out ? *out : none;
        GroupImage gi;
        WhereImage wi;
        group_refusals(h, o, parts, n_parts, terms, n_terms, flags, o.utf16 != 0, go, totals, name, &gi, &wi);
        extras_refusals(h, gi, parts, n_parts, name, &x);
        if (x.by_key && x.by_key->out.out_caps && fmt != ROWS_DENSE) return fail(GX_E_ARG, name + ": out_caps on compact rows (out_ids holds whole rows)");
        if ((n_parts || !wi.none()) && fmt == ROWS_DENSE && n && !caps) return fail(GX_E_ARG, name + ": parts and terms on dense ids need caps");
        if (n >= 0xFFFFFFFFull) return fail(GX_E_LIMIT, name + ": line numbers are 32 bits and one is kept for \"none\"; split batches of 2^32 - 1 lines and more");
        if (!o.device_pointers) refuse_long_host_lines({offsets, o.offsets64 != 0, n}, name, "grouped");
        if (x.by_key) {
            const size_t slots = 2 * static_cast<size_t>(h->T.max_groups);
            gx_by_key_out& b = x.by_key->out;
            if (b.out_caps && slots && n && !caps) return fail(GX_E_ARG, name + ": out_caps without caps");
            if (!slots) b.out_caps = nullptr;
            const uint64_t ow = o.offsets64 ? 8 : 4, un = o.utf16 ? 2 : 1, idr = static_cast<uint64_t>(row_units) * row_unit_bytes(fmt);
            const uint64_t in_units = o.device_pointers ? (n ? 1u : 0u) : HostOffsets{offsets, o.offsets64 != 0, n}[n];
            const uint64_t cap = std::min<uint64_t>(b.cap_lines, n);   // (no more than n lines leave, whatever the capacity says: n < 2^32, no product wraps)
            const std::pair<const void*, uint64_t> outs[7] = {{b.out_index, cap * 4}, {b.out_bytes, b.out_bytes_cap}, {b.out_offsets, (cap + 1) * ow},
                                                              {b.out_ids, cap * idr}, {b.out_caps, cap * slots * 4},
                                                              {b.key_out_lines, (go.max_keys + 1) * 8}, {b.key_out_units, (go.max_keys + 1) * 8}};
            const std::pair<const void*, uint64_t> ins[4] = {{bytes, in_units * un}, {offsets, (n + 1) * ow}, {ids, n * idr},
                                                             {fmt == ROWS_DENSE ? caps : nullptr, n * slots * 4}};
            by_key_overlaps(outs, 7, ins, 4, name);
        }
        if (!h->on_device) return fail(GX_E_DEVICE, "handle was created host-only; no device tables (there is no CPU fallback)");
        if (fmt != ROWS_DENSE) caps = nullptr;
        GX_HIP(hipSetDevice(h->device));
        std::lock_guard<std::mutex> lock(h->mu);
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        const StagedLines in = stage_lines(h, bytes, offsets, n, ids, caps, o, fmt, row_units, Travels{true, caps != nullptr}, stream, name.c_str());
        if (x.top) return top_groups_pass(h, in.v, gi, wi, go.max_keys, *x.top, o.offsets64 != 0, !o.device_pointers, nullptr, stream, name);
        return group_pass(h, in.v, gi, wi, go, o.offsets64 != 0, !o.device_pointers, totals, nullptr, stream, name, x);
    });
}

int gx_group_lines(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps, const gx_group_part* parts,
                   uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms, uint32_t flags, const gx_group_out* out, gx_group_totals* totals,
                   const gx_batch_opts* opts) {
    return group_lines_call("gx_group_lines", h, bytes, offsets, n, ids, caps, parts, n_parts, terms, n_terms, flags, out, totals, opts);
}

int gx_group_quantiles(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps, const gx_group_part* parts,
                       uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms, const gx_quantile* quantiles, uint32_t n_quantiles, uint32_t flags,
                       const gx_group_out* out, gx_quantile_out* key_quantiles, gx_group_totals* totals, const gx_batch_opts* opts) {
    GroupExtras x;
    x.quant = GroupQuant{quantiles, n_quantiles, key_quantiles};
    return group_lines_call("gx_group_quantiles", h, bytes, offsets, n, ids, caps, parts, n_parts, terms, n_terms, flags, out, totals, opts, x);
}

// gx_text_group_lines and, with extras, the calls built on it
static int text_group_call(const std::string& name, gx_handle* h, const uint8_t* text, uint64_t size, const gx_group_part* parts, uint32_t n_parts,
                           const gx_where_term* terms, uint32_t n_terms, uint32_t flags, const gx_group_out* out, gx_group_totals* totals, uint64_t* counts,
                           uint64_t* n_lines, const gx_batch_opts* opts, GroupExtras x = {}) {
    return guarded([&]() -> int {
        if (!h || (size && !text)) return fail(GX_E_ARG, name + ": bad argument");
        const gx_batch_opts o = read_opts(opts);
        const gx_group_out none{};
        const gx_group_out& go = out ? *out : none;
        GroupImage gi;
        WhereImage wi;
        group_refusals(h, o, parts, n_parts, terms, n_terms, flags, false, go, totals, name, &gi, &wi);
        extras_refusals(h, gi, parts, n_parts, name, &x);
        if (x.by_key) {
            const gx_by_key_out& b = x.by_key->out;
            const std::pair<const void*, uint64_t> outs[5] = {{b.out_bytes, b.out_bytes_cap}, {b.out_offsets, 4}, {b.out_index, 4}, {b.key_out_lines, (go.max_keys + 1) * 8},
                                                              {b.key_out_units, (go.max_keys + 1) * 8}};
            const std::pair<const void*, uint64_t> ins[1] = {{text, size}};
            by_key_overlaps(outs, 5, ins, 1, name);
        }
        if (size > 0xFFFFFFFFull) return fail(GX_E_LIMIT, name + ": split texts of 4 GiB and more at a line boundary");
        if (!h->on_device) return fail(GX_E_DEVICE, "handle was created host-only; no device tables (there is no CPU fallback)");
        GX_HIP(hipSetDevice(h->device));
        std::lock_guard<std::mutex> lock(h->mu);
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        // the text's lines and the path; then the passes over the ids, offsets and capture rows they left on the device
        const TextBatch tb = stage_text_lines(h, text, size, o, stream, name.c_str());
        if (n_lines) *n_lines = tb.v.n;
        const int rc = x.top ? top_groups_pass(h, tb.v, gi, wi, go.max_keys, *x.top, o.offsets64 != 0, !o.device_pointers, counts, stream, name)
                             : group_pass(h, tb.v, gi, wi, go, o.offsets64 != 0, !o.device_pointers, totals, counts, stream, name, x);
        // The emit pass reads the offsets, ids and capture rows that text_lines left in the handle's scratch buffers, which the next
        // whole-file call on any stream overwrites: like every gx_text_* call this one returns with its work done (host outputs: the
        // wait that delivered them was that already).
        if (h->group_pending) {
            GX_HIP(hipStreamSynchronize(stream));
            h->group_pending = false;
        }
        if (promise_broken_since(h, stream)) throw GxError(GX_E_ARG, "internal: " + name + ": a line longer than the split pass reported");
        return rc;
    });
}

int gx_text_group_lines(gx_handle* h, const uint8_t* text, uint64_t size, const gx_group_part* parts, uint32_t n_parts, const gx_where_term* terms,
                        uint32_t n_terms, uint32_t flags, const gx_group_out* out, gx_group_totals* totals, uint64_t* counts, uint64_t* n_lines,
                        const gx_batch_opts* opts) {
    return text_group_call("gx_text_group_lines", h, text, size, parts, n_parts, terms, n_terms, flags, out, totals, counts, n_lines, opts);
}

int gx_text_group_quantiles(gx_handle* h, const uint8_t* text, uint64_t size, const gx_group_part* parts, uint32_t n_parts, const gx_where_term* terms,
                            uint32_t n_terms, const gx_quantile* quantiles, uint32_t n_quantiles, uint32_t flags, const gx_group_out* out,
                            gx_quantile_out* key_quantiles, gx_group_totals* totals, uint64_t* counts, uint64_t* n_lines, const gx_batch_opts* opts) {
    GroupExtras x;
    x.quant = GroupQuant{quantiles, n_quantiles, key_quantiles};
    return text_group_call("gx_text_group_quantiles", h, text, size, parts, n_parts, terms, n_terms, flags, out, totals, counts, n_lines, opts, x);
}

// gx_lines_by_key's own arguments as gx_group_lines' callers take them: the flags without GX_BY_KEY_ALL_DIGITS (unknown bits stay in the
// flags and are refused there), and &totals->group.
static GroupExtras by_key_extras(uint64_t min_lines, uint64_t max_lines, uint32_t flags, const gx_by_key_out* out, gx_by_key_totals* totals) {
    ByKeyCall bk;
    bk.min_lines = min_lines;
    bk.max_lines = max_lines;
    bk.all_digits = (flags & GX_BY_KEY_ALL_DIGITS) != 0u;
    if (out) bk.out = *out;
    bk.totals = totals;
    GroupExtras x;
    x.by_key = bk;
    return x;
}

int gx_lines_by_key(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps, const gx_group_part* parts,
                    uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms, uint64_t min_lines, uint64_t max_lines, uint32_t flags, const gx_group_out* keys,
                    const gx_by_key_out* out, gx_by_key_totals* totals, const gx_batch_opts* opts) {
    return group_lines_call("gx_lines_by_key", h, bytes, offsets, n, ids, caps, parts, n_parts, terms, n_terms, flags & ~static_cast<uint32_t>(GX_BY_KEY_ALL_DIGITS), keys,
                            totals ? &totals->group : nullptr, opts, by_key_extras(min_lines, max_lines, flags, out, totals));
}

int gx_text_lines_by_key(gx_handle* h, const uint8_t* text, uint64_t size, const gx_group_part* parts, uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms,
                         uint64_t min_lines, uint64_t max_lines, uint32_t flags, const gx_group_out* keys, uint8_t* out, uint64_t out_cap, void* out_offsets,
                         uint32_t* out_index, uint64_t* key_out_lines, uint64_t* key_out_units, gx_by_key_totals* totals, uint64_t* counts, uint64_t* n_lines,
                         const gx_batch_opts* opts) {
    gx_by_key_out bo{};
    bo.out_index = out_index; bo.out_bytes = out; bo.out_offsets = out_offsets;
    bo.cap_lines = ~0ull;   // (sized by the size query: the header)
    bo.out_bytes_cap = out_cap;
    bo.key_out_lines = key_out_lines; bo.key_out_units = key_out_units;
    return text_group_call("gx_text_lines_by_key", h, text, size, parts, n_parts, terms, n_terms, flags & ~static_cast<uint32_t>(GX_BY_KEY_ALL_DIGITS), keys,
                           totals ? &totals->group : nullptr, counts, n_lines, opts, by_key_extras(min_lines, max_lines, flags, &bo, totals));
}

// gx_group_pairs: gx_group_lines' call with the pairs behind it.  totals == NULL is refused as gx_group_lines refuses it.
static GroupExtras pairs_extras(const int32_t* second_groups, const gx_pairs_out* pairs, gx_pairs_totals* totals) {
    if (totals) {
        *totals = gx_pairs_totals{};
        totals->pairs_exact = 1;
    }
    GroupExtras x;
    x.pairs = PairsCall{second_groups, pairs, totals};
    return x;
}

int gx_group_pairs(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps, const gx_group_part* parts,
                   uint32_t n_parts, const int32_t* second_groups, const gx_where_term* terms, uint32_t n_terms, uint32_t flags, const gx_group_out* keys,
                   const gx_pairs_out* pairs, gx_pairs_totals* totals, const gx_batch_opts* opts) {
    return group_lines_call("gx_group_pairs", h, bytes, offsets, n, ids, caps, parts, n_parts, terms, n_terms, flags, keys, totals ? &totals->group : nullptr, opts,
                            pairs_extras(second_groups, pairs, totals));
}

int gx_text_group_pairs(gx_handle* h, const uint8_t* text, uint64_t size, const gx_group_part* parts, uint32_t n_parts, const int32_t* second_groups,
                        const gx_where_term* terms, uint32_t n_terms, uint32_t flags, const gx_group_out* keys, const gx_pairs_out* pairs, gx_pairs_totals* totals,
                        uint64_t* counts, uint64_t* n_lines, const gx_batch_opts* opts) {
    return text_group_call("gx_text_group_pairs", h, text, size, parts, n_parts, terms, n_terms, flags, keys, totals ? &totals->group : nullptr, counts, n_lines, opts,
                           pairs_extras(second_groups, pairs, totals));
}

// gx_group_series: gx_group_lines' call with the series behind it.  totals == NULL is refused as gx_group_lines refuses it.  The flags
// travel without GX_BUCKET_ALL_DIGITS (unknown bits stay in the flags and are refused there).
static GroupExtras series_extras(const int32_t* number_groups, int64_t origin, int64_t width, uint32_t flags, const gx_series_out* series, gx_series_totals* totals) {
    if (totals) {
        *totals = gx_series_totals{};
        totals->cells_exact = 1;
    }
    SeriesCall sc;
    sc.number_groups = number_groups;
    sc.origin = origin;
    sc.width = width;
    sc.all_digits = (flags & GX_BUCKET_ALL_DIGITS) != 0u;
    sc.asked = series;
    sc.totals = totals;
    GroupExtras x;
    x.series = sc;
    return x;
}
static_assert(sizeof(gx_series_out) == 80 && sizeof(gx_series_totals) == sizeof(gx_group_totals) + 72, "include/gorp_hip.h states these layouts");

int gx_group_series(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps, const gx_group_part* parts,
                    uint32_t n_parts, const int32_t* number_groups, int64_t origin, int64_t width, const gx_where_term* terms, uint32_t n_terms, uint32_t flags,
                    const gx_group_out* keys, const gx_series_out* series, gx_series_totals* totals, const gx_batch_opts* opts) {
    return group_lines_call("gx_group_series", h, bytes, offsets, n, ids, caps, parts, n_parts, terms, n_terms, flags & ~static_cast<uint32_t>(GX_BUCKET_ALL_DIGITS), keys,
                            totals ? &totals->group : nullptr, opts, series_extras(number_groups, origin, width, flags, series, totals));
}

int gx_text_group_series(gx_handle* h, const uint8_t* text, uint64_t size, const gx_group_part* parts, uint32_t n_parts, const int32_t* number_groups, int64_t origin,
                         int64_t width, const gx_where_term* terms, uint32_t n_terms, uint32_t flags, const gx_group_out* keys, const gx_series_out* series,
                         gx_series_totals* totals, uint64_t* counts, uint64_t* n_lines, const gx_batch_opts* opts) {
    return text_group_call("gx_text_group_series", h, text, size, parts, n_parts, terms, n_terms, flags & ~static_cast<uint32_t>(GX_BUCKET_ALL_DIGITS), keys,
                           totals ? &totals->group : nullptr, counts, n_lines, opts, series_extras(number_groups, origin, width, flags, series, totals));
}

// gx_group_sessions: gx_group_lines' call with the sessions behind it.  totals == NULL is refused as gx_group_lines refuses it.  The flags
// travel without GX_BUCKET_ALL_DIGITS (unknown bits stay in the flags and are refused there).
static GroupExtras sessions_extras(const int32_t* number_groups, int64_t max_gap, uint32_t flags, const gx_sessions_out* sessions, gx_sessions_totals* totals) {
    if (totals) *totals = gx_sessions_totals{};
    SessionsCall ss;
    ss.number_groups = number_groups;
    ss.max_gap = max_gap;
    ss.all_digits = (flags & GX_BUCKET_ALL_DIGITS) != 0u;
    ss.asked = sessions;
    ss.totals = totals;
    GroupExtras x;
    x.sessions = ss;
    return x;
}
static_assert(sizeof(gx_sessions_out) == 96 && sizeof(gx_sessions_totals) == sizeof(gx_group_totals) + 64, "include/gorp_hip.h states these layouts");

int gx_group_sessions(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps, const gx_group_part* parts,
                      uint32_t n_parts, const int32_t* number_groups, int64_t max_gap, const gx_where_term* terms, uint32_t n_terms, uint32_t flags,
                      const gx_group_out* keys, const gx_sessions_out* sessions, gx_sessions_totals* totals, const gx_batch_opts* opts) {
    return group_lines_call("gx_group_sessions", h, bytes, offsets, n, ids, caps, parts, n_parts, terms, n_terms, flags & ~static_cast<uint32_t>(GX_BUCKET_ALL_DIGITS), keys,
                            totals ? &totals->group : nullptr, opts, sessions_extras(number_groups, max_gap, flags, sessions, totals));
}

int gx_text_group_sessions(gx_handle* h, const uint8_t* text, uint64_t size, const gx_group_part* parts, uint32_t n_parts, const int32_t* number_groups,
                           int64_t max_gap, const gx_where_term* terms, uint32_t n_terms, uint32_t flags, const gx_group_out* keys, const gx_sessions_out* sessions,
                           gx_sessions_totals* totals, uint64_t* counts, uint64_t* n_lines, const gx_batch_opts* opts) {
    return text_group_call("gx_text_group_sessions", h, text, size, parts, n_parts, terms, n_terms, flags & ~static_cast<uint32_t>(GX_BUCKET_ALL_DIGITS), keys,
                           totals ? &totals->group : nullptr, counts, n_lines, opts, sessions_extras(number_groups, max_gap, flags, sessions, totals));
}

// gx_group_spans: gx_group_lines' call with the spans behind it.  totals == NULL is refused as gx_group_lines refuses it.  The flags
// travel without GX_BY_KEY_ALL_DIGITS (unknown bits stay in the flags and are refused there).
static GroupExtras spans_extras(const int32_t* number_groups, const uint32_t* roles, uint32_t flags, const gx_spans_out* spans, gx_spans_totals* totals) {
    if (totals) *totals = gx_spans_totals{};
    SpansCall sp;
    sp.number_groups = number_groups;
    sp.roles = roles;
    sp.all_digits = (flags & GX_BY_KEY_ALL_DIGITS) != 0u;
    sp.asked = spans;
    sp.totals = totals;
    GroupExtras x;
    x.spans = sp;
    return x;
}
static_assert(sizeof(gx_spans_out) == 104 && sizeof(gx_spans_totals) == sizeof(gx_group_totals) + 120, "include/gorp_hip.h states these layouts");
static_assert(GX_SPAN_BEGIN == SPAN_BEGIN && GX_SPAN_END == SPAN_END, "gx_spans.hpp states the roles again");

int gx_group_spans(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps, const gx_group_part* parts,
                   uint32_t n_parts, const int32_t* number_groups, const uint32_t* roles, const gx_where_term* terms, uint32_t n_terms, uint32_t flags,
                   const gx_group_out* keys, const gx_spans_out* spans, gx_spans_totals* totals, const gx_batch_opts* opts) {
    return group_lines_call("gx_group_spans", h, bytes, offsets, n, ids, caps, parts, n_parts, terms, n_terms, flags & ~static_cast<uint32_t>(GX_BY_KEY_ALL_DIGITS), keys,
                            totals ? &totals->group : nullptr, opts, spans_extras(number_groups, roles, flags, spans, totals));
}

int gx_text_group_spans(gx_handle* h, const uint8_t* text, uint64_t size, const gx_group_part* parts, uint32_t n_parts, const int32_t* number_groups,
                        const uint32_t* roles, const gx_where_term* terms, uint32_t n_terms, uint32_t flags, const gx_group_out* keys, const gx_spans_out* spans,
                        gx_spans_totals* totals, uint64_t* counts, uint64_t* n_lines, const gx_batch_opts* opts) {
    return text_group_call("gx_text_group_spans", h, text, size, parts, n_parts, terms, n_terms, flags & ~static_cast<uint32_t>(GX_BY_KEY_ALL_DIGITS), keys,
                           totals ? &totals->group : nullptr, counts, n_lines, opts, spans_extras(number_groups, roles, flags, spans, totals));
}

// gx_group_windows: gx_group_lines' call with the windows behind it.  totals == NULL is refused as gx_group_lines refuses it.  The flags
// travel without GX_BUCKET_ALL_DIGITS (unknown bits stay in the flags and are refused there).
static GroupExtras windows_extras(const int32_t* number_groups, int64_t window, uint32_t threshold, uint32_t flags, const gx_windows_out* windows,
                                  gx_windows_totals* totals) {
    if (totals) *totals = windows_totals_of_nothing();
    WindowsCall wc;
    wc.number_groups = number_groups;
    wc.window = window;
    wc.threshold = threshold;
    wc.all_digits = (flags & GX_BUCKET_ALL_DIGITS) != 0u;
    wc.asked = windows;
    wc.totals = totals;
    GroupExtras x;
    x.windows = wc;
    return x;
}
static_assert(sizeof(gx_windows_out) == 128 && sizeof(gx_windows_totals) == sizeof(gx_group_totals) + 72 && sizeof(gx_window_sum) == sizeof(WindowSum),
              "include/gorp_hip.h states these layouts");

int gx_group_windows(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps, const gx_group_part* parts,
                     uint32_t n_parts, const int32_t* number_groups, int64_t window, uint32_t threshold, const gx_where_term* terms, uint32_t n_terms, uint32_t flags,
                     const gx_group_out* keys, const gx_windows_out* windows, gx_windows_totals* totals, const gx_batch_opts* opts) {
    return group_lines_call("gx_group_windows", h, bytes, offsets, n, ids, caps, parts, n_parts, terms, n_terms, flags & ~static_cast<uint32_t>(GX_BUCKET_ALL_DIGITS), keys,
                            totals ? &totals->group : nullptr, opts, windows_extras(number_groups, window, threshold, flags, windows, totals));
}

int gx_text_group_windows(gx_handle* h, const uint8_t* text, uint64_t size, const gx_group_part* parts, uint32_t n_parts, const int32_t* number_groups,
                          int64_t window, uint32_t threshold, const gx_where_term* terms, uint32_t n_terms, uint32_t flags, const gx_group_out* keys,
                          const gx_windows_out* windows, gx_windows_totals* totals, uint64_t* counts, uint64_t* n_lines, const gx_batch_opts* opts) {
    return text_group_call("gx_text_group_windows", h, text, size, parts, n_parts, terms, n_terms, flags & ~static_cast<uint32_t>(GX_BUCKET_ALL_DIGITS), keys,
                           totals ? &totals->group : nullptr, counts, n_lines, opts, windows_extras(number_groups, window, threshold, flags, windows, totals));
}

// gx_lookup_lines: what the call adds to gx_group_lines' parts, terms and flags -- the dictionary, keep, the outputs (the text form: its
// three kept outputs in the batch pointers' places) and the totals.
struct LookupCall {
    const void* entry_units = nullptr;
    const void* entry_offsets = nullptr;
    uint64_t m = 0;
    uint32_t keep = 0;
    gx_lookup_out out{};
    gx_lookup_totals* totals = nullptr;
    bool per_line() const { return out.out_index || out.out_offsets || out.out_ids || out.out_caps; }
    bool batch_out() const { return per_line() || out.out_bytes; }
    bool per_entry() const { return out.entry_same || out.entry_lines || out.entry_first_line || out.entry_stats; }
    bool any() const { return batch_out() || per_entry() || out.line_entry; }
};
static_assert(sizeof(gx_lookup_out) == 96 && sizeof(gx_lookup_totals) == 80, "include/gorp_hip.h states these layouts");
static_assert(GX_LOOKUP_NONE == LOOKUP_NONE && GX_LOOKUP_MISS == LOOKUP_MISS && GX_LOOKUP_KEEP_HITS == LOOKUP_KEEP_HITS && GX_LOOKUP_KEEP_OTHERS == LOOKUP_KEEP_OTHERS,
              "gx_lookup.hpp states the sentinels and keep again");

// what both lookup calls refuse before they look at the device: gx_group_lines' refusals of totals, flags, parts, options and terms, then
// the call's own
static void lookup_refusals(const gx_handle* h, const gx_batch_opts& o, const gx_group_part* parts, uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms,
                            uint32_t flags, bool wide, const LookupCall& c, const std::string& name, GroupImage* gi, WhereImage* wi) {
    gx_group_totals unused{};
    group_refusals(h, o, parts, n_parts, terms, n_terms, flags, wide, gx_group_out{}, c.totals ? &unused : nullptr, name, gi, wi);
    if (c.out.entry_stats && !gi->values) throw GxError(GX_E_ARG, name + ": entry_stats without a value_group");
    if (c.keep >= LOOKUP_KEEPS) throw GxError(GX_E_ARG, name + ": keep is not one of GX_LOOKUP_KEEP_NOTHING .. GX_LOOKUP_KEEP_OTHERS");
    if (c.keep == LOOKUP_KEEP_NOTHING && c.batch_out()) throw GxError(GX_E_ARG, name + ": outputs for kept lines with GX_LOOKUP_KEEP_NOTHING");
}
// ... and behind the refusals that only the batch form makes: the dictionary's own.  Host offsets are read here.  Returns the units the
// offsets name, [first, last) (device offsets: unknown, 0 and 0).
static std::pair<uint64_t, uint64_t> lookup_dict_refusals(const gx_batch_opts& o, const LookupCall& c, const std::string& name) {
    if (c.m && !c.entry_offsets) throw GxError(GX_E_ARG, name + ": entry_offsets is NULL");
    if (c.m > LOOKUP_MAX_ENTRIES) throw GxError(GX_E_LIMIT, name + ": more than 2^30 entries");
    if (o.device_pointers || c.m == 0) return {0, 0};
    const HostOffsets eo{c.entry_offsets, o.offsets64 != 0, c.m};
    for (uint64_t j = 0; j < c.m; ++j)
        if (eo[j + 1] - eo[j] > 0xFFFFFFFFull) throw GxError(GX_E_LIMIT, name + ": an entry of 4 G code units or more (or entry offsets that go backwards)");
    if (eo[c.m] > eo[0] && !c.entry_units) throw GxError(GX_E_ARG, name + ": entry_units is NULL");
    return {eo[0], eo[c.m]};
}
// the dictionary's ranges as by_key_overlaps takes inputs (device offsets: the units' length is not known -- their first byte stands for them)
static void lookup_dict_ranges(const gx_batch_opts& o, const LookupCall& c, std::pair<uint64_t, uint64_t> units, std::pair<const void*, uint64_t>* ins) {
    const uint64_t un = o.utf16 ? 2 : 1, ow = o.offsets64 ? 8 : 4;
    ins[0] = {c.m ? c.entry_offsets : nullptr, (c.m + 1) * ow};
    if (o.device_pointers) ins[1] = {c.m ? c.entry_units : nullptr, 1};
    else ins[1] = {c.entry_units ? static_cast<const uint8_t*>(c.entry_units) + units.first * un : nullptr, (units.second - units.first) * un};
}

// The dictionary on the device: the caller's own pointers (device_pointers), or copies that live as long as this object -- the offsets as
// they are, and the units they name, [first, last), so that d.units + offsets[j] is entry j wherever offsets[0] lies.
namespace {
struct StagedDict {
    LookupDict d{};
    DevMem<> units, offsets;
};
}  // namespace
static StagedDict stage_dict(const LookupCall& c, const gx_batch_opts& o, std::pair<uint64_t, uint64_t> named, uint32_t flags, hipStream_t stream) {
    StagedDict s;
    s.d = LookupDict{c.entry_units, c.entry_offsets, o.offsets64 ? 1 : 0, c.m, (flags & GX_GROUP_WEAK_HASH) ? 1u : 0u};
    if (o.device_pointers || c.m == 0) return s;
    const size_t ow = o.offsets64 ? 8 : 4, un = o.utf16 ? 2 : 1;
    const size_t bytes = static_cast<size_t>(named.second - named.first) * un;
    s.offsets = dev_alloc((c.m + 1) * ow);
    s.units = dev_alloc(bytes);
    GX_HIP(hipMemcpyAsync(s.offsets.get(), c.entry_offsets, (c.m + 1) * ow, hipMemcpyHostToDevice, stream));
    if (bytes) GX_HIP(hipMemcpyAsync(s.units.get(), static_cast<const uint8_t*>(c.entry_units) + named.first * un, bytes, hipMemcpyHostToDevice, stream));
    s.d.offsets = s.offsets.get();
    s.d.units = reinterpret_cast<const void*>(reinterpret_cast<uintptr_t>(s.units.get()) - static_cast<uintptr_t>(named.first * un));   // (never read below offsets[0])
    return s;
}

// The passes on the handle's buffers (under h->mu): the dictionary's build, the probe, with keep gx_select.hip's scans, the entries' count;
// ONE synchronisation of the stream, where the host reads the totals and checks the capacities; then the emits and the copy.  The
// caller's outputs are device or host (host_out: staged, and a second wait delivers them).  leave: with device outputs the emits are
// left running under lookup_event (and select_event); the text form waits for them instead.  counts: also the histogram of outcomes.
static int lookup_pass(gx_handle* h, const BatchView& v, const GroupImage& gi, const WhereImage& wi, const LookupCall& c, const LookupDict& dict, bool host_out,
                       bool leave, uint64_t* counts, hipStream_t stream, const std::string& name) {
    const uint32_t K = static_cast<uint32_t>(h->T.n_rules);
    const uint64_t n = v.n, m = c.m;
    gx_lookup_totals& t = *c.totals;
    t = gx_lookup_totals{};
    t.entries = m;
    const bool sel = c.keep != LOOKUP_KEEP_NOTHING;
    wait_pending(h->lookup_event, h->lookup_pending, stream);
    SelectWs sw{};
    if (sel || counts) {
        wait_pending(h->select_event, h->select_pending, stream);
        sw = select_workspace(h->select_ws.get(select_workspace_bytes(n, K, sel)), n, K, sel);
        if (counts) {   // (counts_beside's pass, on the workspace that the probe's flags share)
            GX_HIP(launch_select_flags(v.ids, v.fmt, v.row_units, K, n, nullptr, 0, sw, stream));
            GX_HIP(hipMemcpyAsync(counts, sw.counts, static_cast<size_t>(2u * K + 2u) * 8, hipMemcpyDeviceToHost, stream));
        }
    }
    const uint32_t n_slots = group_slots(m);
    const DevImage img = upload_image(h->lookup_image, &gi.head, sizeof(GroupHead), nullptr, wi, stream);
    const GroupArgs a{v.data, v.wide ? 1 : 0, v.caps, 2u * static_cast<uint32_t>(h->T.max_groups), img.head, img.terms, static_cast<uint32_t>(wi.bytes.size()),
                      gi.values ? 1u : 0u, (gi.head.formats || wi.formats) ? 1u : 0u};
    const LookupWs w = lookup_workspace(h->lookup_table.get(lookup_table_bytes(n_slots, gi.values)), h->lookup_lines.get(lookup_lines_bytes(n, m)), n, m, n_slots, gi.values);
    GX_HIP(launch_lookup_probe(v.ids, v.fmt, v.row_units, K, n, v.offsets, v.off64 ? 1 : 0, a, dict, c.keep, w, sel ? &sw : nullptr, stream));
    if (sel) GX_HIP(launch_select_scans(n, sw, stream));
    uint64_t got[8] = {0, 0, 0, 0, 0, 0, 0, 0}, lines_out = 0, units_out = 0;
    GX_HIP(hipMemcpyAsync(got, w.totals, sizeof(got), hipMemcpyDeviceToHost, stream));
    if (sel) {
        GX_HIP(hipMemcpyAsync(&lines_out, sw.idx_off + n, 8, hipMemcpyDeviceToHost, stream));
        GX_HIP(hipMemcpyAsync(&units_out, sw.dst_off + n, 8, hipMemcpyDeviceToHost, stream));
    }
    GX_HIP(hipStreamSynchronize(stream));
    if (got[2] & 1u) throw GxError(GX_E_LIMIT, name + ": a line or an entry of 4 G code units or more (or offsets that go backwards) cannot be looked up");
    if (got[2] & 2u) throw GxError(GX_E_ARG, "internal: " + name + ": the dictionary's table is full");
    if (got[0] != got[1] + got[3] + got[4] || lines_out > n) throw GxError(GX_E_ARG, "internal: " + name + ": the classes do not add up");
    t.lines = got[0];
    t.unset = got[1];
    t.keyed = got[0] - got[1];
    t.hits = got[3];
    t.misses = got[4];
    t.distinct_entries = got[5];
    t.hit_entries = got[6];
    t.lines_out = lines_out;
    t.units_out = units_out;
    if (!c.any()) return GX_OK;   // size query
    const gx_lookup_out& o = c.out;
    const size_t unit = v.wide ? 2 : 1;
    if (c.per_line() && lines_out > o.cap_lines) return fail(GX_E_LIMIT, name + ": cap_lines is smaller than the result (see totals->lines_out)");
    if (o.out_bytes && units_out * unit > o.out_bytes_cap) return fail(GX_E_LIMIT, name + ": the kept text is larger than the capacity (see totals->units_out)");
    if (o.out_offsets && !v.off64 && units_out > 0xFFFFFFFFull) return fail(GX_E_LIMIT, name + ": 4 G code units and more need offsets64");
    HostTwins twins(host_out);
    const LookupOut lo{twins.of(o.line_entry, n * 4), twins.of(o.entry_same, m * 4), twins.of(o.entry_lines, m * 8), twins.of(o.entry_first_line, m * 4),
                       twins.of(reinterpret_cast<uint64_t*>(o.entry_stats), m * 64)};
    GX_HIP(launch_lookup_emit(n, m, gi.values, w, lo, stream));
    StagedLinesOut kept;
    if (c.batch_out()) {
        kept = stage_lines_out(h, v, LinesOut{o.out_index, o.out_bytes, o.out_offsets, o.out_ids, o.out_caps}, host_out, lines_out, units_out);
        if (kept.dev.offsets && n == 0) GX_HIP(hipMemsetAsync(kept.dev.offsets, 0, v.off64 ? 8 : 4, stream));
        GX_HIP(launch_select_copy(kept.dev, v.data, v.offsets, v.off64 ? 1 : 0, v.wide ? 1 : 0, n, sw, stream));
    }
    if (host_out) {
        twins.deliver(stream);
        kept.deliver(stream);
        GX_HIP(hipStreamSynchronize(stream));
    } else if (leave) {
        leave_pending(h->lookup_event, h->lookup_pending, stream);
        if (c.batch_out()) leave_pending(h->select_event, h->select_pending, stream);
    } else {
        GX_HIP(hipStreamSynchronize(stream));
    }
    return GX_OK;
}

int gx_lookup_lines(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps, const gx_group_part* parts,
                    uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms, const void* entry_units, const void* entry_offsets, uint64_t n_entries,
                    uint32_t keep, uint32_t flags, const gx_lookup_out* out, gx_lookup_totals* totals, const gx_batch_opts* opts) {
    const std::string name = "gx_lookup_lines";
    return guarded([&]() -> int {
        if (!h || !offsets || (n && !ids)) return fail(GX_E_ARG, name + ": bad argument");
        const gx_batch_opts o = read_opts(opts);
        uint32_t row_units = 1;
        const RowFormat fmt = id_format(h, o, &row_units);
        LookupCall c{entry_units, entry_offsets, n_entries, keep, out ? *out : gx_lookup_out{}, totals};
        GroupImage gi;
        WhereImage wi;
        lookup_refusals(h, o, parts, n_parts, terms, n_terms, flags, o.utf16 != 0, c, name, &gi, &wi);
        if (c.out.out_caps && fmt != ROWS_DENSE) return fail(GX_E_ARG, name + ": out_caps on compact rows (out_ids holds whole rows)");
        if (n >= 0xFFFFFFFFull) return fail(GX_E_LIMIT, name + ": line numbers are 32 bits and two are kept for \"none\" and \"miss\"; split batches of 2^32 - 1 lines and more");
        const std::pair<uint64_t, uint64_t> named = lookup_dict_refusals(o, c, name);
        if ((n_parts || !wi.none()) && fmt == ROWS_DENSE && n && !caps) return fail(GX_E_ARG, name + ": parts and terms on dense ids need caps");
        if (!o.device_pointers) refuse_long_host_lines({offsets, o.offsets64 != 0, n}, name, "looked up");
        const size_t slots = 2 * static_cast<size_t>(h->T.max_groups);
        if (c.out.out_caps && slots && n && !caps) return fail(GX_E_ARG, name + ": out_caps without caps");
        if (!slots) c.out.out_caps = nullptr;
        {
            const gx_lookup_out& b = c.out;
            const uint64_t ow = o.offsets64 ? 8 : 4, un = o.utf16 ? 2 : 1, idr = static_cast<uint64_t>(row_units) * row_unit_bytes(fmt), m = n_entries;
            const uint64_t in_units = o.device_pointers ? (n ? 1u : 0u) : HostOffsets{offsets, o.offsets64 != 0, n}[n];
            const uint64_t cap = std::min<uint64_t>(b.cap_lines, n);   // (no more than n lines leave, whatever the capacity says: n < 2^32, no product wraps)
            const std::pair<const void*, uint64_t> outs[10] = {{b.line_entry, n * 4}, {b.entry_same, m * 4}, {b.entry_lines, m * 8}, {b.entry_first_line, m * 4},
                                                               {b.entry_stats, m * 64}, {b.out_index, cap * 4}, {b.out_bytes, b.out_bytes_cap},
                                                               {b.out_offsets, (cap + 1) * ow}, {b.out_ids, cap * idr}, {b.out_caps, cap * slots * 4}};
            std::pair<const void*, uint64_t> ins[6] = {{bytes, in_units * un}, {offsets, (n + 1) * ow}, {ids, n * idr}, {fmt == ROWS_DENSE ? caps : nullptr, n * slots * 4}, {}, {}};
            lookup_dict_ranges(o, c, named, ins + 4);
            by_key_overlaps(outs, 10, ins, 6, name);
        }
        if (!h->on_device) return fail(GX_E_DEVICE, "handle was created host-only; no device tables (there is no CPU fallback)");
        if (fmt != ROWS_DENSE) caps = nullptr;
        GX_HIP(hipSetDevice(h->device));
        std::lock_guard<std::mutex> lock(h->mu);
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        const StagedLines in = stage_lines(h, bytes, offsets, n, ids, caps, o, fmt, row_units, Travels{true, caps != nullptr}, stream, name.c_str());
        const StagedDict sd = stage_dict(c, o, named, flags, stream);
        return lookup_pass(h, in.v, gi, wi, c, sd.d, !o.device_pointers, true, nullptr, stream, name);
    });
}

int gx_text_lookup_lines(gx_handle* h, const uint8_t* text, uint64_t size, const gx_group_part* parts, uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms,
                         const void* entry_units, const void* entry_offsets, uint64_t n_entries, uint32_t keep, uint32_t flags, const gx_lookup_out* out, uint8_t* kept,
                         uint64_t kept_cap, void* kept_offsets, uint32_t* kept_index, gx_lookup_totals* totals, uint64_t* counts, uint64_t* n_lines,
                         const gx_batch_opts* opts) {
    const std::string name = "gx_text_lookup_lines";
    return guarded([&]() -> int {
        if (!h || (size && !text)) return fail(GX_E_ARG, name + ": bad argument");
        const gx_batch_opts o = read_opts(opts);
        LookupCall c{entry_units, entry_offsets, n_entries, keep, out ? *out : gx_lookup_out{}, totals};
        if (c.batch_out()) return fail(GX_E_ARG, name + ": the five batch outputs of `out` must be NULL (kept, kept_offsets and kept_index take the kept lines)");
        c.out.out_bytes = kept; c.out.out_offsets = kept_offsets; c.out.out_index = kept_index;
        c.out.cap_lines = ~0ull;   // (sized by the size query: the header)
        c.out.out_bytes_cap = kept_cap;
        GroupImage gi;
        WhereImage wi;
        lookup_refusals(h, o, parts, n_parts, terms, n_terms, flags, false, c, name, &gi, &wi);
        const std::pair<uint64_t, uint64_t> named = lookup_dict_refusals(o, c, name);
        {
            const gx_lookup_out& b = c.out;
            const uint64_t m = n_entries;
            // (the per-line arrays are as long as the text has lines, which nobody knows yet: their first bytes stand for them)
            const std::pair<const void*, uint64_t> outs[8] = {{b.line_entry, 4}, {b.entry_same, m * 4}, {b.entry_lines, m * 8}, {b.entry_first_line, m * 4},
                                                              {b.entry_stats, m * 64}, {b.out_bytes, b.out_bytes_cap}, {b.out_offsets, 4}, {b.out_index, 4}};
            std::pair<const void*, uint64_t> ins[3] = {{text, size}, {}, {}};
            lookup_dict_ranges(o, c, named, ins + 1);
            by_key_overlaps(outs, 8, ins, 3, name);
        }
        if (size > 0xFFFFFFFFull) return fail(GX_E_LIMIT, name + ": split texts of 4 GiB and more at a line boundary");
        if (!h->on_device) return fail(GX_E_DEVICE, "handle was created host-only; no device tables (there is no CPU fallback)");
        GX_HIP(hipSetDevice(h->device));
        std::lock_guard<std::mutex> lock(h->mu);
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        // the text's lines and the path; then the passes over the ids, offsets and capture rows they left on the device
        const TextBatch tb = stage_text_lines(h, text, size, o, stream, name.c_str());
        if (n_lines) *n_lines = tb.v.n;
        const StagedDict sd = stage_dict(c, o, named, flags, stream);
        // (the emits read what text_lines left in the handle's scratch buffers, which the next whole-file call overwrites: the pass waits for them)
        const int rc = lookup_pass(h, tb.v, gi, wi, c, sd.d, !o.device_pointers, false, counts, stream, name);
        if (promise_broken_since(h, stream)) throw GxError(GX_E_ARG, "internal: " + name + ": a line longer than the split pass reported");
        return rc;
    });
}

// The parts of a gx_bucket_lines call as its kernels read them (gx_bucket.hpp: BucketHead), checked against the handle.  Needs no device.
struct BucketImage {
    BucketHead head{};
    bool values = false;
};
static BucketImage bucket_image(const gx_handle* h, const gx_bucket_part* parts, uint32_t n_parts, int64_t origin, int64_t width, uint32_t flags,
                                const std::string& name) {
    BucketImage img;
    if (flags & ~static_cast<uint32_t>(GX_GROUP_WEAK_HASH | GX_BUCKET_ALL_DIGITS)) throw GxError(GX_E_ARG, name + ": unknown flag bits");
    if (width < 1) throw GxError(GX_E_ARG, name + ": width below 1");
    img.head.flags = flags;
    img.head.origin = origin;
    img.head.width = static_cast<uint64_t>(width);
    if (n_parts == 0) return img;
    if (!parts) throw GxError(GX_E_ARG, name + ": parts is NULL");
    if (n_parts > BUCKET_MAX_PARTS) throw GxError(GX_E_LIMIT, name + ": more than 64 parts");
    const int32_t K = static_cast<int32_t>(h->T.n_rules);
    std::vector<uint32_t> order(n_parts);
    for (uint32_t t = 0; t < n_parts; ++t) {
        const gx_bucket_part& p = parts[t];
        order[t] = t;
        if (p.extraction < 0 || p.extraction >= K) throw GxError(GX_E_ARG, name + ": a part's extraction is not in [0, K)");
        const int32_t groups = gx_num_groups(h, p.extraction);
        if (p.number_group < 0 || p.number_group >= groups) throw GxError(GX_E_ARG, name + ": a part's number_group is not one of its extraction's");
        if (p.value_group < -1 || p.value_group >= groups) throw GxError(GX_E_ARG, name + ": a part's value_group is neither -1 nor one of its extraction's");
        if (p.reserved != 0) throw GxError(GX_E_ARG, name + ": a part's reserved is not 0");
        if (p.value_group >= 0) img.values = true;
    }
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return parts[a].extraction < parts[b].extraction; });
    for (uint32_t q = 0; q < n_parts; ++q) {
        const gx_bucket_part& p = parts[order[q]];
        if (q && parts[order[q - 1]].extraction == p.extraction) throw GxError(GX_E_ARG, name + ": two parts for one extraction");
        img.head.ext[q] = static_cast<uint32_t>(p.extraction);
        img.head.part[q].key_group = static_cast<uint16_t>(p.number_group);
        img.head.part[q].value_group = p.value_group < 0 ? static_cast<uint16_t>(GROUP_NO_VALUE) : static_cast<uint16_t>(p.value_group);
        img.head.nfmt[q] = h->number_format_of(p.extraction, p.number_group);
        if (p.value_group >= 0) img.head.vfmt[q] = h->number_format_of(p.extraction, p.value_group);
        if (img.head.nfmt[q] || img.head.vfmt[q]) img.head.formats = 1u;
    }
    img.head.n_parts = n_parts;
    img.head.has_values = img.values ? 1u : 0u;
    return img;
}

// what both bucket calls refuse before they look at the device: group_refusals' list in its order, with the width behind the flags
static void bucket_refusals(const gx_handle* h, const gx_batch_opts& o, const gx_bucket_part* parts, uint32_t n_parts, int64_t origin, int64_t width,
                            const gx_where_term* terms, uint32_t n_terms, uint32_t flags, bool wide, const gx_bucket_out& out, const gx_bucket_totals* totals,
                            const std::string& name, BucketImage* bi, WhereImage* wi) {
    if (!totals) throw GxError(GX_E_ARG, name + ": totals is NULL");
    *bi = bucket_image(h, parts, n_parts, origin, width, flags, name);
    if (out.bucket_stats && !bi->values) throw GxError(GX_E_ARG, name + ": bucket_stats without a value_group");
    if (o.utf8 == 2) throw GxError(GX_E_ARG, name + ": gx_batch_opts.utf8 = 1 (values are read in the units the offsets count)");
    *wi = where_image(h, terms, n_terms, wide, name);
    if (o.no_sync) throw GxError(GX_E_ARG, name + ": no_sync: the totals are host values");
    if (out.max_buckets > BUCKET_MAX_BUCKETS) throw GxError(GX_E_LIMIT, name + ": max_buckets above 2^30");
}

// The passes on the handle's buffers (under h->mu): build, flags and the scan; ONE synchronisation of the stream, where the host reads
// the totals, the buckets and the range of their words and checks the capacity; then the pairs, the sort and the emits.  out: the
// caller's, device or host (host_out: staged, and a second wait delivers them).  counts: also the histogram of outcomes
// (gx_text_bucket_lines).
static int bucket_pass(gx_handle* h, const BatchView& v, const BucketImage& bi, const WhereImage& wi, const gx_bucket_out& out, bool host_out,
                       gx_bucket_totals* totals, uint64_t* counts, hipStream_t stream, const std::string& name) {
    const uint32_t K = static_cast<uint32_t>(h->T.n_rules);
    const uint64_t n = v.n;
    if (counts) counts_beside(h, v, counts, stream);
    *totals = gx_bucket_totals{};
    totals->exact = 1;
    const bool per_bucket = out.bucket_number || out.bucket_first_line || out.bucket_lines || out.bucket_stats;
    const bool any_out = per_bucket || out.line_bucket;
    if (n == 0 || bi.head.n_parts == 0) {
        GX_HIP(hipStreamSynchronize(stream));
        fill_out(out.line_bucket, 0xFF, n * 4, host_out, stream);   // no line has a bucket
        return GX_OK;
    }
    wait_pending(h->bucket_event, h->bucket_pending, stream);
    const uint32_t n_slots = group_slots(out.max_buckets);
    const DevImage img = upload_image(h->bucket_image, &bi.head, sizeof(BucketHead), nullptr, wi, stream);
    const GroupArgs a{v.data, v.wide ? 1 : 0, v.caps, 2u * static_cast<uint32_t>(h->T.max_groups), img.head, img.terms,
                      static_cast<uint32_t>(wi.bytes.size()), bi.values ? 1u : 0u, (bi.head.formats || wi.formats) ? 1u : 0u};
    const BucketWs w = bucket_workspace(h->bucket_table.get(bucket_table_bytes(n_slots, bi.values)), h->bucket_lines.get(bucket_lines_bytes(n)), n, n_slots, bi.values);
    GX_HIP(launch_bucket_build(v.ids, v.fmt, v.row_units, K, n, v.offsets, v.off64 ? 1 : 0, a, w, stream));
    BucketDev got{};
    uint64_t n_buckets = 0;
    GX_HIP(hipMemcpyAsync(&got, w.totals, sizeof(got), hipMemcpyDeviceToHost, stream));
    GX_HIP(hipMemcpyAsync(&n_buckets, w.before + n_slots, 8, hipMemcpyDeviceToHost, stream));
    GX_HIP(hipStreamSynchronize(stream));
    if (got.status & 1u) throw GxError(GX_E_LIMIT, "a line of 4 G code units or more cannot be bucketed");
    if (got.unset + got.not_numbers + got.out_of_range > got.lines) throw GxError(GX_E_ARG, "internal: " + name + ": the classes exceed the lines that count");
    totals->lines = got.lines;
    totals->unset = got.unset;
    totals->not_numbers = got.not_numbers;
    totals->out_of_range = got.out_of_range;
    totals->bucketed = got.lines - got.unset - got.not_numbers - got.out_of_range;
    totals->n_buckets = n_buckets;
    const uint64_t min_word = ~got.min_inv, max_word = got.max_word;
    if (n_buckets) {
        totals->first_bucket = bucket_number(min_word);
        totals->last_bucket = bucket_number(max_word);
    }
    if (got.status & 2u) {
        totals->exact = 0;
        totals->n_buckets = static_cast<uint64_t>(n_slots) + 1u;
        return fail(GX_E_LIMIT, name + ": the table of " + std::to_string(n_slots) + " slots is full; the number of lines is always a sufficient max_buckets");
    }
    if (!any_out) return GX_OK;
    if (per_bucket && n_buckets > out.max_buckets)
        return fail(GX_E_LIMIT, name + ": " + std::to_string(n_buckets) + " buckets, max_buckets " + std::to_string(out.max_buckets));
    if (n_buckets == 0) {   // lines, and none of them bucketed
        fill_out(out.line_bucket, 0xFF, n * 4, host_out, stream);
        return GX_OK;
    }
    HostTwins twins(host_out);
    const BucketOut o{twins.of(out.bucket_number, n_buckets * 8), twins.of(out.bucket_first_line, n_buckets * 4), twins.of(out.bucket_lines, n_buckets * 8),
                      twins.of(reinterpret_cast<uint64_t*>(out.bucket_stats), n_buckets * 64), twins.of(out.line_bucket, n * 4)};
    const uint32_t n_digits = (bi.head.flags & BUCKET_ALL_DIGITS) ? BUCKET_MAX_DIGITS : bucket_digits(min_word, max_word);
    const BucketSortWs sw = bucket_sort_workspace(h->bucket_sort.get(bucket_sort_workspace_bytes(n_buckets)), n_buckets);
    GX_HIP(launch_bucket_emit(n, n_buckets, n_digits, w, sw, o, stream));
    if (host_out) {
        twins.deliver(stream);
        GX_HIP(hipStreamSynchronize(stream));
    } else {
        leave_pending(h->bucket_event, h->bucket_pending, stream);
    }
    return GX_OK;
}
static_assert(sizeof(gx_bucket_out) == 48 && sizeof(gx_bucket_totals) == 72 && sizeof(gx_bucket_part) == 16, "include/gorp_hip.h states these sizes");

int gx_bucket_lines(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps, const gx_bucket_part* parts,
                    uint32_t n_parts, int64_t origin, int64_t width, const gx_where_term* terms, uint32_t n_terms, uint32_t flags, const gx_bucket_out* out,
                    gx_bucket_totals* totals, const gx_batch_opts* opts) {
    const std::string name = "gx_bucket_lines";
    return guarded([&]() -> int {
        if (!h || !offsets || (n && !ids)) return fail(GX_E_ARG, name + ": bad argument");
        const gx_batch_opts o = read_opts(opts);
        uint32_t row_units = 1;
        const RowFormat fmt = id_format(h, o, &row_units);
        const gx_bucket_out none{};
        const gx_bucket_out& bo = out ? *out : none;
        BucketImage bi;
        WhereImage wi;
        bucket_refusals(h, o, parts, n_parts, origin, width, terms, n_terms, flags, o.utf16 != 0, bo, totals, name, &bi, &wi);
        if ((n_parts || !wi.none()) && fmt == ROWS_DENSE && n && !caps) return fail(GX_E_ARG, name + ": parts and terms on dense ids need caps");
        if (n >= 0xFFFFFFFFull) return fail(GX_E_LIMIT, name + ": line numbers are 32 bits and one is kept for \"none\"; split batches of 2^32 - 1 lines and more");
        if (!o.device_pointers) refuse_long_host_lines({offsets, o.offsets64 != 0, n}, name, "bucketed");
        if (!h->on_device) return fail(GX_E_DEVICE, "handle was created host-only; no device tables (there is no CPU fallback)");
        if (fmt != ROWS_DENSE) caps = nullptr;
        GX_HIP(hipSetDevice(h->device));
        std::lock_guard<std::mutex> lock(h->mu);
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        const StagedLines in = stage_lines(h, bytes, offsets, n, ids, caps, o, fmt, row_units, Travels{true, caps != nullptr}, stream, name.c_str());
        return bucket_pass(h, in.v, bi, wi, bo, !o.device_pointers, totals, nullptr, stream, name);
    });
}

int gx_text_bucket_lines(gx_handle* h, const uint8_t* text, uint64_t size, const gx_bucket_part* parts, uint32_t n_parts, int64_t origin, int64_t width,
                         const gx_where_term* terms, uint32_t n_terms, uint32_t flags, const gx_bucket_out* out, gx_bucket_totals* totals, uint64_t* counts,
                         uint64_t* n_lines, const gx_batch_opts* opts) {
    const std::string name = "gx_text_bucket_lines";
    return guarded([&]() -> int {
        if (!h || (size && !text)) return fail(GX_E_ARG, name + ": bad argument");
        const gx_batch_opts o = read_opts(opts);
        const gx_bucket_out none{};
        const gx_bucket_out& bo = out ? *out : none;
        BucketImage bi;
        WhereImage wi;
        bucket_refusals(h, o, parts, n_parts, origin, width, terms, n_terms, flags, false, bo, totals, name, &bi, &wi);
        if (size > 0xFFFFFFFFull) return fail(GX_E_LIMIT, name + ": split texts of 4 GiB and more at a line boundary");
        if (!h->on_device) return fail(GX_E_DEVICE, "handle was created host-only; no device tables (there is no CPU fallback)");
        GX_HIP(hipSetDevice(h->device));
        std::lock_guard<std::mutex> lock(h->mu);
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        // the text's lines and the path; then the passes over the ids, offsets and capture rows they left on the device
        const TextBatch tb = stage_text_lines(h, text, size, o, stream, name.c_str());
        if (n_lines) *n_lines = tb.v.n;
        const int rc = bucket_pass(h, tb.v, bi, wi, bo, !o.device_pointers, totals, counts, stream, name);
        // (gx_text_group_lines' reason: the emit reads what text_lines left in the handle's scratch buffers)
        if (h->bucket_pending) {
            GX_HIP(hipStreamSynchronize(stream));
            h->bucket_pending = false;
        }
        if (promise_broken_since(h, stream)) throw GxError(GX_E_ARG, "internal: " + name + ": a line longer than the split pass reported");
        return rc;
    });
}

// gx_top_groups' own arguments as gx_group_lines' callers take them: the flags without GX_TOP_GROUPS_SMALLEST and &totals->group (unknown
// flag bits stay in the flags and are refused there), and a gx_group_out that holds what gx_group_lines' refusals look at.
static GroupExtras top_groups_extras(uint32_t rank_by, uint32_t n_wanted, uint32_t flags, const gx_top_groups_out* out, gx_top_groups_totals* totals) {
    TopGroupsCall tg;
    tg.rank_by = rank_by;
    tg.n_wanted = n_wanted;
    tg.smallest = (flags & GX_TOP_GROUPS_SMALLEST) ? 1u : 0u;
    if (out) tg.out = *out;
    tg.totals = totals;
    GroupExtras x;
    x.top = tg;
    return x;
}
static gx_group_out top_groups_keys(const gx_top_groups_out* out, uint64_t max_keys) {
    gx_group_out go{};
    go.key_stats = out ? out->key_stats : nullptr;
    go.max_keys = max_keys;
    return go;
}

int gx_top_groups(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps, const gx_group_part* parts,
                  uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms, uint32_t rank_by, uint32_t n_wanted, uint64_t max_keys, uint32_t flags,
                  const gx_top_groups_out* out, gx_top_groups_totals* totals, const gx_batch_opts* opts) {
    const gx_group_out go = top_groups_keys(out, max_keys);
    return group_lines_call("gx_top_groups", h, bytes, offsets, n, ids, caps, parts, n_parts, terms, n_terms, flags & ~static_cast<uint32_t>(GX_TOP_GROUPS_SMALLEST), &go,
                            totals ? &totals->group : nullptr, opts, top_groups_extras(rank_by, n_wanted, flags, out, totals));
}

int gx_text_top_groups(gx_handle* h, const uint8_t* text, uint64_t size, const gx_group_part* parts, uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms,
                       uint32_t rank_by, uint32_t n_wanted, uint64_t max_keys, uint32_t flags, const gx_top_groups_out* out, gx_top_groups_totals* totals,
                       uint64_t* counts, uint64_t* n_lines, const gx_batch_opts* opts) {
    const gx_group_out go = top_groups_keys(out, max_keys);
    return text_group_call("gx_text_top_groups", h, text, size, parts, n_parts, terms, n_terms, flags & ~static_cast<uint32_t>(GX_TOP_GROUPS_SMALLEST), &go,
                           totals ? &totals->group : nullptr, counts, n_lines, opts, top_groups_extras(rank_by, n_wanted, flags, out, totals));
}

// The parts of a gx_top_lines call as its keys pass reads them (gx_top.hpp: TopHead), checked against the handle.  Needs no device.
static TopHead top_image(const gx_handle* h, const gx_top_part* parts, uint32_t n_parts, uint32_t flags, const std::string& name) {
    TopHead head{};
    if (flags & ~static_cast<uint32_t>(GX_TOP_SMALLEST)) throw GxError(GX_E_ARG, name + ": unknown flag bits");
    head.smallest = (flags & GX_TOP_SMALLEST) ? 1u : 0u;
    if (n_parts == 0) return head;
    if (!parts) throw GxError(GX_E_ARG, name + ": parts is NULL");
    if (n_parts > TOP_MAX_PARTS) throw GxError(GX_E_LIMIT, name + ": more than 64 parts");
    const int32_t K = static_cast<int32_t>(h->T.n_rules);
    std::vector<uint32_t> order(n_parts);
    for (uint32_t t = 0; t < n_parts; ++t) {
        const gx_top_part& p = parts[t];
        order[t] = t;
        if (p.extraction < 0 || p.extraction >= K) throw GxError(GX_E_ARG, name + ": a part's extraction is not in [0, K)");
        if (p.value_group < 0 || p.value_group >= gx_num_groups(h, p.extraction))
            throw GxError(GX_E_ARG, name + ": a part's value_group is not one of its extraction's");
    }
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return parts[a].extraction < parts[b].extraction; });
    for (uint32_t q = 0; q < n_parts; ++q) {
        const gx_top_part& p = parts[order[q]];
        if (q && parts[order[q - 1]].extraction == p.extraction) throw GxError(GX_E_ARG, name + ": two parts for one extraction");
        head.ext[q] = static_cast<uint32_t>(p.extraction);
        head.group[q] = static_cast<uint16_t>(p.value_group);
        head.fmt[q] = h->number_format_of(p.extraction, p.value_group);
        if (head.fmt[q]) head.formats = 1u;
    }
    head.n_parts = n_parts;
    return head;
}

// what both top-lines calls refuse before they look at the device
static void top_refusals(const gx_handle* h, const gx_batch_opts& o, const gx_top_part* parts, uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms,
                         uint32_t n_wanted, uint32_t flags, bool wide, const gx_top_totals* totals, const std::string& name, TopHead* ti, WhereImage* wi) {
    if (!totals) throw GxError(GX_E_ARG, name + ": totals is NULL");
    *ti = top_image(h, parts, n_parts, flags, name);
    if (o.utf8 == 2) throw GxError(GX_E_ARG, name + ": gx_batch_opts.utf8 = 1 (values are read in the units the offsets count)");
    *wi = where_image(h, terms, n_terms, wide, name);
    if (o.no_sync) throw GxError(GX_E_ARG, name + ": no_sync: the totals are host values");
    if (n_wanted > GX_TOP_MAX_LINES) throw GxError(GX_E_LIMIT, name + ": n_wanted above GX_TOP_MAX_LINES");
}

// where the delivered lines go: the caller's pointers, device or host (host_out: staged, and a second wait delivers them)
struct TopOut {
    LinesOut lines;
    int64_t* values;
    uint64_t cap_lines, bytes_cap;
    bool any() const { return lines.any() || values; }
};

// The passes on the handle's workspace (under h->mu): keys, select, choose and order; ONE synchronisation of the stream, where the host
// reads the totals and checks the capacities; then the emit (launch_partition_copy).  counts: also the histogram of outcomes
// (gx_text_top_lines).
static int top_pass(gx_handle* h, const BatchView& v, const TopHead& ti, const WhereImage& wi, uint32_t n_wanted, const TopOut& out, bool host_out,
                    gx_top_totals* totals, uint64_t* counts, hipStream_t stream, const std::string& name) {
    const uint32_t K = static_cast<uint32_t>(h->T.n_rules);
    const size_t slots = 2 * static_cast<size_t>(h->T.max_groups);
    const uint64_t n = v.n;
    if (counts) counts_beside(h, v, counts, stream);
    *totals = gx_top_totals{};
    const size_t unit = v.wide ? 2 : 1, off_w = v.off64 ? 8 : 4;
    if (n == 0 || ti.n_parts == 0) {
        GX_HIP(hipStreamSynchronize(stream));
        fill_out(out.lines.offsets, 0, off_w, host_out, stream);   // no lines: the offsets' one entry
        return GX_OK;
    }
    wait_pending(h->top_event, h->top_pending, stream);
    const DevImage img = upload_image(h->top_image, &ti, sizeof(TopHead), nullptr, wi, stream);
    const TopArgs a{v.data, v.wide ? 1 : 0, v.caps, static_cast<uint32_t>(slots), img.head, img.terms,
                    static_cast<uint32_t>(wi.bytes.size()), ti.smallest, n_wanted, (ti.formats || wi.formats) ? 1u : 0u};
    const TopWs w = top_workspace(h->top_ws.get(top_workspace_bytes(n)), n);
    GX_HIP(launch_top_select(v.ids, v.fmt, v.row_units, K, n, v.offsets, v.off64 ? 1 : 0, a, w, stream));
    struct { uint32_t counts[TOP_COUNTS]; TopSelect sel; } got{};
    static_assert(sizeof(got) == offsetof(TopDev, spare), "the head's first words");
    uint64_t both = 0, units = 0;
    GX_HIP(hipMemcpyAsync(&got, w.head, sizeof(got), hipMemcpyDeviceToHost, stream));
    if (n_wanted) {
        GX_HIP(hipMemcpyAsync(&both, w.before + n, 8, hipMemcpyDeviceToHost, stream));
        GX_HIP(hipMemcpyAsync(&units, w.dst_off + n_wanted, 8, hipMemcpyDeviceToHost, stream));
    }
    GX_HIP(hipStreamSynchronize(stream));
    if (got.counts[TOP_C_STATUS]) throw GxError(GX_E_LIMIT, "a line of 4 G code units or more cannot be ranked");
    totals->numbers = got.counts[TOP_C_NUMBERS];
    totals->unset = got.counts[TOP_C_UNSET];
    totals->not_numbers = got.counts[TOP_C_NOT_NUMBERS];
    totals->lines = totals->numbers + totals->unset + totals->not_numbers;
    const uint64_t n_top = got.sel.n_top;
    totals->n_top = n_top;
    totals->units_top = units;
    if (n_top) {
        // the last delivered line holds the threshold key: the select always takes at least one of its ties
        totals->last_value = top_value(got.sel.prefix, ti.smallest != 0);
        totals->ties_left = (both >> 32) - got.sel.remaining;
    }
    if (!out.any()) return GX_OK;   // size query
    if ((out.lines.per_line() || out.values) && n_top > out.cap_lines) return fail(GX_E_LIMIT, name + ": cap_lines is smaller than the result (see totals->n_top)");
    if (out.lines.bytes && units * unit > out.bytes_cap)
        return fail(GX_E_LIMIT, name + ": the delivered text is larger than the capacity (see totals->units_top)");
    if (out.lines.offsets && !v.off64 && units > 0xFFFFFFFFull) return fail(GX_E_LIMIT, name + ": 4 G code units and more need offsets64");
    const StagedLinesOut so = stage_lines_out(h, v, out.lines, host_out, n_top, units);
    if (so.dev.offsets && n_top == 0) GX_HIP(hipMemsetAsync(so.dev.offsets, 0, off_w, stream));
    PartWs pw{};   // (the copy pass reads the permutation and the output offsets alone)
    pw.perm_sorted = w.perm;
    pw.dst_off = w.dst_off;
    GX_HIP(launch_partition_copy(so.dev, v.data, v.offsets, v.off64 ? 1 : 0, v.wide ? 1 : 0, n, n_top, pw, stream));
    if (out.values && n_top) GX_HIP(hipMemcpyAsync(out.values, w.values, n_top * 8, host_out ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, stream));
    if (host_out) {
        so.deliver(stream);
        GX_HIP(hipStreamSynchronize(stream));
    } else {
        leave_pending(h->top_event, h->top_pending, stream);
    }
    return GX_OK;
}

int gx_top_lines(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps, const gx_top_part* parts,
                 uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms, uint32_t n_wanted, uint32_t flags, uint32_t* out_index, int64_t* out_values,
                 void* out_bytes, void* out_offsets, void* out_ids, int32_t* out_caps, uint64_t cap_lines, uint64_t out_bytes_cap, gx_top_totals* totals,
                 const gx_batch_opts* opts) {
    const std::string name = "gx_top_lines";
    return guarded([&]() -> int {
        if (!h || !offsets || (n && !ids)) return fail(GX_E_ARG, name + ": bad argument");
        const gx_batch_opts o = read_opts(opts);
        uint32_t row_units = 1;
        const RowFormat fmt = id_format(h, o, &row_units);
        TopHead ti;
        WhereImage wi;
        top_refusals(h, o, parts, n_parts, terms, n_terms, n_wanted, flags, o.utf16 != 0, totals, name, &ti, &wi);
        if ((n_parts || !wi.none()) && fmt == ROWS_DENSE && n && !caps) return fail(GX_E_ARG, name + ": parts and terms on dense ids need caps");
        if (n >= 0xFFFFFFFFull) return fail(GX_E_LIMIT, name + ": line numbers are 32 bits; split batches of 2^32 - 1 lines and more");
        if (!o.device_pointers) refuse_long_host_lines({offsets, o.offsets64 != 0, n}, name, "ranked");
        if (!h->on_device) return fail(GX_E_DEVICE, "handle was created host-only; no device tables (there is no CPU fallback)");
        const size_t slots = 2 * static_cast<size_t>(h->T.max_groups);
        if (fmt != ROWS_DENSE) { caps = nullptr; out_caps = nullptr; }
        if (out_caps && slots && n && !caps) return fail(GX_E_ARG, name + ": out_caps without caps");
        if (!slots) out_caps = nullptr;
        GX_HIP(hipSetDevice(h->device));
        std::lock_guard<std::mutex> lock(h->mu);
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        const StagedLines in = stage_lines(h, bytes, offsets, n, ids, caps, o, fmt, row_units, Travels{true, caps != nullptr}, stream, name.c_str());
        const TopOut out{{out_index, out_bytes, out_offsets, out_ids, out_caps}, out_values, cap_lines, out_bytes_cap};
        return top_pass(h, in.v, ti, wi, n_wanted, out, !o.device_pointers, totals, nullptr, stream, name);
    });
}

int gx_text_top_lines(gx_handle* h, const uint8_t* text, uint64_t size, const gx_top_part* parts, uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms,
                      uint32_t n_wanted, uint32_t flags, uint32_t* out_index, int64_t* out_values, uint8_t* out, uint64_t out_cap, uint64_t* out_size,
                      gx_top_totals* totals, uint64_t* counts, uint64_t* n_lines, const gx_batch_opts* opts) {
    const std::string name = "gx_text_top_lines";
    return guarded([&]() -> int {
        if (!h || (size && !text)) return fail(GX_E_ARG, name + ": bad argument");
        const gx_batch_opts o = read_opts(opts);
        TopHead ti;
        WhereImage wi;
        top_refusals(h, o, parts, n_parts, terms, n_terms, n_wanted, flags, false, totals, name, &ti, &wi);
        if (size > 0xFFFFFFFFull) return fail(GX_E_LIMIT, name + ": split texts of 4 GiB and more at a line boundary");
        if (!h->on_device) return fail(GX_E_DEVICE, "handle was created host-only; no device tables (there is no CPU fallback)");
        GX_HIP(hipSetDevice(h->device));
        std::lock_guard<std::mutex> lock(h->mu);
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        // the text's lines and the path; then the passes over the ids, offsets and capture rows they left on the device
        const TextBatch tb = stage_text_lines(h, text, size, o, stream, name.c_str());
        if (n_lines) *n_lines = tb.v.n;
        const TopOut to{{out_index, out, nullptr, nullptr, nullptr}, out_values, n_wanted, out_cap};
        const int rc = top_pass(h, tb.v, ti, wi, n_wanted, to, !o.device_pointers, totals, counts, stream, name);
        if (out_size) *out_size = totals->units_top;
        // The emit pass reads the offsets that text_lines left in the handle's scratch buffers, which the next whole-file call on any
        // stream overwrites: like every gx_text_* call this one returns with its work done.
        if (h->top_pending) {
            GX_HIP(hipStreamSynchronize(stream));
            h->top_pending = false;
        }
        if (promise_broken_since(h, stream)) throw GxError(GX_E_ARG, "internal: " + name + ": a line longer than the split pass reported");
        return rc;
    });
}

// where gx_sort_lines' delivered lines go: the caller's pointers, device or host (host_out: staged, and a second wait delivers them)
struct SortOut {
    LinesOut lines;
    int64_t* values;
    uint8_t* cls;
    uint64_t cap_lines, bytes_cap;
    bool per_line() const { return lines.per_line() || values || cls; }
    bool any() const { return lines.any() || values || cls; }
};

// what both sort calls refuse before they look at the batch: gx_top_lines' refusals of parts and terms, in its order
static void sort_refusals(const gx_handle* h, const gx_batch_opts& o, const gx_top_part* parts, uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms,
                          uint32_t flags, bool wide, const gx_sort_totals* totals, const std::string& name, TopHead* ti, WhereImage* wi) {
    if (!totals) throw GxError(GX_E_ARG, name + ": totals is NULL");
    if (flags & ~SORT_FLAGS) throw GxError(GX_E_ARG, name + ": unknown flag bits");
    *ti = top_image(h, parts, n_parts, (flags & GX_SORT_DESCENDING) ? GX_TOP_SMALLEST : 0u, name);   // (key ascending: top_key(value, descending))
    if (o.utf8 == 2) throw GxError(GX_E_ARG, name + ": gx_batch_opts.utf8 = 1 (values are read in the units the offsets count)");
    *wi = where_image(h, terms, n_terms, wide, name);
    if (o.no_sync) throw GxError(GX_E_ARG, name + ": no_sync: the totals are host values");
}

// The passes on the handle's workspace (under h->mu): keys, scan, compaction, entries and totals; ONE synchronisation of the stream,
// where the host reads the totals, plans the digits and checks the capacities; then the sort, the finish, the scan of the lengths and
// the copy (launch_partition_copy).  counts: also the histogram of outcomes (gx_text_sort_lines).
static int sort_pass(gx_handle* h, const BatchView& v, const TopHead& ti, const WhereImage& wi, uint32_t flags, const SortOut& out, bool host_out,
                     gx_sort_totals* totals, uint64_t* counts, hipStream_t stream, const std::string& name) {
    const uint32_t K = static_cast<uint32_t>(h->T.n_rules);
    const size_t slots = 2 * static_cast<size_t>(h->T.max_groups);
    const uint64_t n = v.n;
    if (counts) counts_beside(h, v, counts, stream);
    *totals = gx_sort_totals{};
    totals->already_ordered = 1;
    const size_t unit = v.wide ? 2 : 1, off_w = v.off64 ? 8 : 4;
    if (n == 0) {
        GX_HIP(hipStreamSynchronize(stream));
        fill_out(out.lines.offsets, 0, off_w, host_out, stream);   // no lines: the offsets' one entry
        return GX_OK;
    }
    wait_pending(h->sort_event, h->sort_pending, stream);
    const SortWs w = sort_workspace(h->sort_ws.get(sort_workspace_bytes(n)), n);
    if (ti.n_parts) {
        const DevImage img = upload_image(h->sort_image, &ti, sizeof(TopHead), nullptr, wi, stream);
        const TopArgs a{v.data, v.wide ? 1 : 0, v.caps, static_cast<uint32_t>(slots), img.head, img.terms,
                        static_cast<uint32_t>(wi.bytes.size()), ti.smallest, 0u, (ti.formats || wi.formats) ? 1u : 0u};
        GX_HIP(launch_sort_entries(v.ids, v.fmt, v.row_units, K, n, v.offsets, v.off64 ? 1 : 0, &a, flags, w, stream));
    } else {
        GX_HIP(launch_sort_entries(v.ids, v.fmt, v.row_units, K, n, v.offsets, v.off64 ? 1 : 0, nullptr, flags, w, stream));   // (no part: every line is a rest line)
    }
    SortDev sd{};
    GX_HIP(hipMemcpyAsync(&sd, w.head, sizeof(SortDev), hipMemcpyDeviceToHost, stream));
    GX_HIP(hipStreamSynchronize(stream));
    if (sd.counts[TOP_C_STATUS]) throw GxError(GX_E_LIMIT, "a line of 4 G code units or more cannot be sorted");
    if (sd.entries > n || sd.rest > n - sd.entries || sd.carried > sd.entries) throw GxError(GX_E_ARG, "internal: " + name + ": more entries or rest lines than there are");
    const bool descending = (flags & GX_SORT_DESCENDING) != 0u;
    const uint64_t m = sd.entries, lines_out = m + ((flags & GX_SORT_REST_LAST) ? sd.rest : 0u), units = sd.units_out;
    const SortPlan plan = sort_plan(sd.key_or, sd.key_and, m, (flags & GX_SORT_ALL_DIGITS) != 0u);
    totals->numbers = sd.counts[TOP_C_NUMBERS];
    totals->unset = sd.counts[TOP_C_UNSET];
    totals->not_numbers = sd.counts[TOP_C_NOT_NUMBERS];
    totals->lines = totals->numbers + totals->unset + totals->not_numbers;
    totals->carried = sd.carried;
    totals->rest = sd.rest;
    totals->lines_out = lines_out;
    totals->units_out = units;
    if (m) {
        totals->first_value = top_value(sd.key_min, descending);
        totals->last_value = top_value(sd.key_max, descending);
    }
    totals->n_passes = plan.n_passes;
    totals->already_ordered = sd.unordered ? 0u : 1u;
    if (!out.any()) return GX_OK;   // size query
    if (out.per_line() && lines_out > out.cap_lines) return fail(GX_E_LIMIT, name + ": cap_lines is smaller than the result (see totals->lines_out)");
    if (out.lines.bytes && units * unit > out.bytes_cap) return fail(GX_E_LIMIT, name + ": the delivered text is larger than the capacity (see totals->units_out)");
    if (out.lines.offsets && !v.off64 && units > 0xFFFFFFFFull) return fail(GX_E_LIMIT, name + ": 4 G code units and more need offsets64");
    if (lines_out == 0) {
        fill_out(out.lines.offsets, 0, off_w, host_out, stream);
        return GX_OK;
    }
    StagedLinesOut so = stage_lines_out(h, v, out.lines, host_out, lines_out, units);
    int64_t* d_values = so.twins.of(out.values, lines_out * 8);
    uint8_t* d_cls = so.twins.of(out.cls, lines_out);
    PartWs pw{};   // (the copy pass reads the permutation and the output offsets alone)
    GX_HIP(launch_sort_emit(n, m, lines_out, plan, flags, w, d_values, d_cls, &pw.perm_sorted, stream));
    pw.dst_off = w.dst_off;
    GX_HIP(launch_partition_copy(so.dev, v.data, v.offsets, v.off64 ? 1 : 0, v.wide ? 1 : 0, n, lines_out, pw, stream));
    if (host_out) {
        so.deliver(stream);
        GX_HIP(hipStreamSynchronize(stream));
    } else {
        leave_pending(h->sort_event, h->sort_pending, stream);
    }
    return GX_OK;
}

int gx_sort_lines(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps, const gx_top_part* parts,
                  uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms, uint32_t flags, const gx_sort_out* out, gx_sort_totals* totals,
                  const gx_batch_opts* opts) {
    const std::string name = "gx_sort_lines";
    return guarded([&]() -> int {
        if (!h || !offsets || (n && !ids)) return fail(GX_E_ARG, name + ": bad argument");
        const gx_batch_opts o = read_opts(opts);
        uint32_t row_units = 1;
        const RowFormat fmt = id_format(h, o, &row_units);
        TopHead ti;
        WhereImage wi;
        sort_refusals(h, o, parts, n_parts, terms, n_terms, flags, o.utf16 != 0, totals, name, &ti, &wi);
        gx_sort_out so = out ? *out : gx_sort_out{};
        if (so.out_caps && fmt != ROWS_DENSE) return fail(GX_E_ARG, name + ": out_caps on compact rows (out_ids holds whole rows)");
        if ((n_parts || !wi.none()) && fmt == ROWS_DENSE && n && !caps) return fail(GX_E_ARG, name + ": parts and terms on dense ids need caps");
        if (n > SORT_MAX_LINES) return fail(GX_E_LIMIT, name + ": the sort's places are 30 bits; split batches of more than 2^30 lines");
        if (!o.device_pointers) refuse_long_host_lines({offsets, o.offsets64 != 0, n}, name, "sorted");
        const size_t slots = 2 * static_cast<size_t>(h->T.max_groups);
        if (so.out_caps && slots && n && !caps) return fail(GX_E_ARG, name + ": out_caps without caps");
        if (!slots) so.out_caps = nullptr;
        {
            const uint64_t ow = o.offsets64 ? 8 : 4, un = o.utf16 ? 2 : 1, idr = static_cast<uint64_t>(row_units) * row_unit_bytes(fmt);
            const uint64_t in_units = o.device_pointers ? (n ? 1u : 0u) : HostOffsets{offsets, o.offsets64 != 0, n}[n];
            const uint64_t cap = std::min<uint64_t>(so.cap_lines, n);   // (no more than n lines leave, whatever the capacity says: no product wraps)
            const std::pair<const void*, uint64_t> outs[7] = {{so.out_index, cap * 4}, {so.out_values, cap * 8}, {so.out_class, cap}, {so.out_bytes, so.out_bytes_cap},
                                                              {so.out_offsets, (cap + 1) * ow}, {so.out_ids, cap * idr}, {so.out_caps, cap * slots * 4}};
            const std::pair<const void*, uint64_t> ins[4] = {{bytes, in_units * un}, {offsets, (n + 1) * ow}, {ids, n * idr},
                                                             {fmt == ROWS_DENSE ? caps : nullptr, n * slots * 4}};
            by_key_overlaps(outs, 7, ins, 4, name);
        }
        if (!h->on_device) return fail(GX_E_DEVICE, "handle was created host-only; no device tables (there is no CPU fallback)");
        if (fmt != ROWS_DENSE) caps = nullptr;
        GX_HIP(hipSetDevice(h->device));
        std::lock_guard<std::mutex> lock(h->mu);
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        const StagedLines in = stage_lines(h, bytes, offsets, n, ids, caps, o, fmt, row_units, Travels{true, caps != nullptr}, stream, name.c_str());
        const SortOut to{{so.out_index, so.out_bytes, so.out_offsets, so.out_ids, so.out_caps}, so.out_values, so.out_class, so.cap_lines, so.out_bytes_cap};
        return sort_pass(h, in.v, ti, wi, flags, to, !o.device_pointers, totals, nullptr, stream, name);
    });
}

int gx_text_sort_lines(gx_handle* h, const uint8_t* text, uint64_t size, const gx_top_part* parts, uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms,
                       uint32_t flags, uint8_t* out, uint64_t out_cap, void* out_offsets, uint32_t* out_index, int64_t* out_values, uint8_t* out_class,
                       gx_sort_totals* totals, uint64_t* counts, uint64_t* n_lines, const gx_batch_opts* opts) {
    const std::string name = "gx_text_sort_lines";
    return guarded([&]() -> int {
        if (!h || (size && !text)) return fail(GX_E_ARG, name + ": bad argument");
        const gx_batch_opts o = read_opts(opts);
        TopHead ti;
        WhereImage wi;
        sort_refusals(h, o, parts, n_parts, terms, n_terms, flags, false, totals, name, &ti, &wi);
        const std::pair<const void*, uint64_t> outs[5] = {{out, out_cap}, {out_offsets, 4}, {out_index, 4}, {out_values, 8}, {out_class, 1}};
        const std::pair<const void*, uint64_t> ins[1] = {{text, size}};
        by_key_overlaps(outs, 5, ins, 1, name);
        if (size > 0xFFFFFFFFull) return fail(GX_E_LIMIT, name + ": split texts of 4 GiB and more at a line boundary");
        if (!h->on_device) return fail(GX_E_DEVICE, "handle was created host-only; no device tables (there is no CPU fallback)");
        GX_HIP(hipSetDevice(h->device));
        std::lock_guard<std::mutex> lock(h->mu);
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        // the text's lines and the path; then the passes over the ids, offsets and capture rows they left on the device
        const TextBatch tb = stage_text_lines(h, text, size, o, stream, name.c_str());
        if (n_lines) *n_lines = tb.v.n;
        if (tb.v.n > SORT_MAX_LINES) return fail(GX_E_LIMIT, name + ": the sort's places are 30 bits; split texts of more than 2^30 lines");
        // (cap_lines: sized by the size query -- the header)
        const SortOut to{{out_index, out, out_offsets, nullptr, nullptr}, out_values, out_class, ~0ull, out_cap};
        const int rc = sort_pass(h, tb.v, ti, wi, flags, to, !o.device_pointers, totals, counts, stream, name);
        // The passes behind the wait read the offsets that text_lines left in the handle's scratch buffers, which the next whole-file
        // call on any stream overwrites: like every gx_text_* call this one returns with its work done.
        if (h->sort_pending) {
            GX_HIP(hipStreamSynchronize(stream));
            h->sort_pending = false;
        }
        if (promise_broken_since(h, stream)) throw GxError(GX_E_ARG, "internal: " + name + ": a line longer than the split pass reported");
        return rc;
    });
}

// what both quantile calls refuse before they look at the device
static void quant_refusals(const gx_handle* h, const gx_batch_opts& o, const gx_top_part* parts, uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms,
                           const gx_quantile* quantiles, uint32_t n_quantiles, const gx_quantile_out* out, bool wide, const gx_quantile_totals* totals,
                           const std::string& name, TopHead* ti, QuantHead* qh, WhereImage* wi) {
    if (!totals) throw GxError(GX_E_ARG, name + ": totals is NULL");
    if (n_quantiles && (!quantiles || !out)) throw GxError(GX_E_ARG, name + ": quantiles or out is NULL");
    if (n_quantiles > GX_QUANTILE_MAX) throw GxError(GX_E_LIMIT, name + ": n_quantiles above GX_QUANTILE_MAX");
    *qh = QuantHead{};
    qh->n_q = n_quantiles;
    for (uint32_t q = 0; q < n_quantiles; ++q) {
        if (quantiles[q].den == 0) throw GxError(GX_E_ARG, name + ": a quantile's den is 0");
        if (quantiles[q].num > quantiles[q].den) throw GxError(GX_E_ARG, name + ": a quantile's num is above its den");
        qh->ask[q] = QuantAsk{quantiles[q].num, quantiles[q].den};
    }
    *ti = top_image(h, parts, n_parts, 0, name);
    if (o.utf8 == 2) throw GxError(GX_E_ARG, name + ": gx_batch_opts.utf8 = 1 (values are read in the units the offsets count)");
    *wi = where_image(h, terms, n_terms, wide, name);
    if (o.no_sync) throw GxError(GX_E_ARG, name + ": no_sync: the results are host values");
}

// The passes on the handle's workspace (under h->mu) and ONE synchronisation of the stream, where the host reads the counts and the
// result rows.  counts: also the histogram of outcomes (gx_text_capture_quantiles).
static_assert(sizeof(gx_quantile_out) == sizeof(QuantOut) && offsetof(gx_quantile_out, below) == offsetof(QuantOut, below), "the rows are copied as they are");
static int quant_pass(gx_handle* h, const BatchView& v, const TopHead& ti, const QuantHead& qh, const WhereImage& wi, gx_quantile_out* out,
                      gx_quantile_totals* totals, uint64_t* counts, hipStream_t stream) {
    const uint32_t K = static_cast<uint32_t>(h->T.n_rules);
    const size_t slots = 2 * static_cast<size_t>(h->T.max_groups);
    const uint64_t n = v.n;
    if (counts) counts_beside(h, v, counts, stream);
    *totals = gx_quantile_totals{};
    for (uint32_t q = 0; q < qh.n_q; ++q) out[q] = gx_quantile_out{};
    if (n == 0 || ti.n_parts == 0) {
        GX_HIP(hipStreamSynchronize(stream));
        return GX_OK;
    }
    // the image: the parts, the quantiles, the terms
    const DevImage img = upload_image(h->quant_image, &ti, sizeof(TopHead), &qh, wi, stream);
    const TopArgs a{v.data, v.wide ? 1 : 0, v.caps, static_cast<uint32_t>(slots), img.head, img.terms,
                    static_cast<uint32_t>(wi.bytes.size()), 0u, 0u, (ti.formats || wi.formats) ? 1u : 0u};
    const QuantWs w = quant_workspace(h->quant_ws.get(quant_workspace_bytes(n)), n);
    GX_HIP(launch_quantiles(v.ids, v.fmt, v.row_units, K, n, v.offsets, v.off64 ? 1 : 0, a, img.head + sizeof(TopHead), qh.n_q, w, stream));
    struct { uint32_t counts[TOP_COUNTS]; QuantOut out[QUANT_MAX]; } got{};
    static_assert(sizeof(got) == offsetof(QuantDev, sel), "the head's first words");
    GX_HIP(hipMemcpyAsync(&got, w.head, sizeof(got), hipMemcpyDeviceToHost, stream));
    GX_HIP(hipStreamSynchronize(stream));
    if (got.counts[TOP_C_STATUS]) throw GxError(GX_E_LIMIT, "a line of 4 G code units or more cannot be measured");
    totals->numbers = got.counts[TOP_C_NUMBERS];
    totals->unset = got.counts[TOP_C_UNSET];
    totals->not_numbers = got.counts[TOP_C_NOT_NUMBERS];
    totals->lines = totals->numbers + totals->unset + totals->not_numbers;
    for (uint32_t q = 0; q < qh.n_q; ++q) out[q] = gx_quantile_out{got.out[q].value, got.out[q].rank, got.out[q].below, got.out[q].equal};
    return GX_OK;
}

int gx_capture_quantiles(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps, const gx_top_part* parts,
                         uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms, const gx_quantile* quantiles, uint32_t n_quantiles, gx_quantile_out* out,
                         gx_quantile_totals* totals, const gx_batch_opts* opts) {
    const std::string name = "gx_capture_quantiles";
    return guarded([&]() -> int {
        if (!h || !offsets || (n && !ids)) return fail(GX_E_ARG, name + ": bad argument");
        const gx_batch_opts o = read_opts(opts);
        uint32_t row_units = 1;
        const RowFormat fmt = id_format(h, o, &row_units);
        TopHead ti;
        QuantHead qh;
        WhereImage wi;
        quant_refusals(h, o, parts, n_parts, terms, n_terms, quantiles, n_quantiles, out, o.utf16 != 0, totals, name, &ti, &qh, &wi);
        if ((n_parts || !wi.none()) && fmt == ROWS_DENSE && n && !caps) return fail(GX_E_ARG, name + ": parts and terms on dense ids need caps");
        if (n >= 0xFFFFFFFFull) return fail(GX_E_LIMIT, name + ": line numbers are 32 bits; split batches of 2^32 - 1 lines and more");
        if (!o.device_pointers) refuse_long_host_lines({offsets, o.offsets64 != 0, n}, name, "measured");
        if (!h->on_device) return fail(GX_E_DEVICE, "handle was created host-only; no device tables (there is no CPU fallback)");
        if (fmt != ROWS_DENSE) caps = nullptr;
        GX_HIP(hipSetDevice(h->device));
        std::lock_guard<std::mutex> lock(h->mu);
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        const StagedLines in = stage_lines(h, bytes, offsets, n, ids, caps, o, fmt, row_units, Travels{true, caps != nullptr}, stream, name.c_str());
        return quant_pass(h, in.v, ti, qh, wi, out, totals, nullptr, stream);
    });
}

int gx_text_capture_quantiles(gx_handle* h, const uint8_t* text, uint64_t size, const gx_top_part* parts, uint32_t n_parts, const gx_where_term* terms,
                              uint32_t n_terms, const gx_quantile* quantiles, uint32_t n_quantiles, gx_quantile_out* out, gx_quantile_totals* totals,
                              uint64_t* counts, uint64_t* n_lines, const gx_batch_opts* opts) {
    const std::string name = "gx_text_capture_quantiles";
    return guarded([&]() -> int {
        if (!h || (size && !text)) return fail(GX_E_ARG, name + ": bad argument");
        const gx_batch_opts o = read_opts(opts);
        TopHead ti;
        QuantHead qh;
        WhereImage wi;
        quant_refusals(h, o, parts, n_parts, terms, n_terms, quantiles, n_quantiles, out, false, totals, name, &ti, &qh, &wi);
        if (size > 0xFFFFFFFFull) return fail(GX_E_LIMIT, name + ": split texts of 4 GiB and more at a line boundary");
        if (!h->on_device) return fail(GX_E_DEVICE, "handle was created host-only; no device tables (there is no CPU fallback)");
        GX_HIP(hipSetDevice(h->device));
        std::lock_guard<std::mutex> lock(h->mu);
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        // the text's lines and the path; then the passes over the ids, offsets and capture rows they left on the device
        const TextBatch tb = stage_text_lines(h, text, size, o, stream, name.c_str());
        if (n_lines) *n_lines = tb.v.n;
        const int rc = quant_pass(h, tb.v, ti, qh, wi, out, totals, counts, stream);
        if (promise_broken_since(h, stream)) throw GxError(GX_E_ARG, "internal: " + name + ": a line longer than the split pass reported");
        return rc;
    });
}

// Keys, sort, scan and the groups on the handle's workspace (under h->mu); then the host reads what it must know before anything is
// written -- the groups' boundaries, whose last entries are the number of kept lines and of kept code units, and whether a line was
// too long to count: ONE small synchronisation of the stream (before it the want mask goes to the device, as select_pass sends it).
// want: host, uint8_t[2K + 1], or nullptr = every outcome 0 .. 2K.  front: bytes at the head of the
// workspace that the caller keeps for itself.
struct Partitioned {
    PartWs w;
    std::vector<uint64_t> groups;   // [2K + 3] lines, then [2K + 3] code units
    uint64_t lines = 0, units = 0;
};
static Partitioned partition_pass(gx_handle* h, const BatchView& v, const uint8_t* want, size_t front, hipStream_t stream) {
    const uint32_t K = static_cast<uint32_t>(h->T.n_rules), bins = 2u * K + 2u;
    wait_pending(h->select_event, h->select_pending, stream);
    Partitioned s;
    uint8_t* ws = static_cast<uint8_t*>(h->select_ws.get(front + partition_workspace_bytes(v.n, K)));
    s.w = partition_workspace(ws + front, v.n, K);
    if (want) GX_HIP(hipMemcpyAsync(s.w.want, want, bins - 1u, hipMemcpyHostToDevice, stream));
    else GX_HIP(hipMemsetAsync(s.w.want, 1, bins - 1u, stream));
    GX_HIP(launch_partition_sort(v.ids, v.fmt, v.row_units, K, v.n, v.offsets, v.off64 ? 1 : 0, s.w, stream));
    s.groups.assign(2 * static_cast<size_t>(bins + 1), 0);
    uint32_t status = 0;
    GX_HIP(hipMemcpyAsync(s.groups.data(), s.w.groups, s.groups.size() * 8, hipMemcpyDeviceToHost, stream));
    GX_HIP(hipMemcpyAsync(&status, s.w.status, 4, hipMemcpyDeviceToHost, stream));
    GX_HIP(hipStreamSynchronize(stream));
    if (status) throw GxError(GX_E_LIMIT, "a line of 4 G code units or more cannot be partitioned");
    s.lines = s.groups[bins];
    s.units = s.groups[2 * static_cast<size_t>(bins) + 1];
    return s;
}

int gx_partition_lines(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps, const uint8_t* want,
                       uint32_t* out_index, void* out_bytes, void* out_offsets, void* out_ids, int32_t* out_caps, uint64_t cap_lines,
                       uint64_t out_bytes_cap, uint64_t* group_lines, uint64_t* group_units, uint64_t* n_out, uint64_t* bytes_out,
                       const gx_batch_opts* opts) {
    return guarded([&]() -> int {
        if (!h || !offsets || !n_out || !bytes_out || (n && !ids)) return fail(GX_E_ARG, "gx_partition_lines: bad argument");
        if (!h->on_device) return fail(GX_E_DEVICE, "handle was created host-only; no device tables (there is no CPU fallback)");
        if (n >= (1ull << 32)) return fail(GX_E_LIMIT, "gx_partition_lines: line numbers are 32 bits; split batches of 4 G lines and more");
        const gx_batch_opts o = read_opts(opts);
        uint32_t row_units = 1;
        const RowFormat fmt = id_format(h, o, &row_units);
        const size_t slots = 2 * static_cast<size_t>(h->T.max_groups);
        if (fmt != ROWS_DENSE) { caps = nullptr; out_caps = nullptr; }
        if (out_caps && slots && n && !caps) return fail(GX_E_ARG, "gx_partition_lines: out_caps without caps");
        if (!slots) out_caps = nullptr;
        if (o.no_sync && !o.device_pointers) return fail(GX_E_ARG, "gx_partition_lines: no_sync needs device pointers");
        GX_HIP(hipSetDevice(h->device));
        std::lock_guard<std::mutex> lock(h->mu);
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        const size_t unit = o.utf16 ? 2 : 1;
        const size_t bins = 2 * static_cast<size_t>(h->T.n_rules) + 2;
        const bool host = !o.device_pointers;
        // (the sizes and the groups depend on the ids and the offsets alone: the text and the capture rows travel only if they are asked for)
        const StagedLines in = stage_lines(h, bytes, offsets, n, ids, caps, o, fmt, row_units, Travels{out_bytes != nullptr, out_caps != nullptr}, stream,
                                           "gx_partition_lines");
        const BatchView& v = in.v;
        const Partitioned s = partition_pass(h, v, want, 0, stream);
        *n_out = s.lines;
        *bytes_out = s.units * unit;
        if (group_lines) std::copy(s.groups.begin(), s.groups.begin() + bins + 1, group_lines);
        if (group_units) std::copy(s.groups.begin() + bins + 1, s.groups.end(), group_units);
        const LinesOut lo{out_index, out_bytes, out_offsets, out_ids, out_caps};
        if (!lo.any()) return GX_OK;   // size query
        if (lo.per_line() && s.lines > cap_lines) return fail(GX_E_LIMIT, "gx_partition_lines: cap_lines is smaller than the partition (see *n_out)");
        if (out_bytes && s.units * unit > out_bytes_cap)
            return fail(GX_E_LIMIT, "gx_partition_lines: out_bytes_cap is smaller than the kept text (see *bytes_out)");
        const StagedLinesOut out = stage_lines_out(h, v, lo, host, s.lines, s.units);
        if (out.dev.offsets && s.lines == 0) GX_HIP(hipMemsetAsync(out.dev.offsets, 0, v.off64 ? 8 : 4, stream));
        GX_HIP(launch_partition_copy(out.dev, v.data, v.offsets, v.off64 ? 1 : 0, v.wide ? 1 : 0, n, s.lines, s.w, stream));
        if (host) out.deliver(stream);
        // (no_sync: the copy pass still reads the workspace: whoever uses it next waits for this)
        if (o.no_sync) leave_pending(h->select_event, h->select_pending, stream);
        else GX_HIP(hipStreamSynchronize(stream));
        return GX_OK;
    });
}

int gx_text_to_jsonl_by_extraction(gx_handle* h, const uint8_t* text, uint64_t size, const char* id_as, uint8_t* out, uint64_t out_cap,
                                   uint64_t* out_size, uint64_t* group_out, uint64_t* counts, uint64_t* n_lines, const gx_batch_opts* opts) {
    return guarded([&]() -> int {
        if (!h || !out_size || (size && !text)) return fail(GX_E_ARG, "gx_text_to_jsonl_by_extraction: bad argument");
        if (!h->on_device) return fail(GX_E_DEVICE, "handle was created host-only; no device tables (there is no CPU fallback)");
        if (size > 0xFFFFFFFFull) return fail(GX_E_LIMIT, "gx_text_to_jsonl_by_extraction: split texts of 4 GiB and more at a line boundary");
        const gx_batch_opts o = read_opts(opts);
        if (o.utf8 == 2) return fail(GX_E_ARG, "gx_text_to_jsonl_by_extraction: gx_batch_opts.utf8 = 1 (the text is written from its bytes)");
        const size_t slots = 2 * static_cast<size_t>(h->T.max_groups);
        if (slots > 128) return fail(GX_E_LIMIT, "gx_text_to_jsonl_by_extraction: more than 64 capture groups per extraction");
        GX_HIP(hipSetDevice(h->device));
        std::lock_guard<std::mutex> lock(h->mu);
        const GxJsonl& tm = jsonl_templates(h, id_as);
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        DevMem<uint8_t> d_out;
        const uint32_t K = static_cast<uint32_t>(h->T.n_rules), bins = 2u * K + 2u;
        const int passthrough = (o.utf8_passthrough || o.utf8) ? 1 : 0;   // (utf8 implies it)
        // 1. lines, 2. the path (no escape bits: they would belong to the original text, and the JSON passes read the partitioned one)
        const TextBatch tb = stage_text_lines(h, text, size, o, stream, "gx_text_to_jsonl_by_extraction");
        const BatchView& v = tb.v;
        const uint64_t n = v.n;
        // 3. the histogram (the head of the workspace) and the partition of the matched lines, outcomes 0 .. K - 1
        const size_t front = counts ? select_workspace_bytes(n, K, false) : 0;
        std::vector<uint8_t> want(bins - 1u, 0);
        std::fill(want.begin(), want.begin() + K, 1);
        wait_pending(h->select_event, h->select_pending, stream);
        (void)h->select_ws.get(front + partition_workspace_bytes(n, K));   // (grown once: the histogram's part stays where it is)
        if (counts) counts_beside(h, v, counts, stream);
        const Partitioned s = partition_pass(h, v, want.data(), front, stream);
        // (the extraction ran on the split pass's own longest line; a kernel that met a longer one after all left rows unwritten)
        if (promise_broken_since(h, stream)) throw GxError(GX_E_ARG, "internal: gx_text_to_jsonl_by_extraction: a line longer than the split pass reported");
        const uint64_t m = s.lines;
        GxBatch b{};
        b.data = h->scratch[8].get(s.units + 16);
        b.offsets = h->scratch[9].get((m + 1) * 4);
        b.n = m;
        b.match_id = static_cast<int32_t*>(h->scratch[10].get(m * 4 + 16));
        b.caps = static_cast<int32_t*>(h->scratch[11].get(m * slots * 4 + 16));
        b.strip_eol = 1;
        SelectOut part{};
        part.bytes = const_cast<void*>(b.data); part.offsets = const_cast<void*>(b.offsets);
        part.col_src[0] = v.ids; part.col_dst[0] = b.match_id; part.col_width[0] = 1; part.col_unit_bytes[0] = 4;
        if (slots) { part.col_src[1] = v.caps; part.col_dst[1] = b.caps; part.col_width[1] = static_cast<uint32_t>(slots); part.col_unit_bytes[1] = 4; }
        if (m == 0) GX_HIP(hipMemsetAsync(part.offsets, 0, 4, stream));
        GX_HIP(launch_partition_copy(part, v.data, v.offsets, 0, 0, n, m, s.w, stream));
        // 4. the text, from the partitioned batch
        void* ws_json = h->scratch[0].get(jsonl_workspace_bytes(m));
        uint64_t* loff = static_cast<uint64_t*>(h->scratch[1].get((m + 1) * 8 + (static_cast<size_t>(K) + 1) * 8));
        uint64_t* d_group_out = loff + m + 1;
        const uint32_t mean_in = m ? static_cast<uint32_t>(std::min<uint64_t>((s.units + m - 1) / m, 1u << 20)) : 1u;
        GX_HIP(launch_jsonl_sizes(tm, b, static_cast<int>(slots), passthrough, mean_in, loff, ws_json, stream));
        uint64_t total = 0;
        GX_HIP(hipMemcpyAsync(&total, loff + m, 8, hipMemcpyDeviceToHost, stream));
        if (group_out) {
            // (group k's objects begin where its first line's object does; the groups' boundaries are still in the workspace)
            GX_HIP(launch_partition_pick(loff, s.w.groups, K + 1u, d_group_out, stream));
            GX_HIP(hipMemcpyAsync(group_out, d_group_out, (static_cast<size_t>(K) + 1) * 8, hipMemcpyDeviceToHost, stream));
        }
        GX_HIP(hipStreamSynchronize(stream));
        *out_size = total;
        if (n_lines) *n_lines = n;
        if (!out) return GX_OK;
        if (total > out_cap) return fail(GX_E_LIMIT, "gx_text_to_jsonl_by_extraction: out_cap is smaller than the text (see *out_size)");
        uint8_t* dst = out;
        if (!o.device_pointers) { d_out = dev_alloc<uint8_t>(total); dst = d_out.get(); }
        const uint32_t mean_out = m ? static_cast<uint32_t>(std::min<uint64_t>((total + m - 1) / m, 1u << 20)) : 1u;
        GX_HIP(launch_jsonl_write(tm, b, static_cast<int>(slots), passthrough, mean_in, mean_out, loff, dst, ws_json, stream));
        if (!o.device_pointers && total) GX_HIP(hipMemcpyAsync(out, dst, total, hipMemcpyDeviceToHost, stream));
        GX_HIP(hipStreamSynchronize(stream));
        return GX_OK;
    });
}

int gx_pack_results(const int32_t* match_id, const int32_t* caps, uint64_t n, int32_t slots, uint16_t* packed, uint64_t* n_overflow,
                    const gx_batch_opts* opts) {
    return guarded([&]() -> int {
        if (slots < 0 || !n_overflow || (n && (!match_id || !packed || (slots && !caps)))) return fail(GX_E_ARG, "gx_pack_results: bad argument");
        const gx_batch_opts o = read_opts(opts);
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        const DevMem<unsigned long long> cnt = dev_alloc<unsigned long long>(8);
        GX_HIP(launch_pack_results(match_id, caps, n, slots, packed, cnt.get(), stream));
        unsigned long long over = 0;
        GX_HIP(hipMemcpyAsync(&over, cnt.get(), 8, hipMemcpyDeviceToHost, stream));
        GX_HIP(hipStreamSynchronize(stream));
        *n_overflow = over;
        return GX_OK;
    });
}

int gx_unpack_results(const uint16_t* packed, uint64_t n, int32_t slots, int32_t* match_id, int32_t* caps, const gx_batch_opts* opts) {
    return guarded([&]() -> int {
        if (slots < 0 || (n && (!match_id || !packed || (slots && !caps)))) return fail(GX_E_ARG, "gx_unpack_results: bad argument");
        const gx_batch_opts o = read_opts(opts);
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        GX_HIP(launch_unpack_results(packed, n, slots, match_id, caps, stream));
        if (!o.no_sync) GX_HIP(hipStreamSynchronize(stream));
        return GX_OK;
    });
}

int gx_unpack_results8(const uint8_t* rows, uint64_t n, int32_t slots, int32_t* match_id, int32_t* caps, const gx_batch_opts* opts) {
    return guarded([&]() -> int {
        if (slots < 0 || (n && (!match_id || !rows || (slots && !caps)))) return fail(GX_E_ARG, "gx_unpack_results8: bad argument");
        const gx_batch_opts o = read_opts(opts);
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        GX_HIP(launch_unpack_results8(rows, n, slots, match_id, caps, stream));
        if (!o.no_sync) GX_HIP(hipStreamSynchronize(stream));
        return GX_OK;
    });
}

int gx_set_extraction_meta(gx_handle* h, int32_t k, const char* name, const char* const* extractor_names, int32_t n_names,
                           const char* append_json) {
    if (!h || !name || k < 0 || k >= h->T.n_rules || n_names < 0 || (n_names && !extractor_names))
        return fail(GX_E_ARG, "gx_set_extraction_meta: bad argument");
    if (n_names != h->T.rules[k].n_groups) return fail(GX_E_ARG, "gx_set_extraction_meta: n_names must equal gx_num_groups(h, k)");
    return guarded([&]() -> int {
        std::lock_guard<std::mutex> lock(h->mu);
        if (static_cast<int>(h->meta.size()) != h->T.n_rules) h->meta.assign(h->T.n_rules, dsl::Extraction());
        dsl::Extraction& x = h->meta[k];
        x.name = name;
        x.extractor_names.assign(extractor_names, extractor_names + n_names);
        x.append_json = append_json ? dsl::canonical_json_object(append_json) : std::string();
        h->jsonl.clear();
        h->append_entries.clear();
        return GX_OK;
    });
}

int gx_set_number_format(gx_handle* h, int32_t k, int32_t g, const gx_number_format* f) {
    if (!h || k < 0 || k >= h->T.n_rules || g < 0 || g >= h->T.rules[k].n_groups) return fail(GX_E_ARG, "gx_set_number_format: bad argument");
    if (f && !number_format_ok(f->kind, f->scale)) return fail(GX_E_ARG, "gx_set_number_format: an unknown kind, or a scale the kind does not take");
    return guarded([&]() -> int {
        std::lock_guard<std::mutex> lock(h->mu);
        if (static_cast<int>(h->number_formats.size()) != h->T.n_rules) h->number_formats.resize(h->T.n_rules);
        std::vector<uint8_t>& row = h->number_formats[k];
        if (static_cast<int>(row.size()) != h->T.rules[k].n_groups) row.assign(h->T.rules[k].n_groups, 0);
        row[g] = f ? number_pack(f->kind, f->scale) : 0;
        return GX_OK;
    });
}

int gx_get_number_format(const gx_handle* h, int32_t k, int32_t g, gx_number_format* out) {
    if (!h || !out || k < 0 || k >= h->T.n_rules || g < 0 || g >= h->T.rules[k].n_groups) return fail(GX_E_ARG, "gx_get_number_format: bad argument");
    const uint8_t packed = h->number_format_of(k, g);
    out->kind = number_kind(packed);
    out->scale = number_scale(packed);
    return GX_OK;
}

int gx_parse_number(const gx_number_format* f, const void* units, uint32_t n_units, uint32_t utf16, int64_t* value, int32_t* is_number) {
    if (!value || !is_number || (n_units && !units)) return fail(GX_E_ARG, "gx_parse_number: bad argument");
    const uint32_t kind = f ? f->kind : static_cast<uint32_t>(NUMBER_LONG), scale = f ? f->scale : 0u;
    if (!number_format_ok(kind, scale)) return fail(GX_E_ARG, "gx_parse_number: an unknown kind, or a scale the kind does not take");
    int64_t v = 0;
    const bool ok = utf16 ? number_parse(kind, scale, static_cast<const uint16_t*>(units), n_units, &v)
                          : number_parse(kind, scale, static_cast<const uint8_t*>(units), n_units, &v);
    *is_number = ok ? 1 : 0;
    if (ok) *value = v;
    return GX_OK;
}

// One host-pointer batch through the workers of gx_handle::host_slot.  `proto` carries the batch's modes (wide,
// offsets64, match_only, strip_eol); lines [0, n) are cut into chunks of whole lines of about chunk_bytes, chunk c goes
// to worker c % HOST_WORKERS.  A chunk's lines keep their offsets: the kernels get a data pointer moved back by the
// chunk's first offset instead of rebased offsets.
static void host_pipeline(gx_handle* h, const GxBatch& proto, const uint8_t* bytes, const HostOffsets& off, uint64_t total,
                          int32_t* match_id, int32_t* caps, int32_t* states, bool compact, bool match_only, uint32_t hint, uint32_t kernel,
                          bool uneven, uint64_t* over_total) {
    const uint64_t n = off.n;
    if (n == 0) return;
    const size_t unit = proto.wide ? 2 : 1, off_w = proto.offsets64 ? 8 : 4;
    const size_t slots = 2 * static_cast<size_t>(h->T.max_groups);
    // chunks: large enough to amortise a launch, small enough that the pipeline has several in flight
    const uint64_t total_bytes = total * unit;
    uint64_t chunk_bytes = std::max<uint64_t>(total_bytes / (4 * gx_handle::HOST_WORKERS), 8ull << 20);
    chunk_bytes = std::min<uint64_t>(chunk_bytes, 128ull << 20);
    std::vector<uint64_t> cuts(1, 0);
    while (cuts.back() < n) {
        const uint64_t a = cuts.back();
        uint64_t b_ = off.lines_at_or_after(off[a] + (chunk_bytes + unit - 1) / unit, a + 1);   // (at least one line per chunk)
        if (b_ - a > 0x7FFFFFF0ull) b_ = a + 0x7FFFFFF0ull;
        cuts.push_back(std::min<uint64_t>(b_, n));
    }
    const size_t n_chunks = cuts.size() - 1;
    const int workers = static_cast<int>(std::min<size_t>(gx_handle::HOST_WORKERS, n_chunks));
    std::atomic<uint64_t> over_sum{0};
    std::mutex err_mu;
    int err_code = GX_OK;
    std::string err_msg;
    auto work = [&](int w) {
        const int rc = guarded([&]() -> int {
            GX_HIP(hipSetDevice(h->device));
            gx_handle::HostSlot& sl = h->host_slot[w];
            if (!sl.stream) GX_HIP(hipStreamCreateWithFlags(sl.stream.out(), hipStreamNonBlocking));
            hipStream_t stream = sl.stream.get();
            if (compact && !sl.over) GX_HIP(hipMalloc(sl.over.out(), 8));
            for (size_t c = static_cast<size_t>(w); c < n_chunks; c += static_cast<size_t>(workers)) {
                const uint64_t a = cuts[c], e = cuts[c + 1], m = e - a;
                const uint64_t b0 = off[a] * unit, nbytes = off[e] * unit - b0;
                uint8_t* place = static_cast<uint8_t*>(sl.bytes.get(nbytes + 64)) + 16;  // (a 16-byte aligned first line, room for the aligned span before it)
                void* d_off = sl.off.get((m + 1) * off_w);
                GxBatch b = proto;
                b.n = m;
                b.data = place - b0;
                b.offsets = d_off;
                if (nbytes) GX_HIP(hipMemcpyAsync(place, bytes + b0, nbytes, hipMemcpyHostToDevice, stream));
                GX_HIP(hipMemcpyAsync(d_off, static_cast<const uint8_t*>(off.p) + a * off_w, (m + 1) * off_w, hipMemcpyHostToDevice, stream));
                if (states) b.state_out = static_cast<int32_t*>(sl.states.get(m * 4));
                const size_t rb = row_bytes(row_format(true, proto.narrow != 0), static_cast<uint32_t>(slots));
                if (compact) {
                    b.packed = static_cast<uint16_t*>(sl.res.get(m * rb));
                    GX_HIP(hipMemsetAsync(sl.over.get(), 0, 8, stream));
                    b.overflow = sl.over.get();
                } else {
                    b.match_id = static_cast<int32_t*>(sl.res.get(m * 4));
                    if (!match_only) b.caps = static_cast<int32_t*>(sl.caps.get(m * slots * 4 + 16));
                }
                launch_batch(h, b, hint, kernel, stream, uneven);
                unsigned long long over = 0;
                if (compact) {
                    GX_HIP(hipMemcpyAsync(reinterpret_cast<uint8_t*>(caps) + a * rb, b.packed, m * rb, hipMemcpyDeviceToHost, stream));
                    GX_HIP(hipMemcpyAsync(&over, sl.over.get(), 8, hipMemcpyDeviceToHost, stream));
                } else {
                    GX_HIP(hipMemcpyAsync(match_id + a, b.match_id, m * 4, hipMemcpyDeviceToHost, stream));
                    if (!match_only && slots) GX_HIP(hipMemcpyAsync(caps + a * slots, b.caps, m * slots * 4, hipMemcpyDeviceToHost, stream));
                }
                if (states) GX_HIP(hipMemcpyAsync(states + a, b.state_out, m * 4, hipMemcpyDeviceToHost, stream));
                GX_HIP(hipStreamSynchronize(stream));  // this worker's buffers are free again; the other workers keep the bus busy
                over_sum += over;
            }
            return GX_OK;
        });
        if (rc == GX_OK) return;
        std::lock_guard<std::mutex> g(err_mu);
        if (err_code == GX_OK) { err_code = rc; err_msg = g_last_error; }
    };
    if (workers == 1) work(0);
    else {
        std::vector<std::thread> pool;
        for (int w = 0; w < workers; ++w) pool.emplace_back(work, w);
        for (auto& t : pool) t.join();
    }
    if (err_code != GX_OK) throw GxError(err_code, err_msg);
    *over_total = over_sum.load();
}

// Do the lines of a batch differ much in length?  Lines run in lock step in groups of 64, a group takes as long as its longest
// line: over a sample of up to 64 groups spread over the batch, (sum of 64 x longest line) / (sum of lengths) > 1.25.
static bool lines_are_uneven(const HostOffsets& off) {
    if (off.n < 128) return false;
    const uint64_t groups = off.n / 64, sample = std::min<uint64_t>(groups, 64), stride = groups / sample;
    uint64_t lock_step = 0, bytes = 0;
    for (uint64_t g = 0; g < sample; ++g) {
        const uint64_t i0 = g * stride * 64;
        uint64_t longest = 0;
        for (uint64_t i = i0; i < i0 + 64; ++i) longest = std::max(longest, off[i + 1] - off[i]);
        lock_step += 64 * longest;
        bytes += off[i0 + 64] - off[i0];
    }
    return bytes > 0 && lock_step * 4 > bytes * 5;
}

// gx_extract_batch, and gx_match_batch when `states` is given (final product-DFA state per line, -1 = dead: the
// per-line generic kernel then, which is the one that keeps it)
static int extract_batch_impl(gx_handle* h, const uint8_t* bytes, const void* offsets, uint64_t n, int32_t* match_id, int32_t* caps,
                              int32_t* states, const gx_batch_opts* opts, DeviceBatch* keep = nullptr) {
    return guarded([&]() -> int {
        if (!h || !offsets) return fail(GX_E_ARG, "gx_extract_batch: bad argument");
        const gx_batch_opts o = read_opts(opts);
        if (o.utf8) {
            if (o.utf16) return fail(GX_E_ARG, "gx_batch_opts.utf8 with utf16: the batch is either UTF-8 bytes or UTF-16 code units");
            if (states) return fail(GX_E_ARG, "gx_batch_opts.utf8: gx_match_batch reads bytes as Latin-1 (the final states of UTF-8 lines: gx_utf8_to_utf16, then utf16)");
            if (o.no_sync)
                return fail(GX_E_ARG, "gx_batch_opts.utf8 with no_sync: the memory for the code units of the lines that hold a byte >= 0x80 is sized by a read "
                                      "on the host; call it without no_sync");
        }
        if (!h->on_device) return fail(GX_E_DEVICE, "handle was created host-only; no device tables (there is no CPU fallback)");
        if (o.kernel > GX_KERNEL_HOP_SLICES) return fail(GX_E_ARG, "gx_batch_opts.kernel: unknown kernel");
        const bool match_only = o.match_only || states || !h->T.has_capture;
        const bool compact = o.compact_results && !match_only;  // rows of u16[1 + slots] (2: u8[1 + slots]) through `caps`
        if (o.compact_results > 2) return fail(GX_E_ARG, "gx_batch_opts.compact_results: 0, 1 (u16 rows) or 2 (u8 rows)");
        if (compact && o.compact_results == 2 && h->T.n_rules > 126)
            return fail(GX_E_ARG, "gx_batch_opts.compact_results = 2: u8 rows hold match ids -128 .. 127 (at most 126 extractions)");
        if (!compact && !match_id) return fail(GX_E_ARG, "gx_extract_batch: match_id is NULL");
        if (!match_only && !caps && n > 0 && (compact || h->T.max_groups > 0)) return fail(GX_E_ARG, "gx_extract_batch: caps is NULL");
        GX_HIP(hipSetDevice(h->device));
        hipStream_t stream = static_cast<hipStream_t>(o.stream);
        GxBatch b{};
        b.n = n;
        b.wide = o.utf16 ? 1 : 0;
        b.offsets64 = o.offsets64 ? 1 : 0;
        b.match_only = match_only ? 1 : 0;
        b.strip_eol = o.strip_eol ? 1 : 0;
        b.narrow = (compact && o.compact_results == 2) ? 1 : 0;
        if (o.device_pointers) {
            b.data = bytes; b.offsets = offsets;
            b.state_out = states;
            if (compact) {
                b.packed = reinterpret_cast<uint16_t*>(caps);
                b.overflow = static_cast<unsigned long long*>(o.overflow);
            } else {
                b.match_id = match_id;
                b.caps = match_only ? nullptr : caps;
            }
            uint32_t hint = o.line_bytes_hint;
            bool uneven = o.uneven_lines == 2;
            if (hint == 0 && n && o.no_sync) {
                hint = h->hint.next(offsets, n, o.offsets64 != 0, stream);
            } else if (hint == 0 && n) {
                // no hint: the mean line length, from the two ends of the offsets array (a small synchronous read;
                // asynchronous callers pass line_bytes_hint themselves)
                const auto [first, last] = device_offset_ends(offsets, n, o.offsets64 != 0, stream);
                hint = static_cast<uint32_t>(std::min<uint64_t>((last - first + n - 1) / n, 4096));
                if (hint == 0) hint = 1;
                if (o.uneven_lines == 0 && n >= 128) {
                    // ... and whether the lines differ much in length: the first 4096 of them
                    const uint64_t m = std::min<uint64_t>(n, 4096);
                    const size_t off_w = o.offsets64 ? 8 : 4;
                    std::vector<uint8_t> sample((m + 1) * off_w);
                    GX_HIP(hipMemcpyAsync(sample.data(), offsets, sample.size(), hipMemcpyDeviceToHost, stream));
                    GX_HIP(hipStreamSynchronize(stream));
                    uneven = lines_are_uneven(HostOffsets{sample.data(), o.offsets64 != 0, m});
                }
            }
            b.max_line_bytes = o.max_line_bytes;
            b.caller_no_sync = o.no_sync ? 1u : 0u;
            DeviceBatch d;
            d.stream = stream;
            launch_batch(h, b, hint, o.kernel, stream, uneven, &d.done);
            d.b = b;
            d.enqueued = true;
            if (keep) *keep = d;   // (gx_extract_batch_multi_device waits for its shards itself)
            if (!o.no_sync) finish_device_batch(h, d);
            if (o.utf8) {
                // the lines that are not ASCII again, as Strings (behind finish_device_batch: a line it takes again is taken on bytes)
                utf8_fixup(h, b, o.utf8, static_cast<const uint8_t*>(o.utf8_line_flags), stream);
                GX_HIP(hipStreamSynchronize(stream));
            }
            return GX_OK;
        }
        if (o.utf8) {
            // host pointers: the whole batch is staged to the device and back (as gx_select_lines does), not cut into chunks
            const HostOffsets off{offsets, o.offsets64 != 0, n};
            const uint64_t first = n ? off[0] : 0, total = n ? off[n] - first : 0;
            if (total && !bytes) return fail(GX_E_ARG, "gx_extract_batch: bytes is NULL");
            const size_t off_w = o.offsets64 ? 8 : 4, slots = 2 * static_cast<size_t>(h->T.max_groups);
            const size_t rb = row_bytes(row_format(true, o.compact_results == 2), static_cast<uint32_t>(slots));
            const size_t res_bytes = compact ? n * rb : n * 4, caps_bytes = (compact || match_only) ? 0 : n * slots * 4;
            DevMem<uint8_t> d_bytes = dev_alloc<uint8_t>(total + 32), d_flags;
            DevMem<> d_off = dev_alloc((n + 1) * off_w), d_res = dev_alloc(res_bytes), d_caps = dev_alloc(caps_bytes);
            DevMem<unsigned long long> d_over = dev_alloc<unsigned long long>(8);
            uint8_t* place = d_bytes.get() + 16;
            // (line i at base + offsets[i], as in the caller's buffer; the base may lie below the allocation: made as an integer)
            const uint8_t* base = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(place) - static_cast<uintptr_t>(first));
            if (total) GX_HIP(hipMemcpyAsync(place, bytes + first, total, hipMemcpyHostToDevice, stream));
            GX_HIP(hipMemcpyAsync(d_off.get(), offsets, (n + 1) * off_w, hipMemcpyHostToDevice, stream));
            GX_HIP(hipMemsetAsync(d_over.get(), 0, 8, stream));
            if (o.utf8_line_flags && n) {
                d_flags = dev_alloc<uint8_t>(n);
                GX_HIP(hipMemcpyAsync(d_flags.get(), o.utf8_line_flags, n, hipMemcpyHostToDevice, stream));
            }
            gx_batch_opts od = o;
            od.struct_size = sizeof(gx_batch_opts);
            od.device_pointers = 1;
            od.overflow = compact ? d_over.get() : nullptr;
            od.utf8_line_flags = o.utf8_line_flags && n ? d_flags.get() : nullptr;
            int32_t* d_mid = compact ? nullptr : static_cast<int32_t*>(d_res.get());
            int32_t* d_rows = compact ? static_cast<int32_t*>(d_res.get()) : static_cast<int32_t*>(d_caps.get());
            const int rc = extract_batch_impl(h, base, d_off.get(), n, d_mid, d_rows, nullptr, &od);
            if (rc != GX_OK) return rc;
            unsigned long long over = 0;
            if (compact) {
                if (res_bytes) GX_HIP(hipMemcpyAsync(caps, d_res.get(), res_bytes, hipMemcpyDeviceToHost, stream));
                GX_HIP(hipMemcpyAsync(&over, d_over.get(), 8, hipMemcpyDeviceToHost, stream));
            } else {
                if (n) GX_HIP(hipMemcpyAsync(match_id, d_res.get(), n * 4, hipMemcpyDeviceToHost, stream));
                if (caps_bytes) GX_HIP(hipMemcpyAsync(caps, d_caps.get(), caps_bytes, hipMemcpyDeviceToHost, stream));
            }
            GX_HIP(hipStreamSynchronize(stream));
            if (compact && o.overflow) *static_cast<uint64_t*>(o.overflow) += over;
            return GX_OK;
        }
        // host pointers: the chunked pipeline (gx_handle::host_slot)
        std::lock_guard<std::mutex> lock(h->mu);
        const HostOffsets off{offsets, o.offsets64 != 0, n};
        const uint64_t total = n ? off[n] - off[0] : 0;  // code units in the batch (offsets need not start at 0: a shard of a larger CSR buffer)
        uint32_t hint = o.line_bytes_hint;
        if (hint == 0 && n) hint = static_cast<uint32_t>(std::min<uint64_t>((total + n - 1) / n, 1u << 20));
        uint64_t over_total = 0;
        const bool uneven = o.uneven_lines == 2 || (o.uneven_lines == 0 && lines_are_uneven(off));
        host_pipeline(h, b, bytes, off, total, match_id, caps, states, compact, match_only, hint, o.kernel, uneven, &over_total);
        if (compact && o.overflow) *static_cast<uint64_t*>(o.overflow) += over_total;
        return GX_OK;
    });
}

int gx_extract_batch(gx_handle* h, const uint8_t* bytes, const void* offsets, uint64_t n, int32_t* match_id, int32_t* caps,
                     const gx_batch_opts* opts) {
    return extract_batch_impl(h, bytes, offsets, n, match_id, caps, nullptr, opts);
}

int gx_match_batch(gx_handle* h, const uint8_t* bytes, const void* offsets, uint64_t n, int32_t* first_match, int32_t* states,
                   const gx_batch_opts* opts) {
    if (!states) return fail(GX_E_ARG, "gx_match_batch: states is NULL (gx_extract_batch with match_only gives the first match alone)");
    return extract_batch_impl(h, bytes, offsets, n, first_match, nullptr, states, opts);
}

int gx_set_device(int device) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return fail(GX_E_DEVICE, "gx_set_device: no such device");
    if (hipSetDevice(device) != hipSuccess) return fail(GX_E_DEVICE, "gx_set_device: hipSetDevice failed");
    return GX_OK;
}

int gx_handle_device(const gx_handle* h) { return h && h->on_device ? h->device : -1; }

int gx_host_register(void* p, size_t bytes) {
    if (!p || !bytes) return fail(GX_E_ARG, "gx_host_register: bad argument");
    const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
    if (e != hipSuccess) return fail(GX_E_DEVICE, std::string("hipHostRegister: ") + hipGetErrorString(e));
    return GX_OK;
}
int gx_host_unregister(void* p) {
    if (!p) return fail(GX_E_ARG, "gx_host_unregister: bad argument");
    const hipError_t e = hipHostUnregister(p);
    if (e != hipSuccess) return fail(GX_E_DEVICE, std::string("hipHostUnregister: ") + hipGetErrorString(e));
    return GX_OK;
}

// One CSR batch in host memory over several devices: lines are independent (core/Gorp.java:159-186 keeps no cross-line
// state), so the batch is cut into contiguous shards of about equal BYTES, one per handle (each on its own GPU, built
// from the same definition or blob), and every shard runs through its handle's host pipeline on its own thread.
int gx_extract_batch_multi(gx_handle* const* handles, int32_t n_handles, const uint8_t* bytes, const void* offsets, uint64_t n,
                           int32_t* match_id, int32_t* caps, const gx_batch_opts* opts) {
    if (!handles || n_handles <= 0 || !offsets) return fail(GX_E_ARG, "gx_extract_batch_multi: bad argument");
    return guarded([&]() -> int {
        const gx_batch_opts o = read_opts(opts);
        if (o.utf8) return fail(GX_E_ARG, "gx_extract_batch_multi: gx_batch_opts.utf8 is for gx_extract_batch (one device); shard the batch and call it per handle");
        if (o.device_pointers) return fail(GX_E_ARG, "gx_extract_batch_multi: host buffers only (device buffers belong to one device: use gx_extract_batch per handle)");
        for (int32_t k = 0; k < n_handles; ++k) {
            if (!handles[k] || !handles[k]->on_device) return fail(GX_E_ARG, "gx_extract_batch_multi: NULL or host-only handle");
            if (handles[k]->T.max_groups != handles[0]->T.max_groups || handles[k]->T.n_rules != handles[0]->T.n_rules)
                return fail(GX_E_ARG, "gx_extract_batch_multi: the handles were not built from the same definition");
        }
        const size_t off_w = o.offsets64 ? 8 : 4;
        const HostOffsets off{offsets, o.offsets64 != 0, n};
        // shard boundaries by bytes
        std::vector<uint64_t> cuts(static_cast<size_t>(n_handles) + 1, n);
        cuts[0] = 0;
        const uint64_t base = n ? off[0] : 0, total = n ? off[n] - base : 0;
        for (int32_t k = 1; k < n_handles; ++k)
            cuts[k] = off.lines_at_or_after(base + total / static_cast<uint64_t>(n_handles) * static_cast<uint64_t>(k), cuts[k - 1]);
        const bool compact = o.compact_results && !(o.match_only || !handles[0]->T.has_capture);
        const size_t slots = 2 * static_cast<size_t>(handles[0]->T.max_groups);
        std::vector<int> rc(static_cast<size_t>(n_handles), GX_OK);
        std::vector<std::string> msg(static_cast<size_t>(n_handles));
        std::vector<uint64_t> over(static_cast<size_t>(n_handles), 0);
        std::vector<std::thread> pool;
        for (int32_t k = 0; k < n_handles; ++k) {
            pool.emplace_back([&, k]() {
                const uint64_t a = cuts[k], m = cuts[k + 1] - cuts[k];
                if (m == 0) return;
                gx_batch_opts ok = o;
                ok.struct_size = sizeof(gx_batch_opts);
                ok.stream = nullptr;
                ok.overflow = compact ? &over[k] : nullptr;
                int32_t* mid_k = match_id ? match_id + a : nullptr;
                const size_t rb = row_bytes(row_format(true, o.compact_results == 2), static_cast<uint32_t>(slots));
                int32_t* caps_k = !caps ? nullptr : compact ? reinterpret_cast<int32_t*>(reinterpret_cast<uint8_t*>(caps) + a * rb) : caps + a * slots;
                rc[k] = gx_extract_batch(handles[k], bytes, static_cast<const uint8_t*>(offsets) + a * off_w, m, mid_k, caps_k, &ok);
                if (rc[k] != GX_OK) msg[k] = gx_last_error();
            });
        }
        for (auto& t : pool) t.join();
        for (int32_t k = 0; k < n_handles; ++k) if (rc[k] != GX_OK) return fail(rc[k], msg[k]);
        if (compact && o.overflow) for (uint64_t v : over) *static_cast<uint64_t*>(o.overflow) += v;
        return GX_OK;
    });
}

int gx_extract_batch_multi_device(const gx_device_shard* shards, int32_t n_shards, const gx_batch_opts* opts) {
    if (!shards || n_shards <= 0) return fail(GX_E_ARG, "gx_extract_batch_multi_device: bad argument");
    return guarded([&]() -> int {
        const gx_batch_opts o = read_opts(opts);
        if (o.utf8)
            return fail(GX_E_ARG, "gx_extract_batch_multi_device: gx_batch_opts.utf8 is for gx_extract_batch (its fix-up waits for a read on the host: one "
                                  "device at a time); call it per shard");
        for (int32_t k = 0; k < n_shards; ++k)
            if (!shards[k].handle || !shards[k].handle->on_device) return fail(GX_E_ARG, "gx_extract_batch_multi_device: NULL or host-only handle");
        DeviceScope scope;
        int first_rc = GX_OK;
        std::string first_msg;
        std::vector<hipStream_t> used(static_cast<size_t>(n_shards), nullptr);
        std::vector<DeviceBatch> batches(static_cast<size_t>(n_shards));
        // enqueue everything first (asynchronous launches from this one thread), wait afterwards
        for (int32_t k = 0; k < n_shards; ++k) {
            const gx_device_shard& sh = shards[k];
            gx_handle* h = sh.handle;
            hipStream_t stream = static_cast<hipStream_t>(sh.stream);
            if (!stream) {
                std::lock_guard<std::mutex> lock(h->slot_mu);
                if (!h->multi_stream) {
                    if (hipSetDevice(h->device) != hipSuccess || hipStreamCreateWithFlags(h->multi_stream.out(), hipStreamNonBlocking) != hipSuccess) {
                        if (first_rc == GX_OK) { first_rc = GX_E_DEVICE; first_msg = "gx_extract_batch_multi_device: no stream on the shard's device"; }
                        continue;
                    }
                }
                stream = h->multi_stream.get();
            }
            used[k] = stream;
            gx_batch_opts ok = o;
            ok.struct_size = sizeof(gx_batch_opts);
            ok.device_pointers = 1;
            ok.no_sync = 1;
            ok.stream = stream;
            ok.overflow = sh.overflow;
            const int rc = sh.n ? extract_batch_impl(h, sh.bytes, sh.offsets, sh.n, sh.match_id, sh.caps, nullptr, &ok, &batches[k]) : GX_OK;
            if (rc != GX_OK && first_rc == GX_OK) { first_rc = rc; first_msg = gx_last_error(); }
        }
        if (!o.no_sync) {
            for (int32_t k = 0; k < n_shards; ++k) {
                if (!used[k]) continue;
                if (hipSetDevice(shards[k].handle->device) != hipSuccess || hipStreamSynchronize(used[k]) != hipSuccess) {
                    if (first_rc == GX_OK) { first_rc = GX_E_DEVICE; first_msg = "gx_extract_batch_multi_device: a shard's stream failed"; }
                    continue;
                }
                // this call waits for its batches, so a shard whose max_line_bytes promise did not hold (its kernel left the longer lines'
                // rows unwritten) is made good before it returns, as a synchronous gx_extract_batch is: the lines that were left, and
                // only they, so that the shard's *overflow counts every line once
                if (!batches[k].enqueued) continue;
                const int rc = guarded([&]() -> int { finish_device_batch(shards[k].handle, batches[k]); return GX_OK; });
                if (rc != GX_OK && first_rc == GX_OK) { first_rc = rc; first_msg = gx_last_error(); }
            }
        }
        if (first_rc != GX_OK) return fail(first_rc, first_msg);
        return GX_OK;
    });
}

// ---- one process, all GPUs of a node: the tables on every device, the rows back on one (north_star: "broadcast of the DFA tables
// and a final gather over xGMI" -- for the caller that is ONE process, core/Gorp.java:22; ranks of a job use RCCL: gorp_amd/dist.py) ----
int gx_create_on_devices(const void* blob, size_t size, const int32_t* devices, int32_t n_devices, uint32_t flags, gx_handle** handles) {
    if (!blob || !devices || !handles || n_devices <= 0) return fail(GX_E_ARG, "gx_create_on_devices: bad argument");
    if (flags & GX_CREATE_HOST_ONLY) return fail(GX_E_ARG, "gx_create_on_devices: host-only handles live on no device");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(GX_E_DEVICE, "no HIP device available (libgorp_hip needs a gfx950 GPU; there is no CPU fallback)");
    for (int32_t k = 0; k < n_devices; ++k) {
        handles[k] = nullptr;
        if (devices[k] < 0 || devices[k] >= count) return fail(GX_E_ARG, "gx_create_on_devices: no such device");
    }
    DeviceScope scope;
    // the first handle from the blob (host work + upload over the bus), the others beside it: their host-side tables in threads of
    // their own, their device images copied from the first handle's device
    int rc = GX_OK;
    std::string msg;
    if (hipSetDevice(devices[0]) != hipSuccess) rc = GX_E_DEVICE, msg = "gx_create_on_devices: hipSetDevice failed";
    if (rc == GX_OK) {
        rc = gx_create_from_blob(blob, size, flags, &handles[0]);
        if (rc != GX_OK) msg = gx_last_error();
    }
    if (rc == GX_OK && n_devices > 1) {
        std::vector<int> rcs(static_cast<size_t>(n_devices), GX_OK);
        std::vector<std::string> msgs(static_cast<size_t>(n_devices));
        std::vector<std::thread> th;
        const gx_handle* first = handles[0];
        for (int32_t k = 1; k < n_devices; ++k)
            th.emplace_back([&, k]() {
                if (hipSetDevice(devices[k]) != hipSuccess) { rcs[k] = GX_E_DEVICE; msgs[k] = "gx_create_on_devices: hipSetDevice failed"; return; }
                int can = 0;   // (peers read each other's memory directly once this is on; failing that the runtime stages the copy)
                if (devices[k] != first->device && hipDeviceCanAccessPeer(&can, devices[k], first->device) == hipSuccess && can)
                    (void)hipDeviceEnablePeerAccess(first->device, 0);
                (void)hipGetLastError();
                g_peer_src = first;
                rcs[k] = gx_create_from_blob(blob, size, flags, &handles[k]);
                g_peer_src = nullptr;
                if (rcs[k] != GX_OK) msgs[k] = gx_last_error();
            });
        for (auto& t : th) t.join();
        for (int32_t k = 1; k < n_devices && rc == GX_OK; ++k)
            if (rcs[k] != GX_OK) { rc = rcs[k]; msg = msgs[k]; }
    }
    if (rc != GX_OK) {
        for (int32_t k = 0; k < n_devices; ++k) { if (handles[k]) gx_destroy(handles[k]); handles[k] = nullptr; }
        return fail(rc, msg);
    }
    return GX_OK;
}

int gx_gather_rows(const gx_rows_shard* shards, int32_t n_shards, uint32_t row_bytes, int32_t dst_device, void* dst_rows, int32_t no_sync) {
    if (!shards || n_shards <= 0 || row_bytes == 0 || !dst_rows) return fail(GX_E_ARG, "gx_gather_rows: bad argument");
    for (int32_t k = 0; k < n_shards; ++k)
        if (!shards[k].handle || !shards[k].handle->on_device || (shards[k].n && !shards[k].rows)) return fail(GX_E_ARG, "gx_gather_rows: NULL or host-only handle, or no rows");
    DeviceScope scope;
    int rc = GX_OK;
    std::string msg;
    auto bad = [&](const char* what) { if (rc == GX_OK) { rc = GX_E_DEVICE; msg = what; } };
    uint64_t at = 0;
    for (int32_t k = 0; k < n_shards && rc == GX_OK; ++k) {
        gx_handle* h = shards[k].handle;
        const uint64_t bytes = shards[k].n * static_cast<uint64_t>(row_bytes);
        uint8_t* dst = static_cast<uint8_t*>(dst_rows) + at;
        at += bytes;
        if (bytes == 0) continue;
        if (hipSetDevice(h->device) != hipSuccess) { bad("gx_gather_rows: hipSetDevice failed"); break; }
        std::lock_guard<std::mutex> lock(h->slot_mu);
        if (!h->gather_stream) {
            if (hipStreamCreateWithFlags(h->gather_stream.out(), hipStreamNonBlocking) != hipSuccess ||
                hipEventCreateWithFlags(h->gather_event.out(), hipEventDisableTiming) != hipSuccess) { bad("gx_gather_rows: no stream on the shard's device"); break; }
            int can = 0;   // the shard's device writes into the root's memory itself: one link per peer, all of them at once
            if (h->device != dst_device && hipDeviceCanAccessPeer(&can, h->device, dst_device) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(dst_device, 0);
            (void)hipGetLastError();
        }
        // behind the shard's kernel (the stream it was enqueued on: the caller's, or the one gx_extract_batch_multi_device used) ...
        hipStream_t ks = static_cast<hipStream_t>(shards[k].stream);
        if (!ks) ks = h->multi_stream.get();
        if (ks) {
            if (hipEventRecord(h->gather_event.get(), ks) != hipSuccess || hipStreamWaitEvent(h->gather_stream.get(), h->gather_event.get(), 0) != hipSuccess) { bad("gx_gather_rows: event"); break; }
        }
        // ... on the copy stream of the shard's own device: the kernels of the next batch go on beside it
        const hipError_t e = h->device == dst_device ? hipMemcpyAsync(dst, shards[k].rows, bytes, hipMemcpyDeviceToDevice, h->gather_stream.get())
                                                     : hipMemcpyPeerAsync(dst, dst_device, shards[k].rows, h->device, bytes, h->gather_stream.get());
        if (e != hipSuccess) bad("gx_gather_rows: the copy between the devices failed");
    }
    if (rc == GX_OK && !no_sync) {
        for (int32_t k = 0; k < n_shards; ++k) {
            gx_handle* h = shards[k].handle;
            if (!h->gather_stream) continue;
            if (hipSetDevice(h->device) != hipSuccess || hipStreamSynchronize(h->gather_stream.get()) != hipSuccess) bad("gx_gather_rows: a copy stream failed");
        }
    }
    if (rc != GX_OK) return fail(rc, msg);
    return GX_OK;
}

int gx_gather_wait(gx_handle* const* handles, int32_t n_handles) {
    if (!handles || n_handles <= 0) return fail(GX_E_ARG, "gx_gather_wait: bad argument");
    DeviceScope scope;
    int rc = GX_OK;
    for (int32_t k = 0; k < n_handles; ++k) {
        gx_handle* h = handles[k];
        if (!h || !h->on_device) { rc = GX_E_ARG; continue; }
        if (!h->gather_stream) continue;
        if (hipSetDevice(h->device) != hipSuccess || hipStreamSynchronize(h->gather_stream.get()) != hipSuccess) rc = GX_E_DEVICE;
    }
    if (rc != GX_OK) return fail(rc, "gx_gather_wait: a handle without a device, or a copy stream that failed");
    return GX_OK;
}

int gx_state_accepts(const gx_handle* h, int32_t state, int32_t* indexes, int32_t cap) {
    if (!h || state >= h->T.m_states || (cap > 0 && !indexes)) return -GX_E_ARG;
    if (state < 0) return 0;
    const uint32_t b = h->T.m_accept_off[state], e = h->T.m_accept_off[state + 1];
    for (uint32_t i = b; i < e && static_cast<int32_t>(i - b) < cap; ++i) indexes[i - b] = h->T.m_accept_list[i];
    return static_cast<int>(e - b);
}

// mode: 0 = extract, 1 = match only, -(k + 1) = extraction k's capture regexp alone.
// One String per call is latency, not throughput: the handle keeps a device scratch buffer and a pinned host mirror
// of it ([offsets 8 B][code units][match id, state, captures]), so a call is one copy in, one launch, one copy out.
static int one_line(gx_handle* h, const uint16_t* s, int32_t len, int32_t* match_id, int32_t* caps, int32_t* state, int mode) {
    if (!h || len < 0 || (len && !s)) return fail(GX_E_ARG, "bad argument");
    if (!h->on_device) return fail(GX_E_DEVICE, "handle was created host-only; no device tables (there is no CPU fallback)");
    return guarded([&]() -> int {
        GX_HIP(hipSetDevice(h->device));
        std::lock_guard<std::mutex> lock(h->mu);
        const size_t slots = 2 * static_cast<size_t>(h->T.max_groups);
        const size_t out_words = 2 + slots;
        const size_t in_bytes = 8 + ((static_cast<size_t>(len) * 2 + 7) & ~size_t(7));  // offsets + code units: one copy in
        const size_t need = in_bytes + out_words * 4 + 16;
        gx_handle::OneScratch& one = h->one;
        if (need > one.cap) {
            one = {};
            const size_t cap = std::max<size_t>(need * 2, 4096);
            GX_HIP(hipMalloc(one.dev.out(), cap));
            GX_HIP(hipHostMalloc(one.host.out(), cap, hipHostMallocDefault));
            one.cap = cap;
        }
        uint8_t* hb = one.host.get();
        uint8_t* db = one.dev.get();
        uint32_t* offs = reinterpret_cast<uint32_t*>(hb);
        offs[0] = 0; offs[1] = static_cast<uint32_t>(len);
        if (len) memcpy(hb + 8, s, static_cast<size_t>(len) * 2);
        bool latin1 = mode == 0 && len > 0 && len <= 4096 && h->tiles.tile_ok;
        for (int32_t q = 0; latin1 && q < len; ++q) latin1 = s[q] <= 0xFFu;
        if (latin1 && h->svc.enabled && static_cast<uint32_t>(len) <= GX_SERVICE_MAX_BYTES) {
            // the resident wave (gx_service.hip): the line into the mailbox -- every cache line's text before its tag, the first cache
            // line, whose tag is what the wave polls, last -- and a spin on the answer's sequence number
            gx_handle::Service& sv = h->svc;
            uint32_t* mb = sv.host.get();
            int32_t* ans = reinterpret_cast<int32_t*>(mb + 17 * 16);
            uint32_t* state = mb + 17 * 16 + 80;
            const uint32_t seq = ++sv.seq ? sv.seq : ++sv.seq;   // (never 0... the wave compares for inequality only, but keep it tidy)
            const uint32_t ulen = static_cast<uint32_t>(len);
            for (uint32_t cl = 1; 56u + 60u * (cl - 1u) < ulen; ++cl) {
                uint8_t* dst = reinterpret_cast<uint8_t*>(mb + 16u * cl) + 4;
                const uint32_t from = 56u + 60u * (cl - 1u), cnt = std::min(60u, ulen - from);
                for (uint32_t q = 0; q < cnt; ++q) dst[q] = static_cast<uint8_t>(s[from + q]);
                __atomic_store_n(mb + 16u * cl, seq, __ATOMIC_RELEASE);
            }
            {
                uint8_t* dst = reinterpret_cast<uint8_t*>(mb) + 8;
                for (uint32_t q = 0; q < std::min(56u, ulen); ++q) dst[q] = static_cast<uint8_t>(s[q]);
                mb[1] = ulen;   // (flags 0)
                __atomic_store_n(mb, seq, __ATOMIC_RELEASE);
            }
            auto start_wave = [&]() {
                __atomic_store_n(state, 1u, __ATOMIC_RELEASE);
                // the wave starts with the PREVIOUS sequence number as the last one it has seen: the request that is waiting is new to it
                GX_HIP(launch_one_service(sv.mode, sv.L, static_cast<const uint8_t*>(h->d_img[IMG_DENSE].get()), sv.dev, reinterpret_cast<int32_t*>(sv.dev + 17 * 16),
                                          sv.dev + 17 * 16 + 80, seq - 1u, h->T.max_groups, 30000ull, 2000000ull, sv.stream.get()));
                sv.started = true;
                ++sv.launches;
            };
            if (!sv.started) start_wave();
            const uint32_t* ans_seq = reinterpret_cast<const uint32_t*>(ans) + 1 + 2 * h->T.max_groups;
            uint64_t spins = 0;
            while (__atomic_load_n(ans_seq, __ATOMIC_ACQUIRE) != seq) {
                if ((++spins & 63u) == 0 && __atomic_load_n(state, __ATOMIC_ACQUIRE) == 2u && hipStreamQuery(sv.stream.get()) == hipSuccess) {
                    // the wave has left (idle, or its time was up) -- without this request's answer: a fresh one
                    if (__atomic_load_n(ans_seq, __ATOMIC_ACQUIRE) == seq) break;
                    start_wave();
                }
                if (spins > (1ull << 34)) throw GxError(GX_E_DEVICE, "the resident one-line service does not answer");
            }
            if (match_id) *match_id = ans[0];
            if (caps) for (size_t t = 0; t < slots; ++t) caps[t] = h->T.has_capture ? ans[1 + t] : -1;
            return GX_OK;
        }
        // the result words, in the pinned buffer after the line: match id, state, captures
        int32_t* out = reinterpret_cast<int32_t*>(hb + in_bytes);
        GxBatch b{};
        b.n = 1;
        if (latin1) {
            // Gorp.extract(String) on a Latin-1 line -- nearly every call: the line's BYTES go through the batch kernels as a batch of
            // one (tables in LDS, the line staged there too: a step costs an LDS round trip, not two trips to L2 as in the per-line
            // kernel), straight out of the pinned buffer and back into it; the host knows the line fits: no follow-up launch
            uint8_t* bytes = hb + 8;
            for (int32_t q = 0; q < len; ++q) bytes[q] = static_cast<uint8_t>(s[q]);   // (in place of the units copied above)
            b.data = bytes; b.offsets = hb;
            b.match_only = h->T.has_capture ? 0 : 1;
            b.match_id = out; b.caps = h->T.has_capture ? out + 2 : nullptr;
            b.no_followup = 1;
            launch_batch(h, b, static_cast<uint32_t>(len), GX_KERNEL_AUTO, nullptr);
        } else {
            b.wide = 1;
            b.match_only = mode < 0 ? mode : ((mode == 1 || !h->T.has_capture) ? 1 : 0);
            PikeGate pike_gate(h, nullptr);
            if (len <= 16384) {
                // the short way: the kernel reads the units out of the pinned buffer and writes the result words into it (no copy commands)
                b.match_id = out; b.state_out = out + 1; b.caps = b.match_only == 1 ? nullptr : out + 2;
                GX_HIP(launch_extract_one(h->dev, reinterpret_cast<const uint16_t*>(hb + 8), static_cast<uint32_t>(len), b, nullptr));
            } else {
                // (the results area is not initialised: the kernel writes every word that is read back)
                GX_HIP(hipMemcpyAsync(db, hb, in_bytes, hipMemcpyHostToDevice, nullptr));
                int32_t* dout = reinterpret_cast<int32_t*>(db + in_bytes);
                b.data = db + 8; b.offsets = db;
                b.match_id = dout; b.state_out = dout + 1; b.caps = b.match_only == 1 ? nullptr : dout + 2;
                GX_HIP(launch_extract_generic(h->dev, b, nullptr));
                GX_HIP(hipMemcpyAsync(out, dout, (b.match_only == 1 ? 2 : out_words) * 4, hipMemcpyDeviceToHost, nullptr));
            }
        }
        GX_HIP(hipStreamSynchronize(nullptr));
        if (match_id) *match_id = out[0];
        if (state) *state = out[1];
        if (caps) for (size_t t = 0; t < slots; ++t) caps[t] = b.match_only == 1 ? -1 : out[2 + t];
        return GX_OK;
    });
}

int gx_capture_one_utf16(gx_handle* h, int32_t k, const uint16_t* s, int32_t len, int32_t* matched, int32_t* caps) {
    if (!h || k < 0 || k >= h->T.n_rules || !matched) return fail(GX_E_ARG, "gx_capture_one_utf16: bad argument");
    if (!h->T.has_capture) {  // no extraction of this definition has groups: a plain regexp match (the generic kernel needs capture tables)
        return fail(GX_E_ARG, "gx_capture_one_utf16: the definition has no capture groups");
    }
    int32_t mid = -1;
    const int rc = one_line(h, s, len, &mid, caps, nullptr, -(k + 1));
    if (rc != GX_OK) return rc;
    *matched = mid == k ? 1 : 0;
    return GX_OK;
}

int gx_extract_one_utf16(gx_handle* h, const uint16_t* s, int32_t len, int32_t* match_id, int32_t* caps) {
    if (!match_id) return fail(GX_E_ARG, "gx_extract_one_utf16: match_id is NULL");
    return one_line(h, s, len, match_id, caps, nullptr, 0);
}

int gx_match_one_utf16(gx_handle* h, const uint16_t* s, int32_t len, int32_t* indexes, int32_t cap) {
    int32_t mid = -1, state = -1;
    int rc = one_line(h, s, len, &mid, nullptr, &state, 1);
    if (rc != GX_OK) return -rc;
    if (state < 0) return 0;
    const uint32_t b = h->T.m_accept_off[state], e = h->T.m_accept_off[state + 1];
    for (uint32_t i = b; i < e && static_cast<int32_t>(i - b) < cap; ++i) indexes[i - b] = h->T.m_accept_list[i];
    return static_cast<int>(e - b);
}

static int string_result(const ustr& r, char* out, size_t cap, size_t* out_len) {
    std::string u = u16_to_utf8(r);
    if (out_len) *out_len = u.size();
    if (!out || cap < u.size() + 1) return fail(GX_E_ARG, "output buffer too small");
    memcpy(out, u.c_str(), u.size() + 1);
    return GX_OK;
}

int gx_quote_literal_as_regexp(const char* text, char* out, size_t cap, size_t* out_len) {
    if (!text) return fail(GX_E_ARG, "null text");
    return guarded([&]() -> int { return string_result(quote_literal_as_regexp(utf8_to_u16(text)), out, cap, out_len); });
}
int gx_massage_regexp_for_automaton(const char* pattern, char* out, size_t cap, size_t* out_len) {
    if (!pattern) return fail(GX_E_ARG, "null pattern");
    return guarded([&]() -> int { return string_result(massage_regexp_for_automaton(utf8_to_u16(pattern)), out, cap, out_len); });
}
int gx_massage_regexp_for_jdk(const char* pattern, char* out, size_t cap, size_t* out_len) {
    if (!pattern) return fail(GX_E_ARG, "null pattern");
    return guarded([&]() -> int { return string_result(massage_regexp_for_jdk(utf8_to_u16(pattern)), out, cap, out_len); });
}

int gx_create_from_definition(const char* definition_text, const char* source_ref, uint32_t flags, gx_handle** out) {
    if (!definition_text || !out) return fail(GX_E_ARG, "gx_create_from_definition: bad argument");
    return guarded([&]() -> int {
        std::vector<dsl::Extraction> xs = dsl::read_definition(definition_text, source_ref ? source_ref : "<input string>");
        std::vector<ustr> a, j;
        for (auto& x : xs) {
            std::string as, js;
            dsl::build_regex_strings(x, as, js);
            a.push_back(utf8_to_u16(as.c_str()));
            j.push_back(utf8_to_u16(js.c_str()));
        }
        std::unique_ptr<gx_handle> h(new gx_handle());
        try {
            h->T = compile_tables(a, &j, (flags & GX_CREATE_PROGRAMS) != 0);
        } catch (GxError& e) {
            // core/Gorp.java:84-90
            if (e.code == GX_E_DEVICE || e.code == GX_E_NOMEM) throw;
            throw GxError(e.code, std::string("(N/A): Internal error: problem with PolyMatcher construction: ") + e.what());
        }
        h->meta = xs;
        return finish_create(h, flags, out);
    });
}

const char* gx_extraction_name(const gx_handle* h, int32_t k) {
    if (!h || k < 0 || k >= static_cast<int32_t>(h->meta.size())) return nullptr;
    return h->meta[k].name.c_str();
}
const char* gx_extractor_name(const gx_handle* h, int32_t k, int32_t g) {
    if (!h || k < 0 || k >= static_cast<int32_t>(h->meta.size())) return nullptr;
    if (g < 0 || g >= static_cast<int32_t>(h->meta[k].extractor_names.size())) return nullptr;
    return h->meta[k].extractor_names[g].c_str();
}
const char* gx_extraction_append_json(const gx_handle* h, int32_t k) {
    if (!h || k < 0 || k >= static_cast<int32_t>(h->meta.size()) || h->meta[k].append_json.empty()) return nullptr;
    return h->meta[k].append_json.c_str();
}

static const std::vector<std::pair<std::string, std::string>>* append_entries_of(const gx_handle* hc, int32_t k) {
    gx_handle* h = const_cast<gx_handle*>(hc);
    if (!h || k < 0 || k >= static_cast<int32_t>(h->meta.size())) return nullptr;
    std::lock_guard<std::mutex> lock(h->mu);
    if (h->append_entries.size() != h->meta.size()) {
        h->append_entries.assign(h->meta.size(), {});
        for (size_t x = 0; x < h->meta.size(); ++x)
            if (!h->meta[x].append_json.empty()) h->append_entries[x] = dsl::json_object_entries(h->meta[x].append_json);
    }
    return &h->append_entries[k];
}
int32_t gx_extraction_append_count(const gx_handle* h, int32_t k) {
    auto* e = append_entries_of(h, k);
    return e ? static_cast<int32_t>(e->size()) : 0;
}
const char* gx_extraction_append_key(const gx_handle* h, int32_t k, int32_t j) {
    auto* e = append_entries_of(h, k);
    return (e && j >= 0 && j < static_cast<int32_t>(e->size())) ? (*e)[j].first.c_str() : nullptr;
}
const char* gx_extraction_append_value_json(const gx_handle* h, int32_t k, int32_t j) {
    auto* e = append_entries_of(h, k);
    return (e && j >= 0 && j < static_cast<int32_t>(e->size())) ? (*e)[j].second.c_str() : nullptr;
}

int gx_definition_to_json(const char* definition_text, const char* source_ref, const char* stage, char* out, size_t cap,
                          size_t* out_len) {
    if (!definition_text || !stage) return fail(GX_E_ARG, "gx_definition_to_json: bad argument");
    return guarded([&]() -> int {
        std::string js = dsl::dump_json(definition_text, source_ref ? source_ref : "<input string>", stage);
        if (out_len) *out_len = js.size();
        if (!out || cap < js.size() + 1) return fail(GX_E_ARG, "output buffer too small");
        memcpy(out, js.c_str(), js.size() + 1);
        return GX_OK;
    });
}

}  // extern "C"

#ifdef GX_DEV
// Developer build only (libgorp_hip_dev.so, `python -m gorp_amd.build --dev`): the tile kernel adds up the cycles
// each wave spends in its four phases (stage, prefetch issue, walk, results) into this device buffer,
// 8 x uint64 per wave of the grid (256 workgroups x 12 waves at most; gx_tile_body.hpp: TileIO::stamps).  Not part of the product ABI.
namespace gx { hipError_t jsonl_dev_phases(unsigned long long* out16, int reset); }
// cycles per phase of the JSONL tile kernels summed over their waves since the last reset: [0..5] sizes pass, [8..13] write pass
extern "C" int gx_dev_jsonl_phases(unsigned long long* out16, int reset) { return gx::jsonl_dev_phases(out16, reset) == hipSuccess ? GX_OK : GX_E_DEVICE; }
extern "C" int gx_dev_set_stamps(gx_handle* h, void* device_buffer) {
    if (!h) return GX_E_ARG;
    h->dev_stamps = static_cast<unsigned long long*>(device_buffer);
    return GX_OK;
}
#endif
