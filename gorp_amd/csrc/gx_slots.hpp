// gx_slots.hpp -- the bookkeeping of a handle's launch slots: plain C++ over stream keys, no HIP.  gx_api.cpp keeps the slots'
// device words and events and makes the HIP calls beside the calls into this struct.
//
// Tile-kernel launches that are in flight share nothing but these slots: one word each, into which a launch stores its sequence
// number when it meets a line it cannot stage (gx_device.hpp: GxBatch::oversize_flag).  A slot belongs to ONE STREAM for the life of
// the handle (launches of a stream run in order, so the word is free again when the stream's next launch begins: nothing to wait for,
// nothing to record); the last slot is shared by the streams that come after N - 1 others and is handed over with an event.
// Batches that promise their longest line (gx_batch_opts.max_line_bytes) have no follow-up launch; their flag word is in pinned host
// memory (one per slot; the device writes it only if the promise is broken), so that the host can see it.  That word holds the
// sequence number of the last launch of the slot that broke its promise.
#pragma once
#include <atomic>
#include <cstdint>

namespace gx {

struct LaunchSlots {
    static const int N = 32;
    const void* stream[N] = {};          // the stream that owns slot q < N - 1
    bool taken[N] = {};
    uint32_t seen[N] = {};               // the slot's pinned word as the host last saw it
    uint32_t steal_parity[N] = {};       // the row the slot's next tile-kernel launch draws from
    uint32_t chunk_tickets[N] = {};      // what the slot's chunk counter will read when its next launch begins
    bool shared_used = false;            // the shared slot has had a user: the next one waits for its event
    uint32_t next_seq = 1;
    std::atomic<uint64_t> promises_broken{0};
    const uint32_t* broken = nullptr;    // the pinned words [N] (null: the handle has no slots)

    struct Use {
        int slot;
        bool shared;
        bool wait_shared;   // the shared slot's previous user must be done first
        uint32_t seq;
    };

    // The slot of `key`'s launches: the one it owns, else the shared one.
    int slot_of(const void* key) const {
        for (int q = 0; q < N - 1; ++q)
            if (taken[q] && stream[q] == key) return q;
        return N - 1;
    }
    // A new launch on `key`: its sequence number (never 0) and its slot -- the one the stream owns, a free one, or the shared one.
    Use take(const void* key) {
        const uint32_t seq = next_seq++;
        if (next_seq == 0) next_seq = 1;
        int slot = slot_of(key);
        for (int q = 0; q < N - 1 && slot == N - 1; ++q)
            if (!taken[q]) { taken[q] = true; stream[q] = key; slot = q; }
        const bool shared = slot == N - 1, wait = shared && shared_used;
        if (shared) shared_used = true;
        return Use{slot, shared, wait, seq};
    }
    uint32_t word(int slot) const { return __atomic_load_n(&broken[slot], __ATOMIC_RELAXED); }
    // Has a launch of the slot broken its promise since the host last looked?  Marks the word seen and counts the break.
    bool consume_broken(int slot) {
        if (!broken) return false;
        const uint32_t w = word(slot);
        if (w == seen[slot]) return false;
        mark_seen(slot, w);
        return true;
    }
    // The caller found launch `seq`'s own break and puts it right itself: seen, and counted.
    void mark_seen(int slot, uint32_t seq) {
        seen[slot] = seq;
        promises_broken.fetch_add(1);
    }
};

}  // namespace gx
