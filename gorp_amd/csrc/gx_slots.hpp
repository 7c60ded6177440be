// gx_slots.hpp -- the bookkeeping of a handle's launch slots: plain C++ over stream keys, no HIP.  gx_api.cpp keeps the slots'
// device words and events and makes the HIP calls beside the calls into this struct (tests/cpp/slots_test.cpp plays the device).
//
// Tile-kernel launches that are in flight share nothing but these slots: one word each, into which a launch stores its sequence
// number when it meets a line it cannot stage (gx_device.hpp: GxBatch::oversize_flag).  A slot belongs to ONE STREAM for the life of
// the handle (launches of a stream run in order, so the word is free again when the stream's next launch begins: nothing to wait for,
// nothing to record); the last slot is shared by the streams that come after N - 1 others and is handed over with an event.
//
// Batches that promise their longest line (gx_batch_opts.max_line_bytes) have no follow-up launch; their flag word is in pinned host
// memory, so that the host can see it, and has a neighbour (the device writes both only if the promise is broken):
//   broken[slot]         the sequence number of the last launch of the slot that broke its promise   ("did THIS launch break?")
//   broken_count[slot]   how many launches of the slot have broken their promise, ever                ("did one before it break?")
// A launch exchanges its sequence number into the first word wherever it leaves a line and adds one to the second when the word held
// another number before -- once per launch, since the launches of a slot run one after the other.  The host keeps the word as it last
// saw it and the count it has accounted for: every break is reported exactly once, either made good by the synchronous call that
// caused it (finished) or as an error by the first call on the slot that sees the count ahead (take_slot through consume_broken,
// or finished).  Without the counts (broken_count null) a changed word is all there is to see: one report for however many
// launches broke.  The streams of the shared slot share its reports as they share its words: a break on one of them is reported
// to whichever of them calls next, and a synchronous launch whose word another stream's launch has overwritten since is not made
// good but reported like a no_sync one.
#pragma once
#include <atomic>
#include <cstdint>

namespace gx {

struct LaunchSlots {
    static const int N = 32;
    const void* stream[N] = {};          // the stream that owns slot q < N - 1
    bool taken[N] = {};
    uint32_t seen[N] = {};               // the slot's pinned word as the host last saw it
    uint32_t seen_count[N] = {};         // the slot's count of broken promises that the host has accounted for
    uint32_t steal_parity[N] = {};       // the row the slot's next tile-kernel launch draws from
    uint32_t chunk_tickets[N] = {};      // what the slot's chunk counter will read when its next launch begins
    bool shared_used = false;            // the shared slot has had a user: the next one waits for its event
    uint32_t next_seq = 1;
    std::atomic<uint64_t> promises_broken{0};   // launches that broke their promise, as accounted for so far (gx_stat(h, 24))
    const uint32_t* broken = nullptr;    // the pinned words [N] (null: the handle has no slots)
    const uint32_t* broken_count = nullptr;   // the pinned counts [N]

    struct Use {
        int slot;
        bool shared;
        bool wait_shared;   // the shared slot's previous user must be done first
        uint32_t seq;
    };
    // What the host owes after a launch of a slot has finished.
    struct Verdict {
        bool mine;      // this launch left lines: run its follow-up now (the caller waits for its batch, so it can)
        bool earlier;   // a launch before it, which nobody waited for, left lines: their rows are unwritten -- report it
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
    // Launches of the slot that have broken their promise and are not accounted for yet: accounts for them (the caller reports them).
    // May be called while launches of the slot are in flight: a break that shows later is found by a later call.
    uint32_t consume_broken(int slot) {
        if (!broken) return 0;
        const uint32_t w = word(slot);
        uint32_t fresh = w != seen[slot] ? 1u : 0u;
        if (broken_count) fresh = __atomic_load_n(&broken_count[slot], __ATOMIC_RELAXED) - seen_count[slot];   // (modulo 2^32, as the device counts)
        seen[slot] = w;
        seen_count[slot] += fresh;
        promises_broken.fetch_add(fresh);
        return fresh;
    }
    // The caller found launch `seq`'s own break and puts it right itself: seen, and counted.
    void mark_seen(int slot, uint32_t seq) {
        seen[slot] = seq;
        ++seen_count[slot];
        promises_broken.fetch_add(1);
    }
    // Launch `seq` of the slot has finished and so has everything before it on its stream(s); `promised`: it ran without a follow-up
    // launch, on the caller's promise.  Accounts for every break the slot has had since the host last looked and tells them apart.
    Verdict finished(int slot, uint32_t seq, bool promised) {
        if (!broken) return Verdict{false, false};
        // (a word that still holds this number from 2^32 launches ago while the count has not moved: nothing broke now)
        const bool moved = broken_count ? __atomic_load_n(&broken_count[slot], __ATOMIC_RELAXED) != seen_count[slot] : word(slot) != seen[slot];
        const bool mine = promised && word(slot) == seq && moved;
        if (mine) mark_seen(slot, seq);
        return Verdict{mine, consume_broken(slot) != 0};
    }
};

}  // namespace gx
