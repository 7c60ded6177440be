// slots_test.cpp -- LaunchSlots (gorp_amd/csrc/gx_slots.hpp) on the CPU: this program plays the device (it writes a slot's pinned
// words the way announce_left_line in gx_device.hpp does) and the host calls of gx_api.cpp (take_slot, finish_device_batch), and
// replays the orders in which batches that break their max_line_bytes promise can meet on a stream.  The invariant throughout: a
// no_sync batch that left a row unwritten is reported by an error from a later call on its stream, at the latest by the first call
// after the stream has drained; a synchronous call learns of its own break (and makes good); every break is accounted for once.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gx_slots.hpp"

using gx::LaunchSlots;

static int failures = 0;
#define CHECK(cond, what)                                                                 \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            std::printf("FAIL %s:%d: %s -- %s\n", __FILE__, __LINE__, #cond, what);     \
            ++failures;                                                                   \
        }                                                                                 \
    } while (0)

// A handle's slots and their pinned words, the device, and the host's two calls.
struct Model {
    LaunchSlots S;
    uint32_t words[2 * LaunchSlots::N] = {};
    int errors = 0;   // calls that ended with the "an earlier no_sync batch ..." error

    Model() { S.broken = words; S.broken_count = words + LaunchSlots::N; }

    struct Batch {
        LaunchSlots::Use use{};
        bool promised = false;
        bool launched = false;
    };
    // the device: a launch leaves a line (announce_left_line: exchange the word, count the launch's first)
    void device_leaves(const Batch& b) {
        const uint32_t old = words[b.use.slot];
        words[b.use.slot] = b.use.seq;
        if (old != b.use.seq) ++words[LaunchSlots::N + b.use.slot];
    }
    // take_slot: a new launch; refused (and the break reported) when the slot shows a break nobody has accounted for
    Batch submit(const void* stream, bool promised) {
        Batch b;
        b.use = S.take(stream);
        b.promised = promised;
        if (S.consume_broken(b.use.slot)) { ++errors; return b; }
        b.launched = true;
        return b;
    }
    // finish_device_batch after the stream has drained: returns the verdict; `earlier` is an error to the caller
    LaunchSlots::Verdict finish(const Batch& b) {
        const LaunchSlots::Verdict v = S.finished(b.use.slot, b.use.seq, b.promised);
        if (v.earlier) ++errors;
        return v;
    }
    uint64_t stat24() const { return S.promises_broken.load(); }
};

static const void* key(uintptr_t k) { return reinterpret_cast<const void*>(k * 64); }

static void a_breaks_b_sync_breaks() {
    Model m;
    Model::Batch a = m.submit(key(1), true);   // no_sync
    Model::Batch b = m.submit(key(1), true);   // synchronous, submitted while A is still queued
    CHECK(a.launched && b.launched && m.errors == 0, "nothing has run: nothing to report at B's submission");
    m.device_leaves(a);
    m.device_leaves(a);
    m.device_leaves(b);
    const LaunchSlots::Verdict v = m.finish(b);
    CHECK(v.mine, "B broke its own promise: it makes good");
    CHECK(v.earlier, "A's unwritten row is reported when B finishes");
    CHECK(m.errors == 1 && m.stat24() == 2, "two broken batches, one error");
    Model::Batch c = m.submit(key(1), false);
    CHECK(c.launched && m.errors == 1, "reported once: the next call is clean");
    CHECK(!m.finish(c).mine && !m.finish(c).earlier && m.stat24() == 2, "nothing new");
}

static void a_breaks_b_sync_holds() {
    Model m;
    Model::Batch a = m.submit(key(1), true);
    Model::Batch b = m.submit(key(1), true);
    m.device_leaves(a);
    const LaunchSlots::Verdict v = m.finish(b);
    CHECK(!v.mine, "B's promise held: nothing to make good (and no second run of B)");
    CHECK(v.earlier && m.errors == 1 && m.stat24() == 1, "A is reported by B");
    // the same with A finished before B is submitted: B is refused at submission
    Model m2;
    Model::Batch a2 = m2.submit(key(1), true);
    m2.device_leaves(a2);
    Model::Batch b2 = m2.submit(key(1), true);
    CHECK(!b2.launched && m2.errors == 1 && m2.stat24() == 1, "A is reported at B's submission");
    Model::Batch c2 = m2.submit(key(1), true);
    CHECK(c2.launched && !m2.finish(c2).earlier && m2.errors == 1, "once");
}

static void two_no_sync_breaks_then_a_clean_call() {
    for (int order = 0; order < 3; ++order) {
        Model m;
        Model::Batch a = m.submit(key(1), true);
        if (order == 1) m.device_leaves(a);            // A has run before B is submitted: B is refused
        Model::Batch b = m.submit(key(1), true);
        if (order == 2) m.device_leaves(a);            // ... before C is submitted: C is refused
        if (b.launched && order == 2) m.device_leaves(b);
        Model::Batch c = m.submit(key(1), false);
        if (order == 0) { m.device_leaves(a); m.device_leaves(b); }
        if (c.launched) {
            const LaunchSlots::Verdict v = m.finish(c);
            CHECK(!v.mine, "C made no promise");
            CHECK(v.earlier == (order == 0), "C reports what its submission did not");
        }
        CHECK(m.errors >= 1, "B or C raises");
        Model::Batch d = m.submit(key(1), false);      // the first call after the stream has drained
        if (d.launched) m.finish(d);
        const int errors = m.errors;
        CHECK(m.stat24() == (order == 1 ? 1u : 2u), "every batch that ran and broke is accounted for");
        Model::Batch e = m.submit(key(1), false);
        CHECK(e.launched && !m.finish(e).earlier && m.errors == errors, "a further clean call does not raise again");
    }
}

static void two_streams_each_report_their_own() {
    Model m;
    Model::Batch a = m.submit(key(1), true), b = m.submit(key(2), true);
    CHECK(a.use.slot != b.use.slot, "a slot per stream");
    m.device_leaves(a);
    Model::Batch a2 = m.submit(key(1), false);
    CHECK(!a2.launched && m.errors == 1, "stream 1 reports its own break");
    Model::Batch b2 = m.submit(key(2), false);
    CHECK(b2.launched && !m.finish(b2).earlier && m.errors == 1, "stream 2 has none yet, and is not told of stream 1's");
    m.device_leaves(b);
    Model::Batch a3 = m.submit(key(1), false);
    CHECK(a3.launched && !m.finish(a3).earlier && m.errors == 1, "stream 1 is not told of stream 2's");
    Model::Batch b3 = m.submit(key(2), false);
    CHECK(!b3.launched && m.errors == 2 && m.stat24() == 2, "stream 2 reports its own");
}

static void promises_that_hold_count_nothing() {
    Model m;
    for (int q = 0; q < 1000; ++q) {
        Model::Batch b = m.submit(key(1 + q % 5), q % 2 == 0);
        CHECK(b.launched, "no break, no refusal");
        if (q % 3 == 0) {
            const LaunchSlots::Verdict v = m.finish(b);
            CHECK(!v.mine && !v.earlier, "no break, no verdict");
        }
    }
    CHECK(m.errors == 0 && m.stat24() == 0, "gx_stat(h, 24) does not move while all promises hold");
    // a launch that ran with its follow-up (no promise taken) and left lines wrote device words, not these: never `mine`
    Model::Batch b = m.submit(key(1), false);
    CHECK(!m.finish(b).mine, "not promised");
    // a handle without slots
    LaunchSlots none;
    const LaunchSlots::Use u = none.take(key(1));
    CHECK(none.consume_broken(u.slot) == 0 && !none.finished(u.slot, u.seq, true).mine, "no words, no breaks");
}

static void sequence_numbers_wrap_past_zero() {
    Model m;
    m.S.next_seq = 0xFFFFFFFEu;
    Model::Batch a = m.submit(key(1), true), b = m.submit(key(1), true), c = m.submit(key(1), true);
    CHECK(a.use.seq == 0xFFFFFFFEu && b.use.seq == 0xFFFFFFFFu && c.use.seq == 1u, "0 is never a sequence number (the words start as 0)");
    m.device_leaves(b);
    m.device_leaves(c);
    const LaunchSlots::Verdict v = m.finish(c);
    CHECK(v.mine && v.earlier && m.stat24() == 2, "across the wrap");
    // the count wraps too: the host's arithmetic is the device's
    Model w;
    w.words[LaunchSlots::N + 0] = 0xFFFFFFFFu;
    w.S.seen_count[0] = 0xFFFFFFFFu;
    Model::Batch d = w.submit(key(1), true);
    CHECK(d.use.slot == 0 && d.launched, "seen == count: nothing fresh");
    w.device_leaves(d);
    CHECK(w.words[LaunchSlots::N] == 0u, "the device's count wrapped");
    const LaunchSlots::Verdict vw = w.finish(d);
    CHECK(vw.mine && !vw.earlier && w.stat24() == 1, "one break across the count's wrap");
    // a word that still holds this launch's number from 2^32 launches ago, and nothing broke now
    Model s;
    Model::Batch e = s.submit(key(1), true);
    s.device_leaves(e);
    CHECK(s.finish(e).mine, "the break");
    s.S.next_seq = e.use.seq;
    Model::Batch f = s.submit(key(1), true);
    CHECK(f.use.seq == e.use.seq && f.launched, "the same number again");
    const LaunchSlots::Verdict vs = s.finish(f);
    CHECK(!vs.mine && !vs.earlier && s.stat24() == 1, "a stale word is not a break");
}

static void the_shared_slot() {
    Model m;
    std::vector<Model::Batch> own;
    for (uintptr_t k = 1; k <= static_cast<uintptr_t>(LaunchSlots::N - 1); ++k) {
        own.push_back(m.submit(key(k), true));
        CHECK(own.back().use.slot == static_cast<int>(k - 1) && !own.back().use.shared, "the first N - 1 streams own a slot each");
    }
    Model::Batch x = m.submit(key(100), true);
    CHECK(x.use.slot == LaunchSlots::N - 1 && x.use.shared && !x.use.wait_shared, "the next stream takes the shared slot; its first user waits for nobody");
    Model::Batch y = m.submit(key(101), true);
    CHECK(y.use.slot == LaunchSlots::N - 1 && y.use.shared && y.use.wait_shared, "later users wait for the one before (the event)");
    CHECK(m.submit(key(3), true).use.slot == 2, "an owner keeps its slot");
    // launches of the shared slot run one after the other (the event), so the word and the count work as on one stream; its
    // streams share the reports as they share the words
    m.device_leaves(x);
    m.device_leaves(y);
    const LaunchSlots::Verdict v = m.finish(y);
    CHECK(v.mine && v.earlier && m.errors == 1 && m.stat24() == 2, "stream 101 makes good and reports stream 100's break");
    Model::Batch x2 = m.submit(key(100), false);
    CHECK(x2.launched && m.errors == 1, "reported once");
    m.device_leaves(own[4]);
    Model::Batch z = m.submit(key(102), false);
    CHECK(z.launched && !m.finish(z).earlier, "an owned slot's break is not the shared slot's");
    Model::Batch o = m.submit(key(5), false);
    CHECK(!o.launched && m.errors == 2 && m.stat24() == 3, "... but its owner's");
}

int main() {
    a_breaks_b_sync_breaks();
    a_breaks_b_sync_holds();
    two_no_sync_breaks_then_a_clean_call();
    two_streams_each_report_their_own();
    promises_that_hold_count_nothing();
    sequence_numbers_wrap_past_zero();
    the_shared_slot();
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("slots checks ok\n");
    return 0;
}
