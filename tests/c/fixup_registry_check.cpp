// Host-only check of mpich_amd/csrc/redop_fixup.h, the one header it
// includes: the registry of the split combiners' fixup-word buffers against a
// fake device.  Built with g++ by tests/test_fixup_registry.py, as it is and
// with -fsanitize=thread.
//
// The fake device: a stream is a FIFO of kernels and event markers; nothing in
// it completes until the test pops it (complete()).  It fails the run when
//   * a buffer is freed twice, freed while a caller holds it, or freed while a
//     kernel that names it is still in a FIFO;
//   * a kernel is enqueued on a buffer that is not allocated;
//   * a k_fixup32 does not directly follow its own k_contig32 in its FIFO, or
//     a k_contig32 follows a k_contig32.
// The per-thread stream handle (value 2) is a FIFO of its own in every thread.
//
//   fixup_registry_check shared      8 threads x 2,000 cycles, one stream key
//   fixup_registry_check perthread   the same on the per-thread handle
//   fixup_registry_check growth      one thread's requests grow, 7 share its key
//   fixup_registry_check finalize    one thread finalizes while 7 cycle
//   fixup_registry_check prune       10,000 keys one after another
//   fixup_registry_check allocfail   the Nth allocation fails, N = 1 .. 8
//   fixup_registry_check all
#include "redop_fixup.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <condition_variable>
#include <deque>
#include <map>
#include <set>
#include <thread>

using namespace mpix;

static std::atomic<int> fails{0};

#define CHECK(cond, ...)                                                                          \
    do {                                                                                          \
        if (!(cond)) {                                                                            \
            if (++fails <= 20) {                                                                  \
                printf("FAIL %s: ", #cond);                                                       \
                printf(__VA_ARGS__);                                                              \
                printf("\n");                                                                     \
            }                                                                                     \
        }                                                                                         \
    } while (0)

constexpr uintptr_t kPerThread = 2;

struct Fake {
    struct Buf {
        size_t bytes;
        int held = 0;       // callers between acquire and release
        long queued = 0;    // kernels in a FIFO that name it
    };
    struct Item {
        int kind;           // 0 k_contig32, 1 k_fixup32, 2 event marker
        uintptr_t what;     // the buffer, or the event
        uint64_t call;
    };
    struct Stream {
        std::deque<Item> fifo;
        int last_kind = 1;  // of the last kernel enqueued
        uintptr_t last_buf = 0;
        uint64_t last_call = 0;
        long pairs = 0;
    };
    using StreamId = std::pair<uintptr_t, uintptr_t>;

    std::mutex mu;
    std::condition_variable cv;
    std::map<uintptr_t, Buf> bufs;              // live ones
    std::set<uintptr_t> freed;
    std::map<StreamId, Stream> streams;
    std::map<uintptr_t, long> events;           // live ones: markers still in a FIFO
    uintptr_t next_buf = 0x10000, next_ev = 1;
    long allocs = 0, frees = 0, fail_at = 0, max_live = 0, ev_made = 0, ev_dropped = 0;

    static StreamId id(uintptr_t stream)
    {
        return {stream, stream == kPerThread ? fixup_thread_token() : 0};
    }

    // ---- the registry's operations
    void *alloc(int, size_t bytes)
    {
        std::lock_guard<std::mutex> l(mu);
        if (++allocs == fail_at)
            return nullptr;
        const uintptr_t p = next_buf += 0x100;
        bufs[p].bytes = bytes;
        max_live = std::max<long>(max_live, (long) bufs.size());
        return (void *) p;
    }
    void free(int, void *ptr)
    {
        std::lock_guard<std::mutex> l(mu);
        const uintptr_t p = (uintptr_t) ptr;
        CHECK(!freed.count(p), "buffer %#lx freed twice", (unsigned long) p);
        auto it = bufs.find(p);
        CHECK(it != bufs.end(), "buffer %#lx freed, never allocated", (unsigned long) p);
        if (it == bufs.end())
            return;
        CHECK(it->second.held == 0, "buffer %#lx freed while held", (unsigned long) p);
        CHECK(it->second.queued == 0, "buffer %#lx freed with %ld kernels queued", (unsigned long) p,
              it->second.queued);
        bufs.erase(it);
        freed.insert(p);
        ++frees;
    }
    void *record(int, uintptr_t stream, void *ev)
    {
        std::lock_guard<std::mutex> l(mu);
        uintptr_t e = (uintptr_t) ev;
        if (!e) {
            e = next_ev++;
            events[e] = 0;
            ++ev_made;
        }
        CHECK(events.count(e), "event %lu recorded after its drop", (unsigned long) e);
        ++events[e];
        streams[id(stream)].fifo.push_back(Item{2, e, 0});
        return (void *) e;
    }
    bool done(void *ev)
    {
        std::lock_guard<std::mutex> l(mu);
        auto it = events.find((uintptr_t) ev);
        CHECK(it != events.end(), "query of a dropped event");
        return it != events.end() && it->second == 0;
    }
    bool wait(void *ev)
    {
        std::unique_lock<std::mutex> l(mu);
        auto it = events.find((uintptr_t) ev);
        CHECK(it != events.end(), "wait for a dropped event");
        if (it == events.end())
            return false;
        cv.wait(l, [&] { return events[(uintptr_t) ev] == 0; });
        return true;
    }
    void drop(int, void *ev)
    {
        std::lock_guard<std::mutex> l(mu);
        CHECK(events.erase((uintptr_t) ev) == 1, "event dropped twice");
        ++ev_dropped;
    }
    bool sync(int, uintptr_t)
    {
        CHECK(false, "stream synchronised (no event failed)");
        return false;
    }

    // ---- the test's side
    void hold(void *ptr, size_t want, int d)
    {
        std::lock_guard<std::mutex> l(mu);
        auto it = bufs.find((uintptr_t) ptr);
        CHECK(it != bufs.end(), "a lease on a buffer that is not allocated");
        if (it == bufs.end())
            return;
        CHECK(it->second.bytes >= want, "buffer of %zu bytes for a request of %zu",
              it->second.bytes, want);
        it->second.held += d;
    }
    void enqueue(uintptr_t stream, int kind, void *ptr, uint64_t call)
    {
        std::lock_guard<std::mutex> l(mu);
        const uintptr_t p = (uintptr_t) ptr;
        auto it = bufs.find(p);
        CHECK(it != bufs.end(), "kernel enqueued on a freed buffer");
        if (it == bufs.end())
            return;
        Stream &s = streams[id(stream)];
        if (kind == 0) {
            CHECK(s.last_kind == 1, "k_contig32 of call %llu follows the k_contig32 of call %llu",
                  (unsigned long long) call, (unsigned long long) s.last_call);
        } else {
            CHECK(s.last_kind == 0 && s.last_call == call && s.last_buf == p,
                  "k_fixup32 of call %llu follows kind %d of call %llu", (unsigned long long) call,
                  s.last_kind, (unsigned long long) s.last_call);
            ++s.pairs;
        }
        s.last_kind = kind;
        s.last_call = call;
        s.last_buf = p;
        ++it->second.queued;
        s.fifo.push_back(Item{kind, p, call});
    }
    // pops up to n items of every FIFO (n < 0: all of them)
    void complete(long n)
    {
        std::lock_guard<std::mutex> l(mu);
        for (auto &kv : streams) {
            std::deque<Item> &f = kv.second.fifo;
            for (long i = 0; !f.empty() && (n < 0 || i < n); ++i) {
                const Item it = f.front();
                f.pop_front();
                if (it.kind == 2) {
                    auto e = events.find(it.what);
                    if (e != events.end())      // (a dropped event's marker: nothing to mark)
                        --e->second;
                } else {
                    auto b = bufs.find(it.what);
                    CHECK(b != bufs.end(), "a kernel ran on a freed buffer");
                    if (b != bufs.end())
                        --b->second.queued;
                }
            }
        }
        cv.notify_all();
    }
    long pairs()
    {
        std::lock_guard<std::mutex> l(mu);
        long n = 0;
        for (auto &kv : streams)
            n += kv.second.pairs;
        return n;
    }
    size_t live()
    {
        std::lock_guard<std::mutex> l(mu);
        return bufs.size();
    }
};

struct FakeOps {
    Fake *f;
    void *alloc(int d, size_t b) { return f->alloc(d, b); }
    void free(int d, void *p) { f->free(d, p); }
    void *record(int d, uintptr_t s, void *e) { return f->record(d, s, e); }
    bool done(void *e) { return f->done(e); }
    bool wait(void *e) { return f->wait(e); }
    void drop(int d, void *e) { f->drop(d, e); }
    bool sync(int d, uintptr_t s) { return f->sync(d, s); }
};
using Reg = FixupRegistry<FakeOps>;

static std::atomic<uint64_t> g_call{0};

// one call of a split combiner: acquire, both kernels, release
static void *cycle(Reg &reg, Fake &fake, uintptr_t stream, size_t bytes, bool may_fail = false)
{
    const FixupKey key{0, stream, stream == kPerThread ? fixup_thread_token() : 0};
    const Reg::Lease l = reg.acquire(key, bytes);
    if (!l.ptr) {
        CHECK(may_fail, "acquire of %zu bytes failed", bytes);
        CHECK(l.entry == nullptr, "a failed acquire left a lease");
        return nullptr;
    }
    const uint64_t call = ++g_call;
    fake.hold(l.ptr, bytes, +1);
    fake.enqueue(stream, 0, l.ptr, call);
    std::this_thread::yield();
    fake.enqueue(stream, 1, l.ptr, call);
    fake.hold(l.ptr, bytes, -1);
    reg.release(l);
    return l.ptr;
}

// drains everything, finalizes, and nothing may be left
static void settle(Reg &reg, Fake &fake, const char *what)
{
    fake.complete(-1);
    reg.finalize();
    CHECK(fake.live() == 0, "%s: %zu buffers left after finalize", what, fake.live());
    CHECK(fake.allocs - (fake.fail_at && fake.allocs >= fake.fail_at ? 1 : 0) == fake.frees,
          "%s: %ld allocations, %ld frees", what, fake.allocs, fake.frees);
    CHECK(fake.ev_made == fake.ev_dropped, "%s: %ld events made, %ld dropped", what, fake.ev_made,
          fake.ev_dropped);
    CHECK(reg.entries() == 0, "%s: %zu entries left", what, reg.entries());
}

// a thread that completes a few items of every FIFO at a time until told to stop
struct Completer {
    Fake &fake;
    std::atomic<bool> stop{false};
    std::thread th;
    explicit Completer(Fake &f) : fake(f), th([this] {
        while (!stop.load()) {
            fake.complete(3);
            std::this_thread::yield();
        }
    }) {}
    ~Completer()
    {
        stop = true;
        th.join();
    }
};

constexpr int kThreads = 8, kCycles = 2000;

static void shared_or_perthread(bool per_thread)
{
    Fake fake;
    Reg reg(FakeOps{&fake});
    const uintptr_t stream = per_thread ? kPerThread : 0x7000;
    std::vector<void *> first(kThreads, nullptr);
    {
        Completer c(fake);
        std::vector<std::thread> ts;
        for (int t = 0; t < kThreads; ++t)
            ts.emplace_back([&, t] {
                for (int i = 0; i < kCycles; ++i) {
                    void *p = cycle(reg, fake, stream, 8 * (size_t) (1 + (i * 7 + t) % 5000));
                    if (i == 0)
                        first[t] = p;
                    else
                        CHECK(p == first[t], "thread %d: another buffer at cycle %d", t, i);
                }
            });
        for (auto &t : ts)
            t.join();
    }
    const std::set<void *> distinct(first.begin(), first.end());
    CHECK(distinct.size() == (per_thread ? (size_t) kThreads : 1u), "%zu distinct buffers",
          distinct.size());
    CHECK(fake.pairs() == (long) kThreads * kCycles, "%ld pairs", fake.pairs());
    CHECK(fake.streams.size() == (per_thread ? (size_t) kThreads : 1u), "%zu FIFOs",
          fake.streams.size());
    settle(reg, fake, per_thread ? "perthread" : "shared");
}

// thread 0 alternates small requests and ever larger ones (a buffer never
// shrinks, so each large one regrows it); with_finalize: thread 1 calls
// finalize over and over instead of cycling
static void growth(bool with_finalize)
{
    Fake fake;
    Reg reg(FakeOps{&fake});
    const uintptr_t stream = 0x7100;
    std::atomic<int> cyclers{0};
    long finalizes = 0;
    {
        Completer c(fake);
        std::vector<std::thread> ts;
        for (int t = 0; t < kThreads; ++t)
            ts.emplace_back([&, t] {
                if (with_finalize && t == 1) {
                    while (cyclers.load() < kThreads - 1 || finalizes < 50) {
                        reg.finalize();
                        ++finalizes;
                        std::this_thread::yield();
                    }
                    return;
                }
                for (int i = 0; i < kCycles; ++i) {
                    size_t bytes = 8 * (size_t) (1 + i % 100);
                    if (t == 0 && (i & 1))
                        bytes = kFixupMinBytes + 4096 * (size_t) i;
                    // (with finalize, a second stream too: entries nobody holds)
                    cycle(reg, fake, with_finalize && (i % 3 == 0) ? stream + 1 + t : stream, bytes);
                }
                ++cyclers;
            });
        for (auto &t : ts)
            t.join();
        // the cyclers go on working after the last finalize
        for (int i = 0; i < 10; ++i)
            cycle(reg, fake, stream, 64);
    }
    if (!with_finalize)
        CHECK(fake.allocs >= kCycles / 2, "%ld allocations: the buffer did not regrow", fake.allocs);
    else
        CHECK(fake.frees > 0, "no finalize freed anything (%ld finalizes)", finalizes);
    settle(reg, fake, with_finalize ? "finalize" : "growth");
}

static void prune()
{
    Fake fake;
    Reg reg(FakeOps{&fake});
    for (uintptr_t k = 0; k < 10000; ++k) {
        cycle(reg, fake, 0x100000 + 16 * k, 512);
        fake.complete(-1);
        CHECK(fake.live() <= kFixupMaxIdle, "%zu buffers live at key %lu", fake.live(),
              (unsigned long) k);
    }
    CHECK(fake.max_live <= (long) kFixupMaxIdle, "%ld buffers live at once", fake.max_live);
    CHECK(fake.frees >= 10000 - (long) kFixupMaxIdle, "%ld frees", fake.frees);
    // keys whose work stays pending are not pruned: nothing is freed early
    // (the fake checks), and all of it goes once the work completes
    for (uintptr_t k = 0; k < 100; ++k)
        cycle(reg, fake, 0x900000 + 16 * k, 512);
    CHECK(fake.live() >= 100, "pending buffers were freed: %zu live", fake.live());
    fake.complete(-1);
    cycle(reg, fake, 0xa00000, 512);
    CHECK(fake.live() <= kFixupMaxIdle, "%zu buffers live after the work completed", fake.live());
    settle(reg, fake, "prune");
}

static void allocfail()
{
    for (long n = 1; n <= 8; ++n) {
        Fake fake;
        fake.fail_at = n;
        Reg reg(FakeOps{&fake});
        long failed = 0;
        // allocations: a new key, its growth (work pending), a second key,
        // growth again after completion, ...
        const size_t sizes[] = {64, kFixupMinBytes + 8, 64, 2 * kFixupMinBytes, 4 * kFixupMinBytes};
        for (int round = 0; round < 2; ++round)
            for (uintptr_t s = 0; s < 2; ++s)
                for (size_t b : sizes) {
                    const long before = fake.allocs;
                    void *p = cycle(reg, fake, 0x7200 + 16 * s, b << round, true);
                    const bool hit = fake.allocs == n && before == n - 1;
                    CHECK((p == nullptr) == hit, "N = %ld: acquire %s", n,
                          p ? "succeeded on the failing allocation" : "failed");
                    failed += !p;
                    if (s)
                        fake.complete(-1);
                }
        CHECK(failed == 1, "N = %ld: %ld acquires failed", n, failed);
        settle(reg, fake, "allocfail");
    }
}

int main(int argc, char **argv)
{
    const char *mode = argc > 1 ? argv[1] : "all";
    const bool all = !strcmp(mode, "all");
    bool ran = false;
    if (all || !strcmp(mode, "shared"))
        shared_or_perthread(false), ran = true;
    if (all || !strcmp(mode, "perthread"))
        shared_or_perthread(true), ran = true;
    if (all || !strcmp(mode, "growth"))
        growth(false), ran = true;
    if (all || !strcmp(mode, "finalize"))
        growth(true), ran = true;
    if (all || !strcmp(mode, "prune"))
        prune(), ran = true;
    if (all || !strcmp(mode, "allocfail"))
        allocfail(), ran = true;
    if (!ran) {
        fprintf(stderr, "unknown mode %s\n", mode);
        return 2;
    }
    if (fails.load()) {
        printf("fixup registry %s: %d failures\n", mode, fails.load());
        return 1;
    }
    printf("fixup registry %s: ok\n", mode);
    return 0;
}
