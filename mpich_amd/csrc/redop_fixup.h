// redop_fixup.h -- the registry of the split combiners' fixup-word buffers
// (redop_kernels.h is_split: k_contig32 writes one 64-bit word per 64 units,
// k_fixup32 reads them in a second launch).  This is the one piece of host
// state two launches of the data path share, so it has rules of its own:
//
//   * A caller holds a Lease from acquire() until release(): it enqueues both
//     kernels in between.  Callers with the same key hold it one at a time,
//     so on one stream every k_contig32 is directly followed by its own
//     k_fixup32, and stream order then keeps the next pair off the words
//     until this pair is through with them.
//   * The key is (device, stream handle, thread token); the token is 0 except
//     for the per-thread stream handle, which names a different stream in
//     every thread: those get a buffer per calling thread.
//   * A buffer is passed to `free` only when nobody holds it and the event
//     recorded at its last release has completed.  Growth and finalize move
//     a buffer with work pending to a retired list, reaped (polled) by later
//     calls; finalize waits for the retired events -- events, never stream
//     handles, which may be destroyed by then -- and leaves held buffers to
//     their holders.
//   * Retained buffers are bounded: when a new key would make more than
//     kFixupMaxIdle entries, idle ones (not held, no work pending) are freed,
//     least recently used first.  So at most kFixupMaxIdle buffers idle, plus
//     one per stream that has work of ours pending or a caller inside.
//
// No HIP: the device operations are injected (redop_capi.cpp supplies the HIP
// ones, tests/c/fixup_registry_check.cpp a fake device;
// tests/test_fixup_registry.py builds that with g++ alone).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <mutex>
#include <vector>

namespace mpix {

constexpr size_t kFixupMinBytes = (size_t) 64 << 10;   // 524,288 units
constexpr size_t kFixupMaxIdle = 32;

// a token no other thread of the process has or will have (thread ids are reused)
inline uintptr_t fixup_thread_token()
{
    static std::atomic<uintptr_t> next{1};
    thread_local uintptr_t mine = next.fetch_add(1, std::memory_order_relaxed);
    return mine;
}

struct FixupKey {
    int dev;
    uintptr_t stream;
    uintptr_t thread;   // fixup_thread_token() for the per-thread handle, else 0
    bool operator==(const FixupKey &o) const
    {
        return dev == o.dev && stream == o.stream && thread == o.thread;
    }
};

// Ops:  void *alloc(int dev, size_t bytes)         nullptr: none to be had
//       void free(int dev, void *p)
//       void *record(int dev, uintptr_t stream, void *ev)
//             an event after everything enqueued on `stream` so far: `ev`
//             recorded again, or (ev == nullptr) a new one; nullptr on failure
//       bool done(void *ev)                         true only when known complete
//       bool wait(void *ev)                         blocks; false: not known complete
//       void drop(int dev, void *ev)                destroys the event
//       bool sync(int dev, uintptr_t stream)        a stream the caller just used
template <class Ops>
class FixupRegistry
{
    struct Entry {
        FixupKey key;
        void *ptr = nullptr;
        size_t bytes = 0;
        void *ev = nullptr;     // recorded at the last release; nullptr: nothing pending
        int users = 0;          // leases out or waited for (under mu_)
        uint64_t used = 0;      // tick of the last release (under mu_)
        std::mutex hold;        // from acquire to release
    };
    struct Retired {
        int dev;
        void *ptr;
        void *ev;               // never nullptr
    };

  public:
    struct Lease {
        void *ptr = nullptr;    // nullptr: acquire failed, nothing to release
        void *entry = nullptr;
    };

    explicit FixupRegistry(Ops ops) : ops_(ops) {}

    Lease acquire(const FixupKey &key, size_t bytes)
    {
        std::vector<Retired> dead;
        Entry *e = nullptr;
        {
            std::lock_guard<std::mutex> l(mu_);
            reap(dead);
            for (Entry *x : entries_)
                if (x->key == key)
                    e = x;
            if (!e) {
                if (entries_.size() >= kFixupMaxIdle)
                    prune(dead);
                e = new Entry;
                e->key = key;
                entries_.push_back(e);
            }
            ++e->users;
        }
        destroy(dead);
        e->hold.lock();
        if (e->bytes >= bytes)
            return Lease{e->ptr, e};
        const size_t want = bytes < kFixupMinBytes ? kFixupMinBytes : bytes;
        void *p = ops_.alloc(key.dev, want);
        if (!p) {               // the smaller buffer stays as it is
            e->hold.unlock();
            std::lock_guard<std::mutex> l(mu_);
            --e->users;
            return Lease{};
        }
        if (e->ptr) {
            // enqueued kernels may still name the old buffer: it goes with
            // the event of its last release
            if (e->ev) {
                std::lock_guard<std::mutex> l(mu_);
                retired_.push_back(Retired{key.dev, e->ptr, e->ev});
                e->ev = nullptr;
            } else {
                ops_.free(key.dev, e->ptr);
            }
        }
        e->ptr = p;
        e->bytes = want;
        return Lease{p, e};
    }

    // after both kernels are enqueued on the key's stream (or none, on an error)
    void release(const Lease &lease)
    {
        Entry *e = static_cast<Entry *>(lease.entry);
        if (!e)
            return;
        void *ev = ops_.record(e->key.dev, e->key.stream, e->ev);
        if (!ev) {
            // no event to be had: wait here, so that nothing is pending
            const bool idle = ops_.sync(e->key.dev, e->key.stream);
            if (e->ev && idle) {
                ops_.drop(e->key.dev, e->ev);
                e->ev = nullptr;
            }
            // (not known idle: the old event stays and says "pending" for good,
            // the buffer is then never freed -- a leak, not a use after free)
        } else {
            e->ev = ev;
        }
        e->hold.unlock();
        std::vector<Retired> dead;
        {
            std::lock_guard<std::mutex> l(mu_);
            --e->users;
            e->used = ++tick_;
            reap(dead);
        }
        destroy(dead);
    }

    // Frees what is idle, waits for the retired buffers' events and frees
    // those; an entry a caller holds or waits for stays with that caller.
    void finalize()
    {
        std::vector<Retired> dead, pending;
        {
            std::lock_guard<std::mutex> l(mu_);
            std::vector<Entry *> keep;
            for (Entry *e : entries_) {
                if (e->users) {
                    keep.push_back(e);
                    continue;
                }
                if (e->ptr && e->ev && !ops_.done(e->ev))
                    pending.push_back(Retired{e->key.dev, e->ptr, e->ev});
                else if (e->ptr || e->ev)
                    dead.push_back(Retired{e->key.dev, e->ptr, e->ev});
                delete e;
            }
            entries_.swap(keep);
            pending.insert(pending.end(), retired_.begin(), retired_.end());
            retired_.clear();
        }
        destroy(dead);
        for (Retired &r : pending) {
            if (ops_.wait(r.ev)) {
                ops_.drop(r.dev, r.ev);
                ops_.free(r.dev, r.ptr);
            } else {            // not known complete: back on the list
                std::lock_guard<std::mutex> l(mu_);
                retired_.push_back(r);
            }
        }
    }

    size_t entries()
    {
        std::lock_guard<std::mutex> l(mu_);
        return entries_.size();
    }

  private:
    // under mu_: retired buffers whose event has completed
    void reap(std::vector<Retired> &dead)
    {
        size_t k = 0;
        for (Retired &r : retired_) {
            if (ops_.done(r.ev))
                dead.push_back(r);
            else
                retired_[k++] = r;
        }
        retired_.resize(k);
    }

    // under mu_: idle entries, least recently used first, until a new one fits
    void prune(std::vector<Retired> &dead)
    {
        while (entries_.size() >= kFixupMaxIdle) {
            size_t best = entries_.size();
            for (size_t i = 0; i < entries_.size(); ++i) {
                Entry *e = entries_[i];
                if (e->users || (e->ev && !ops_.done(e->ev)))
                    continue;
                if (best == entries_.size() || e->used < entries_[best]->used)
                    best = i;
            }
            if (best == entries_.size())
                return;         // every one held or pending
            Entry *e = entries_[best];
            if (e->ptr || e->ev)
                dead.push_back(Retired{e->key.dev, e->ptr, e->ev});
            delete e;
            entries_.erase(entries_.begin() + (long) best);
        }
    }

    // outside mu_ (a device free may wait for the device)
    void destroy(std::vector<Retired> &dead)
    {
        for (Retired &r : dead) {
            if (r.ev)
                ops_.drop(r.dev, r.ev);
            if (r.ptr)
                ops_.free(r.dev, r.ptr);
        }
        dead.clear();
    }

    Ops ops_;
    std::mutex mu_;
    std::vector<Entry *> entries_;
    std::vector<Retired> retired_;
    uint64_t tick_ = 0;
};

}  // namespace mpix
