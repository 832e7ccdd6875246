// redop_hostpath.h -- the host-resident operands' pure host logic: which
// form a synchronous call takes (host_route), the wave form's chunk schedule
// and worker slices, the workers' threads, barrier, first error and step
// trace.  No HIP: redop_capi.cpp is the only user in the library, and
// tests/c/hostpath_check.cpp builds it alone with g++ (tests/test_hostpath.py).
#pragma once

#include <immintrin.h>
#include <pthread.h>
#include <sched.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>
#include <vector>

namespace mpix {
namespace {     // internal to the unit that includes it: the library exports none of it

enum class Place { Device, Pinned, Pageable };

// The forms of the synchronous MPIX_Reduce_local, in the order they are
// tried.  Bounce, Wave and Worker may answer -1 (buffers not to be had, or
// the worker set busy): host_route(..., that route) gives the next one.
enum class Route { None = -1, PeerStaged, PeerEqual, Bounce, EqualWhole, Wave, Worker, Staged, Direct };

struct HostCall {
    Place in, io;
    bool no_peer;       // both on devices, two of them, without peer access
    uint64_t bytes;     // per operand
    bool equal;         // MPIX_EQUAL
    // MPIX_REDOP_PINNED, _BOUNCE_BYTES, _PAGEABLE_THREADS, _PAGEABLE_MODE, _PAGEABLE_CHUNK
    bool zero_copy;
    uint64_t bounce_bytes;
    int threads;
    bool wave;
    uint64_t chunk;
};

// in_host / io_host: the form copies that operand itself and takes the
// caller's pointer; the other is handed over as the device sees it.
// zero_copy (Direct only): the kernel reads page-locked host memory.
struct HostRoute {
    Route route;
    bool in_host, io_host, zero_copy;
};

inline HostRoute host_route(const HostCall &c, Route declined = Route::None)
{
    const bool in_pg = c.in == Place::Pageable, io_pg = c.io == Place::Pageable;
    const bool in_stage = in_pg || (c.in == Place::Pinned && !c.zero_copy);
    const bool io_stage = io_pg || (c.io == Place::Pinned && !c.zero_copy);
    // operands on two devices without peer access: the kernel runs where
    // inout lives and `in` is copied over in chunks (hipMemcpyPeerAsync);
    // MPIX_EQUAL's one header covers the whole message: copied whole
    if (c.no_peer)
        return {c.equal ? Route::PeerEqual : Route::PeerStaged, false, false, false};
    // only pageable operands bounce; pinned ones are used through their mapping
    if (declined < Route::Bounce && (in_pg || io_pg) && c.bytes <= c.bounce_bytes)
        return {Route::Bounce, in_pg, io_pg, false};
    // MPIX_EQUAL is one comparison over the whole buffer behind one 8-byte
    // header (opequal.c:20-35; MPIR_Reduce_equal: "we can't split the
    // message"), so it is never chunked
    if (c.equal && (in_stage || io_stage))
        return {Route::EqualWhole, in_stage, io_stage, false};
    // pageable operands through the workers' pinned buffers; a pinned
    // operand is used through its device mapping
    if (declined < Route::Wave && (in_pg || io_pg) && c.zero_copy && c.threads > 0 &&
        c.bytes >= (c.wave ? 2 : 2 * (uint64_t) c.threads) * c.chunk)
        return {c.wave ? Route::Wave : Route::Worker, in_pg, io_pg, false};
    if (in_stage || io_stage)
        return {Route::Staged, in_stage, io_stage, false};
    return {Route::Direct, false, false, c.in == Place::Pinned || c.io == Place::Pinned};
}

// The wave's chunks, (offset, count) in elements: chunk sizes ramp up
// (chunk/8, /4, /2) so the first kernel starts after a short copy-in, and down
// again at the end so the last copy-out is short; full chunks in between.
struct Chunk {
    uint64_t off, count;    // in elements
};
inline std::vector<Chunk> wave_chunks(uint64_t count, uint64_t chunk)
{
    std::vector<Chunk> chunks;
    uint64_t off = 0;
    for (int r = 3; r >= 1 && off < count; --r) {
        const uint64_t c = std::max<uint64_t>(chunk >> r, 1);
        const uint64_t m = std::min(c, count - off);
        chunks.push_back(Chunk{off, m});
        off += m;
    }
    const uint64_t tail_split = chunk;      // the last full chunk's worth goes in halves
    while (count - off > chunk + tail_split) {
        chunks.push_back(Chunk{off, chunk});
        off += chunk;
    }
    for (int r = 1; off < count; r = r < 3 ? r + 1 : 3) {
        const uint64_t c = std::max<uint64_t>(chunk >> r, 1);
        const uint64_t m = (count - off <= c || r == 3) ? std::min(count - off, chunk) : c;
        chunks.push_back(Chunk{off, m});
        off += m;
    }
    return chunks;
}

// worker w of W's slice of a chunk of `bytes`: 4 KiB-aligned parts
inline void slice(int w, int W, size_t bytes, size_t *lo, size_t *len)
{
    size_t per = ((bytes + (size_t) W - 1) / (size_t) W + 4095) & ~(size_t) 4095;
    *lo = std::min(bytes, per * (size_t) w);
    *len = std::min(bytes - *lo, per);
}

// Host workers for one pageable call: the configured count, at most one per
// CPU this process may run on (more would only take turns on the same cores).
inline int worker_count(int nthreads)
{
    int w = nthreads < 1 ? 1 : nthreads;
    cpu_set_t mine;
    if (sched_getaffinity(0, sizeof mine, &mine) == 0) {
        const int cpus = CPU_COUNT(&mine);
        if (cpus >= 1 && w > cpus)
            w = cpus;
    }
    return w;
}

// a sysfs cpulist ("a-b,c", as in local_cpulist) or an explicit one
inline std::vector<int> parse_cpulist(const char *txt)
{
    std::vector<int> out;
    for (const char *p = txt; *p;) {
        char *e;
        long a = strtol(p, &e, 10);
        if (e == p)
            break;
        long b = a;
        p = e;
        if (*p == '-') {
            b = strtol(p + 1, &e, 10);
            p = e;
        }
        for (long c = a; c <= b && c < 4096; ++c)
            out.push_back((int) c);
        while (*p == ',' || *p == ' ' || *p == '\n')
            ++p;
    }
    return out;
}

// work(0) on the caller (its affinity is its own), work(1 .. W-1) on threads
// of their own, pinned round-robin to `cpus` when it is not empty; joined.
template <class F>
void run_workers(int W, const std::vector<int> &cpus, F work)
{
    std::vector<std::thread> pool;
    pool.reserve(W > 0 ? (size_t) W - 1 : 0);
    for (int w = 1; w < W; ++w)
        pool.emplace_back([&, w]() {
            if (!cpus.empty()) {
                cpu_set_t set;
                CPU_ZERO(&set);
                CPU_SET(cpus[(size_t) w % cpus.size()], &set);
                (void) pthread_setaffinity_np(pthread_self(), sizeof set, &set);
            }
            work(w);
        });
    work(0);
    for (std::thread &t : pool)
        t.join();
}

// The first non-zero code any worker reports (fail(0) reports nothing).
struct FirstError {
    std::atomic<int> rc{0};
    void fail(int e)
    {
        int z = 0;
        rc.compare_exchange_strong(z, e);
    }
    bool ok() const { return rc.load() == 0; }
};

// Barrier of the wave workers (sense reversal).  A waiter spins with `pause`
// for up to kSpinNs, then sleeps on a futex on the generation word until the
// last worker arrives and wakes it.  Not a yield loop: a yielding waiter on a
// CPU shared with other runnable tasks can be left off it for a whole
// scheduler slice, and every step waits for the last worker to leave -- one
// such stall took a 256 MiB call from 12.6 to 21 ms
// (profiles/r04_pageable_swing.json, the slowest trace's step 7).  Not a long
// spin either: with fewer cores than workers, spinning waiters
// would keep the worker they wait for off the core.  The steps' own imbalance
// is well under the spin window, so a balanced wave never sleeps.
struct SpinBarrier {
    static constexpr int64_t kSpinNs = 200000;
    std::atomic<int> left;
    std::atomic<int> gen{0};
    std::atomic<int> sleepers{0};
    const int n;
    explicit SpinBarrier(int n_) : left(n_), n(n_) {}
    void wait()
    {
        const int g = gen.load();
        if (left.fetch_sub(1) == 1) {
            left.store(n);
            gen.fetch_add(1);           // seq_cst: ordered before the sleepers check
            if (sleepers.load() > 0)
                syscall(SYS_futex, reinterpret_cast<int *>(&gen), FUTEX_WAKE_PRIVATE, INT32_MAX,
                        nullptr, nullptr, 0);
            return;
        }
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t spins = 1; gen.load(std::memory_order_acquire) == g; ++spins) {
            _mm_pause();
            if ((spins & 0xff) == 0 &&
                std::chrono::steady_clock::now() - t0 > std::chrono::nanoseconds(kSpinNs))
                break;
        }
        if (gen.load() != g)
            return;
        sleepers.fetch_add(1);          // seq_cst: the releaser sees it, or we see its gen
        while (gen.load() == g)
            syscall(SYS_futex, reinterpret_cast<int *>(&gen), FUTEX_WAIT_PRIVATE, g, nullptr,
                    nullptr, 0);
        sleepers.fetch_sub(1);
    }
};

// MPIX_REDOP_PIPE_TRACE=1: `rows` x 5 host times in ns from the call's start
// (-1: never marked), printed by the form as the last member of its one JSON
// line on stderr.  Off, it holds nothing and mark() does nothing.
struct StepTrace {
    const bool on;
    std::vector<int64_t> ns;
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit StepTrace(size_t rows) : on(enabled()), ns(on ? rows * 5 : 0, -1) {}
    static bool enabled()       // read once per process
    {
        static const bool e = getenv("MPIX_REDOP_PIPE_TRACE") != nullptr;
        return e;
    }
    void mark(size_t row, int what)
    {
        if (on)
            ns[row * 5 + (size_t) what] = std::chrono::duration_cast<std::chrono::nanoseconds>(
                                              std::chrono::steady_clock::now() - t0).count();
    }
    // ..."ns": [t,t,...]}} and the line's end
    void print_ns(FILE *f) const
    {
        fprintf(f, "\"ns\": [");
        for (size_t i = 0; i < ns.size(); ++i)
            fprintf(f, "%s%lld", i ? "," : "", (long long) ns[i]);
        fprintf(f, "]}}\n");
    }
};

}  // namespace
}  // namespace mpix
