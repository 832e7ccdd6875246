// Host-only check of mpich_amd/csrc/redop_hostpath.h, the one header it
// includes.  Built with g++ by tests/test_hostpath.py (once more with
// -fsanitize=thread for `workers`).
//   hostpath_check props     wave_chunks' properties and goldens, slice, parse_cpulist
//   hostpath_check workers   SpinBarrier under run_workers
//   hostpath_check chunks    stdin "count chunk" lines -> the chunk list of each
//   hostpath_check routes    stdin "in io no_peer equal zc threads wave bytes bounce chunk"
//                            lines -> the chain of forms of each, every form that can
//                            answer -1 taken to do so (tests/golden/make_host_routes.py)
#include "redop_hostpath.h"

#include <string.h>

#include <random>
#include <string>

using namespace mpix;

static int fails = 0;

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

static std::string chunk_list(uint64_t count, uint64_t chunk)
{
    std::string s;
    for (const auto &c : wave_chunks(count, chunk))
        s += (s.empty() ? "" : ",") + std::to_string(c.count);
    return s;
}

// the chunks tile [0, count) in order, none empty, none above `chunk` (a ring half)
static void check_chunks(uint64_t count, uint64_t chunk)
{
    uint64_t off = 0;
    for (const auto &c : wave_chunks(count, chunk)) {
        CHECK(c.off == off && c.count >= 1 && c.count <= chunk, "count %llu chunk %llu at %llu",
              (unsigned long long) count, (unsigned long long) chunk, (unsigned long long) off);
        off += c.count;
    }
    CHECK(off == count, "count %llu chunk %llu covered %llu", (unsigned long long) count,
          (unsigned long long) chunk, (unsigned long long) off);
}

static int props()
{
    const uint64_t chunks[] = {1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 1000, 16384, (1ull << 24) + 3};
    std::mt19937_64 rng(0x5EED0002);
    long cases = 0;
    for (uint64_t chunk : chunks) {
        for (uint64_t count = 1; count <= 40 * std::min<uint64_t>(chunk, 64); ++count, ++cases)
            check_chunks(count, chunk);
        for (int i = 0; i < 300; ++i, ++cases)
            check_chunks(1 + rng() % (200 * chunk), chunk);
    }
    CHECK(chunk_list(165, 16) == "2,4,8,16,16,16,16,16,16,16,16,8,4,11", "%s",
          chunk_list(165, 16).c_str());
    CHECK(chunk_list(33, 16) == "2,4,8,8,4,7", "%s", chunk_list(33, 16).c_str());
    CHECK(chunk_list(5, 16) == "2,3", "%s", chunk_list(5, 16).c_str());

    // slice: disjoint, in order, covering [0, bytes), every lo on a 4 KiB boundary
    for (int W = 1; W <= 16; ++W)
        for (size_t bytes : {(size_t) 1, (size_t) 4095, (size_t) 4096, (size_t) 4097,
                             (size_t) 65536 * 1, (size_t) 65536 * 8, (size_t) 65536 * 12,
                             (size_t) 65536 * 32}) {
            size_t end = 0;
            for (int w = 0; w < W; ++w) {
                size_t lo, len;
                slice(w, W, bytes, &lo, &len);
                CHECK(lo % 4096 == 0 || (lo == bytes && len == 0), "W %d bytes %zu w %d lo %zu", W,
                      bytes, w, lo);
                CHECK(len == 0 || lo == end, "W %d bytes %zu w %d lo %zu after %zu", W, bytes, w,
                      lo, end);
                CHECK(lo + len <= bytes, "W %d bytes %zu w %d", W, bytes, w);
                if (len)
                    end = lo + len;
            }
            CHECK(end == bytes, "W %d bytes %zu covered %zu", W, bytes, end);
        }

    auto cpus = [](const char *txt) {
        std::string s;
        for (int c : parse_cpulist(txt))
            s += (s.empty() ? "" : ",") + std::to_string(c);
        return s;
    };
    CHECK(cpus("0-3,5") == "0,1,2,3,5", "%s", cpus("0-3,5").c_str());
    CHECK(parse_cpulist("64-127").size() == 64 && parse_cpulist("64-127").front() == 64 &&
              parse_cpulist("64-127").back() == 127, "64-127");
    CHECK(cpus("7") == "7", "%s", cpus("7").c_str());
    CHECK(cpus("") == "", "%s", cpus("").c_str());
    CHECK(cpus("3-1") == "", "%s", cpus("3-1").c_str());
    CHECK(cpus("0-1,8\n") == "0,1,8", "%s", cpus("0-1,8\n").c_str());
    CHECK(worker_count(0) == 1 && worker_count(1) == 1 && worker_count(16) <= 16, "worker_count");
    printf("wave_chunks cases: %ld\n", cases);
    return fails;
}

// W workers over `steps` steps: each adds one to the step's counter, meets
// the others, and must then read W there; the first error any worker reports
static int workers()
{
    const int steps = 2000;
    for (int W : {1, 2, 8}) {
        std::vector<std::atomic<int>> counter((size_t) steps);
        for (auto &c : counter)
            c.store(0);
        SpinBarrier bar(W);
        FirstError err;
        std::atomic<int> ran{0};
        run_workers(W, std::vector<int>(), [&](int w) {
            ran.fetch_add(1 << w);
            for (int s = 0; s < steps; ++s) {
                counter[(size_t) s].fetch_add(1, std::memory_order_relaxed);
                bar.wait();
                if (counter[(size_t) s].load(std::memory_order_relaxed) != W)
                    err.fail(100 + w);
            }
            err.fail(0);        // no error
            err.fail(8 + w);
        });
        CHECK(ran.load() == (1 << W) - 1, "W %d ran %x", W, ran.load());
        const int first = err.rc.load();
        err.fail(99);           // a later one does not replace it
        CHECK(first >= 8 && first < 8 + W && err.rc.load() == first && !err.ok(),
              "W %d first error %d then %d", W, first, err.rc.load());
    }
    // pinned to the CPUs this process may run on, round-robin
    cpu_set_t mine;
    std::vector<int> cpus;
    if (sched_getaffinity(0, sizeof mine, &mine) == 0)
        for (int c = 0; c < CPU_SETSIZE && cpus.size() < 2; ++c)
            if (CPU_ISSET(c, &mine))
                cpus.push_back(c);
    std::vector<int> on(4, -1);
    run_workers(4, cpus, [&](int w) { on[(size_t) w] = sched_getcpu(); });
    for (int w = 1; w < 4 && !cpus.empty(); ++w)
        CHECK(on[(size_t) w] == cpus[(size_t) w % cpus.size()], "worker %d on cpu %d", w,
              on[(size_t) w]);
    return fails;
}

static const char *step_code(Route r)
{
    switch (r) {
        case Route::PeerStaged: return "PS";
        case Route::PeerEqual: return "PE";
        case Route::Bounce: return "B";
        case Route::EqualWhole: return "E";
        case Route::Wave: return "W";
        case Route::Worker: return "K";
        case Route::Staged: return "S";
        case Route::Direct: return "D";
        default: return "?";
    }
}

static int routes()
{
    int in, io, no_peer, equal, zc, threads, wave;
    unsigned long long bytes, bounce, chunk;
    while (scanf("%d %d %d %d %d %d %d %llu %llu %llu", &in, &io, &no_peer, &equal, &zc, &threads,
                 &wave, &bytes, &bounce, &chunk) == 10) {
        const HostCall c{(Place) in, (Place) io, no_peer != 0, bytes, equal != 0,
                         zc != 0, bounce, threads, wave != 0, chunk};
        Route declined = Route::None;
        for (int n = 0; n < 8; ++n) {
            const HostRoute r = host_route(c, declined);
            printf("%s%s%d%d%d", n ? ">" : "", step_code(r.route), r.in_host, r.io_host,
                   r.zero_copy);
            if (r.route != Route::Bounce && r.route != Route::Wave && r.route != Route::Worker)
                break;
            declined = r.route;
        }
        printf("\n");
    }
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "chunks") {
        unsigned long long count, chunk;
        while (scanf("%llu %llu", &count, &chunk) == 2)
            printf("%s\n", chunk_list(count, chunk).c_str());
        return 0;
    }
    if (mode == "routes")
        return routes();
    if (mode != "props" && mode != "workers")
        return 2;
    const int bad = mode == "props" ? props() : workers();
    printf("hostpath %s: %s\n", mode.c_str(), bad ? "FAIL" : "ok");
    return bad ? 1 : 0;
}
