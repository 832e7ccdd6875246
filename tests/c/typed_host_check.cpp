// typed_host_check.cpp -- the host side of the typed accumulate entries (the
// packed-order table built at plan creation, MPIX_Iov_plan_locate,
// MPIX_Iov_plan_info_packed and the launch entries' checks that need no device)
// under AddressSanitizer + UndefinedBehaviorSanitizer: built by
// mpich_amd/csrc/sanitize.mk against the sanitizer build of redop_capi.cpp, run
// on the CPU, nothing preloaded.  What _locate answers for every packed index
// is compared with a straightforward walk of the merged runs re-derived here.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "mpix_redop.h"

namespace {

int g_errors = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            ++g_errors;                                                    \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);     \
        }                                                                  \
    } while (0)

const MPIX_Datatype kDouble = 0x4c00080b, kFloat = 0x4c00040a, kInt16 = 0x4c000238,
                    kInt8 = 0x4c000137, kDoubleInt = (MPIX_Datatype) 0x8c000001;
const MPIX_Op kSum = 0x58000003, kBand = 0x58000006, kReplace = 0x5800000d, kNoOp = 0x5800000e;
enum { OK = 0, BUFFER = 1, COUNT = 2, TYPE = 3, OP = 9, ARG = 12 };

struct Run {
    int64_t off, n;
};

uint64_t g_seed = 0x5EED1200;
uint32_t rnd(uint32_t n)
{
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t) (g_seed >> 33) % n;
}

// the merged runs, restated: empty runs dropped, a run joins its predecessor
// in call order when it starts where that one ends
std::vector<Run> merge(const std::vector<Run> &in, int64_t ext)
{
    std::vector<Run> m;
    for (const Run &r : in) {
        if (r.n == 0)
            continue;
        if (!m.empty() && m.back().off + m.back().n * ext == r.off)
            m.back().n += r.n;
        else
            m.push_back(r);
    }
    return m;
}

// every packed index (or, of a long table, every run's first and last one, the
// indices around every multiple of 256 and a random sample) against the walk
void check_locate(const std::vector<Run> &runs, MPIX_Datatype dt, int64_t ext, bool every)
{
    std::vector<MPIX_Aint> offs, cnts;
    for (const Run &r : runs) {
        offs.push_back(r.off);
        cnts.push_back(r.n);
    }
    MPIX_Iov_plan p = nullptr;
    CHECK(MPIX_Iov_plan_create((MPIX_Aint) runs.size(), offs.data(), cnts.data(), dt, &p) == OK);
    if (!p)
        return;
    const std::vector<Run> m = merge(runs, ext);
    std::vector<int64_t> prefix(m.size() + 1, 0);
    for (size_t k = 0; k < m.size(); ++k)
        prefix[k + 1] = prefix[k] + m[k].n;
    const int64_t total = prefix[m.size()];
    MPIX_Aint elements = -1, nrun = -1, bytes = -1;
    CHECK(MPIX_Iov_plan_info(p, &elements, &nrun, nullptr, nullptr, nullptr, nullptr) == OK);
    CHECK(elements == total && nrun == (MPIX_Aint) m.size());
    CHECK(MPIX_Iov_plan_info_packed(p, &bytes) == OK);
    CHECK(bytes == (m.size() <= 1 ? 0
                                  : (MPIX_Aint) ((2 * m.size() + 1) * 8 +
                                                 ((total + 255) / 256 + 1) * 4)));
    auto want = [&](int64_t q) {
        const size_t s = std::upper_bound(prefix.begin(), prefix.end(), q) - prefix.begin() - 1;
        return m[s].off + (q - prefix[s]) * ext;
    };
    int bad = 0;
    auto one = [&](int64_t q) {
        if (q < 0 || q >= total)
            return;
        MPIX_Aint got = INT64_MIN;
        if (MPIX_Iov_plan_locate(p, q, &got) != OK || got != want(q))
            ++bad;
    };
    if (every) {
        for (int64_t q = 0; q < total; ++q)
            one(q);
    } else {
        for (size_t k = 0; k < m.size(); ++k) {
            one(prefix[k]);
            one(prefix[k + 1] - 1);
        }
        for (int64_t q = 0; q < total + 256; q += 256)
            for (int64_t d = -2; d <= 2; ++d)
                one(q + d);
        for (int k = 0; k < 20000 && total; ++k)
            one((int64_t) (((uint64_t) rnd(1u << 30) << 20 | rnd(1u << 20)) % (uint64_t) total));
    }
    CHECK(bad == 0);
    MPIX_Aint v = 77;
    CHECK(MPIX_Iov_plan_locate(p, -1, &v) == COUNT && MPIX_Redop_last_error() == COUNT);
    CHECK(MPIX_Iov_plan_locate(p, total, &v) == COUNT);
    CHECK(MPIX_Iov_plan_locate(p, INT64_MAX, &v) == COUNT);
    CHECK(MPIX_Iov_plan_locate(p, 0, nullptr) == ARG);
    CHECK(v == 77);
    CHECK(MPIX_Iov_plan_free(&p) == OK && p == nullptr);
}

void tables()
{
    check_locate({}, kDouble, 8, true);
    check_locate({{0, 0}, {64, 0}}, kDouble, 8, true);
    check_locate({{24, 700}}, kDouble, 8, true);
    check_locate({{24, 255}, {4000, 1}, {5000, 1}, {6004, 255}, {9000, 300}, {-800, 5}}, kDouble, 8,
                 true);
    // 10^5 runs of one element: strided (nothing merges), descending, and
    // every 7th one on the other residue (chains of 6 merge)
    const int N = 100000;
    std::vector<Run> r(N);
    for (int k = 0; k < N; ++k)
        r[k] = Run{16 * (int64_t) k - 8 * (int64_t) N, 1};
    check_locate(r, kDouble, 8, true);
    std::reverse(r.begin(), r.end());
    check_locate(r, kDouble, 8, true);
    for (int k = 0; k < N; ++k)
        r[k] = Run{8 * (int64_t) k + (k % 7 ? 0 : 8 * (int64_t) N + 4), 1};
    check_locate(r, kDouble, 8, true);
    // 10^5 long runs: 2.5 * 10^7 elements, sampled
    for (int k = 0; k < N; ++k)
        r[k] = Run{(int64_t) k * 4096 + 4 * (k & 1), 1 + (int64_t) rnd(500)};
    check_locate(r, kDouble, 8, false);
    // random tables: lengths 0..5 and up to 700, gaps of 0 (a merge) or more,
    // residues, negative offsets, shuffled order, three extents
    const struct {
        MPIX_Datatype dt;
        int64_t ext, step;
    } types[3] = {{kDouble, 8, 4}, {kInt16, 2, 2}, {kInt8, 1, 1}};
    for (int round = 0; round < 60; ++round) {
        const auto &t = types[round % 3];
        const int n = 1 + (int) rnd(round < 30 ? 40 : 3000);
        std::vector<Run> q;
        int64_t pos = -(int64_t) rnd(5000) * t.ext;
        for (int k = 0; k < n; ++k) {
            const int64_t len = rnd(4) ? rnd(6) : rnd(700);
            if (rnd(3))
                pos += (int64_t) rnd(4) * t.step;
            q.push_back(Run{pos, len});
            pos += len * t.ext;
        }
        if (round & 1)
            for (size_t k = q.size() - 1; k > 0; --k)
                std::swap(q[k], q[rnd((uint32_t) k + 1)]);
        check_locate(q, t.dt, t.ext, true);
    }
    // the padded pair's raw iov with a hole after element 20: two runs
    std::vector<MPIX_Aint> o, l;
    for (int k = 0; k < 37; ++k) {
        const MPIX_Aint at = 16 * k + (k > 20 ? 32 : 0);
        o.insert(o.end(), {at, at + 8});
        l.insert(l.end(), {8, 4});
    }
    MPIX_Iov_plan p = nullptr;
    CHECK(MPIX_Iov_plan_create_iovec(74, o.data(), l.data(), kDoubleInt, &p) == OK && p);
    for (int k = 0; k < 37; ++k) {
        MPIX_Aint got = -1;
        CHECK(MPIX_Iov_plan_locate(p, k, &got) == OK && got == 16 * k + (k > 20 ? 32 : 0));
    }
    CHECK(MPIX_Iov_plan_free(&p) == OK);
}

// the typed entries' checks that come before any device work, one per numbered
// check of mpix_redop.h, on pointers that are never dereferenced
void launch_errors()
{
    char *A = (char *) 0x100000, *B = (char *) 0x200000, *T = (char *) 0x300000;
    void *wild = (void *) -1;
    MPIX_Aint offs[2] = {96, -64}, cnts[2] = {4, 4}, cnts9[2] = {4, 5};
    MPIX_Iov_plan p = nullptr, pf = nullptr, p9 = nullptr, empty = nullptr;
    MPIX_Iov_plan junk = (MPIX_Iov_plan) (uintptr_t) 0xdead0;
    CHECK(MPIX_Iov_plan_create(2, offs, cnts, kDouble, &p) == OK);
    CHECK(MPIX_Iov_plan_create(2, offs, cnts, kFloat, &pf) == OK);
    CHECK(MPIX_Iov_plan_create(2, offs, cnts9, kDouble, &p9) == OK);
    CHECK(MPIX_Iov_plan_create(0, nullptr, nullptr, kDouble, &empty) == OK);
    // 1, 2
    CHECK(MPIX_Accumulate_local_typed_async(A, p, T, nullptr, kBand, nullptr) == ARG);
    CHECK(MPIX_Get_accumulate_local_typed(A, p, B, p, T, nullptr, kBand) == ARG);
    CHECK(MPIX_Accumulate_local_typed(nullptr, pf, nullptr, p, kBand) == OP);
    CHECK(MPIX_Get_accumulate_local_typed_async(wild, pf, wild, pf, wild, empty, kBand, nullptr) ==
          OP);
    // 3: type, then count, origin before result, before zero elements and buffers
    CHECK(MPIX_Accumulate_local_typed_async(nullptr, pf, nullptr, p, kSum, nullptr) == TYPE);
    CHECK(MPIX_Accumulate_local_typed(nullptr, p9, nullptr, p, kSum) == COUNT);
    CHECK(MPIX_Get_accumulate_local_typed(nullptr, p, nullptr, pf, nullptr, p, kSum) == TYPE);
    CHECK(MPIX_Get_accumulate_local_typed(nullptr, p9, nullptr, pf, nullptr, p, kSum) == COUNT);
    CHECK(MPIX_Get_accumulate_local_typed_async(wild, p, wild, empty, wild, empty, kSum, nullptr) ==
          COUNT);
    // 4
    for (MPIX_Op op : {kSum, kNoOp, kReplace}) {
        CHECK(MPIX_Accumulate_local_typed(wild, empty, nullptr, empty, op) == OK);
        CHECK(MPIX_Get_accumulate_local_typed_async(nullptr, nullptr, wild, empty, wild, empty, op,
                                                    nullptr) == OK);
    }
    // under MPI_NO_OP neither origin nor origin_plan is looked at
    CHECK(MPIX_Get_accumulate_local_typed(wild, junk, nullptr, empty, nullptr, empty, kNoOp) == OK);
    CHECK(MPIX_Accumulate_local_typed(wild, junk, nullptr, empty, kNoOp) == OK);
    CHECK(MPIX_Get_accumulate_local_typed(nullptr, junk, B, p, T, p, kNoOp) == BUFFER);
    // 5, 6
    CHECK(MPIX_Accumulate_local_typed_async(nullptr, p, T, p, kSum, nullptr) == BUFFER);
    CHECK(MPIX_Get_accumulate_local_typed(A, p, wild, p, T, p, kSum) == BUFFER);
    for (long z : {-191L, -64L, 0L, 50L, 191L}) {
        CHECK(MPIX_Get_accumulate_local_typed_async(A, p, T + z, p, T, p, kSum, nullptr) == BUFFER);
        CHECK(MPIX_Accumulate_local_typed_async(T + z, p, T, p, kSum, nullptr) == BUFFER);
        CHECK(MPIX_Get_accumulate_local_typed(A + z, p, A, p, T, p, kSum) == BUFFER);
    }
    CHECK(MPIX_Redop_last_error() == BUFFER);
    // 8: disjoint operands get as far as placement, which refuses wild pointers
    CHECK(MPIX_Get_accumulate_local_typed_async(A, p, B, nullptr, T, p, kSum, nullptr) == BUFFER);
    CHECK(MPIX_Iov_plan_prepare_packed(nullptr, 0) == ARG);
    CHECK(MPIX_Iov_plan_info_packed(nullptr, nullptr) == ARG);
    CHECK(MPIX_Iov_plan_locate(nullptr, 0, nullptr) == ARG);
    for (MPIX_Iov_plan *q : {&p, &pf, &p9, &empty})
        CHECK(MPIX_Iov_plan_free(q) == OK);
}

}  // namespace

int main()
{
    tables();
    launch_errors();
    printf("typed_host_check: %d errors\n", g_errors);
    return g_errors ? 1 : 0;
}
