// plan_host_check.cpp -- the host side of the committed iov plans
// (MPIX_Iov_plan_create[_iovec], _info, _free and the launch entries' checks
// that need no device) under AddressSanitizer + UndefinedBehaviorSanitizer:
// built by mpich_amd/csrc/sanitize.mk against the sanitizer build of
// redop_capi.cpp, run on the CPU, nothing preloaded.  What _info reports is
// compared with a straightforward re-derivation of the merged runs here.
#include <limits.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <set>
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

// handles and error classes of mpix_redop.h / mpi.h as this library numbers them
const MPIX_Datatype kDouble = 0x4c00080b, kInt16 = 0x4c000238, kInt8 = 0x4c000137,
                    kDoubleInt = (MPIX_Datatype) 0x8c000001, kFloatInt = (MPIX_Datatype) 0x8c000000,
                    kUnknown = 0x4c0000ff;
const MPIX_Op kSum = 0x58000003, kBand = 0x58000006, kNoOp = 0x5800000e, kNullOp = 0x18000000;
enum { OK = 0, BUFFER = 1, COUNT = 2, TYPE = 3, OP = 9, ARG = 12 };

struct Run {
    int64_t off, n;
};

struct Info {
    MPIX_Aint elements, runs, groups, lo, hi, table_bytes;
    bool operator==(const Info &o) const
    {
        return elements == o.elements && runs == o.runs && groups == o.groups && lo == o.lo &&
               hi == o.hi && table_bytes == o.table_bytes;
    }
};

// The plan of element runs (off, n) of extent `ext`, restated: drop the empty
// runs, merge a run into its predecessor when it starts where that one ends,
// group by offset modulo the extent; per group 3 n + 1 64-bit words and one
// 32-bit word per 256 elements plus one; nothing for at most one run.
Info derive(const std::vector<Run> &in, int64_t ext)
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
    Info i{0, (MPIX_Aint) m.size(), 0, 0, 0, 0};
    std::vector<int64_t> resid;
    std::vector<int64_t> nrun, total;
    for (size_t k = 0; k < m.size(); ++k) {
        i.elements += m[k].n;
        i.lo = k ? std::min<int64_t>(i.lo, m[k].off) : m[k].off;
        i.hi = k ? std::max<int64_t>(i.hi, m[k].off + m[k].n * ext) : m[k].off + m[k].n * ext;
        const int64_t r = ((m[k].off % ext) + ext) % ext;
        size_t g = std::find(resid.begin(), resid.end(), r) - resid.begin();
        if (g == resid.size()) {
            resid.push_back(r);
            nrun.push_back(0);
            total.push_back(0);
        }
        ++nrun[g];
        total[g] += m[k].n;
    }
    i.groups = (MPIX_Aint) resid.size();
    if (m.size() > 1)
        for (size_t g = 0; g < resid.size(); ++g)
            i.table_bytes += (3 * nrun[g] + 1) * 8 + ((total[g] + 255) / 256 + 1) * 4;
    return i;
}

Info info_of(MPIX_Iov_plan p)
{
    Info i{-1, -1, -1, -1, -1, -1};
    CHECK(MPIX_Iov_plan_info(p, &i.elements, &i.runs, &i.groups, &i.lo, &i.hi, &i.table_bytes) == OK);
    return i;
}

// create from element runs, compare _info with the re-derivation, free
void check_runs(const std::vector<Run> &runs, MPIX_Datatype dt, int64_t ext)
{
    std::vector<MPIX_Aint> offs, cnts;
    for (const Run &r : runs) {
        offs.push_back(r.off);
        cnts.push_back(r.n);
    }
    MPIX_Iov_plan p = nullptr;
    CHECK(MPIX_Iov_plan_create((MPIX_Aint) runs.size(), offs.data(), cnts.data(), dt, &p) == OK);
    CHECK(p != nullptr);
    if (!p)
        return;
    const Info want = derive(runs, ext), got = info_of(p);
    if (!(want == got))
        fprintf(stderr, "runs %ld/%ld groups %ld/%ld elements %ld/%ld bytes %ld/%ld\n",
                (long) got.runs, (long) want.runs, (long) got.groups, (long) want.groups,
                (long) got.elements, (long) want.elements, (long) got.table_bytes,
                (long) want.table_bytes);
    CHECK(want == got);
    CHECK(MPIX_Iov_plan_free(&p) == OK && p == nullptr);
}

int create_rc(MPIX_Aint nseg, const MPIX_Aint *a, const MPIX_Aint *b, MPIX_Datatype dt, bool iovec)
{
    MPIX_Iov_plan p = (MPIX_Iov_plan) (uintptr_t) 0xdead;
    const int rc = iovec ? MPIX_Iov_plan_create_iovec(nseg, a, b, dt, &p)
                         : MPIX_Iov_plan_create(nseg, a, b, dt, &p);
    CHECK(MPIX_Redop_last_error() == rc);
    CHECK((rc != OK) == (p == nullptr));
    if (p)
        CHECK(MPIX_Iov_plan_free(&p) == OK);
    return rc;
}

uint64_t g_seed = 0x5EED0D00;
uint32_t rnd(uint32_t n)
{
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t) (g_seed >> 33) % n;
}

void tables()
{
    // empty ones
    check_runs({}, kDouble, 8);
    check_runs({{0, 0}, {64, 0}, {-8, 0}}, kDouble, 8);
    check_runs({{3, 0}}, kDouble, 8);
    {
        MPIX_Iov_plan p = nullptr;
        CHECK(MPIX_Iov_plan_create(0, nullptr, nullptr, kDouble, &p) == OK && p);
        CHECK(info_of(p) == (Info{0, 0, 0, 0, 0, 0}));
        CHECK(MPIX_Iov_plan_free(&p) == OK);
    }
    // 10^5 single-element runs: contiguous (one run), every 7th one displaced
    // (nothing but chains of 6 merges), strided (nothing merges), reversed
    const int N = 100000;
    std::vector<Run> r(N);
    for (int k = 0; k < N; ++k)
        r[k] = Run{8 * (int64_t) k, 1};
    check_runs(r, kDouble, 8);
    CHECK(derive(r, 8).runs == 1);
    for (int k = 0; k < N; k += 7)
        r[k].off += 8 * (int64_t) N + 4;        // the other residue
    check_runs(r, kDouble, 8);
    CHECK(derive(r, 8).groups == 2);
    for (int k = 0; k < N; ++k)
        r[k] = Run{16 * (int64_t) k - 8 * (int64_t) N, 1};     // negative offsets
    check_runs(r, kDouble, 8);
    CHECK(derive(r, 8).runs == N && derive(r, 8).lo == -8 * (int64_t) N);
    std::reverse(r.begin(), r.end());
    check_runs(r, kDouble, 8);
    for (int k = 0; k < N; ++k)
        r[k] = Run{8 * (int64_t) (N - 1 - k), 1};   // adjacent in memory, descending: no merge
    check_runs(r, kDouble, 8);
    CHECK(derive(r, 8).runs == N);
    // random tables: lengths 0..5 (tile edges inside long merged chains), gaps
    // of 0 (a merge) or more, residues 0 / 4, negative offsets, three extents
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
        check_runs(q, t.dt, t.ext);
    }
    // the padded pair's raw iov: 37 contiguous MPI_DOUBLE_INT elements as 74
    // segments are one run; with a hole after element 20 they are two
    std::vector<MPIX_Aint> o, l;
    for (int k = 0; k < 37; ++k) {
        const MPIX_Aint at = 16 * k + (k > 20 ? 32 : 0);
        o.insert(o.end(), {at, at + 8});
        l.insert(l.end(), {8, 4});
    }
    MPIX_Iov_plan p = nullptr;
    CHECK(MPIX_Iov_plan_create_iovec(74, o.data(), l.data(), kDoubleInt, &p) == OK && p);
    Info i = info_of(p);
    CHECK(i.elements == 37 && i.runs == 2 && i.groups == 1 && i.lo == 0 && i.hi == 37 * 16 + 32);
    CHECK(MPIX_Iov_plan_free(&p) == OK);
    for (int k = 21; k < 37; ++k) {
        o[2 * k] -= 32;
        o[2 * k + 1] -= 32;
    }
    CHECK(MPIX_Iov_plan_create_iovec(74, o.data(), l.data(), kDoubleInt, &p) == OK && p);
    i = info_of(p);
    CHECK(i.elements == 37 && i.runs == 1 && i.table_bytes == 0 && i.hi == 37 * 16);
    CHECK(MPIX_Iov_plan_free(&p) == OK);
    // merged segments of the same pairs: {8, 4 + 8, ..., 4}
    CHECK(MPIX_Iov_plan_create_iovec(1, o.data(), l.data(), kDoubleInt, &p) == OK && p);
    CHECK(info_of(p).elements == 0);            // 8 bytes never complete an element
    CHECK(MPIX_Iov_plan_free(&p) == OK);
}

void create_errors()
{
    const MPIX_Aint top = (MPIX_Aint) 1 << 56;
    MPIX_Aint a[2] = {0, 64}, b[2] = {2, 2};
    for (int iovec = 0; iovec < 2; ++iovec) {
        CHECK(create_rc(-1, a, b, kUnknown, iovec) == COUNT);
        CHECK(create_rc((MPIX_Aint) INT_MAX + 1, nullptr, nullptr, kUnknown, iovec) == COUNT);
        CHECK(create_rc(1, nullptr, b, kDouble, iovec) == BUFFER);
        CHECK(create_rc(1, a, nullptr, kDouble, iovec) == BUFFER);
    }
    b[1] = -1;
    CHECK(create_rc(2, a, b, kUnknown, false) == COUNT);
    CHECK(create_rc(2, a, b, kUnknown, true) == TYPE);
    b[0] = 16;
    CHECK(create_rc(2, a, b, kDouble, true) == COUNT);
    b[0] = 12, b[1] = 4;
    CHECK(create_rc(1, a, b, kDouble, true) == ARG);            // a partial element
    MPIX_Aint f[2] = {0, 4}, fl[2] = {4, 4};
    CHECK(create_rc(2, f, fl, kFloatInt, true) == ARG);         // no padding: not a pairtype
    b[0] = 2, b[1] = 2;
    CHECK(create_rc(2, a, b, kUnknown, false) == TYPE);
    a[1] = 66;
    CHECK(create_rc(2, a, b, kDouble, false) == ARG);           // 2 mod 8
    a[1] = 68;
    CHECK(create_rc(2, a, b, kDouble, false) == OK);            // 4 mod 8
    a[0] = 1;
    CHECK(create_rc(1, a, b, kInt16, false) == ARG);
    a[0] = 2, b[0] = top / 8;
    CHECK(create_rc(1, a, b, kDouble, false) == ARG);           // the residue before the cap
    a[0] = 0;
    CHECK(create_rc(1, a, b, kDouble, false) == COUNT);
    b[0] = top / 8 - 1;
    CHECK(create_rc(1, a, b, kDouble, false) == OK);
    a[1] = 0, b[0] = b[1] = top / 16;
    CHECK(create_rc(2, a, b, kDouble, false) == COUNT);         // the sum
    a[1] = top - 8, b[0] = b[1] = 1;
    CHECK(create_rc(2, a, b, kDouble, false) == COUNT);         // the bounding range
    a[0] = -((MPIX_Aint) 1 << 62), a[1] = (MPIX_Aint) 1 << 62;
    CHECK(create_rc(2, a, b, kDouble, false) == COUNT);
    b[0] = INT64_MAX;
    CHECK(create_rc(1, a, b, kDouble, false) == COUNT);
    b[0] = top;
    a[0] = 0;
    CHECK(create_rc(1, a, b, kDouble, true) == COUNT);
    b[0] = 4;
    CHECK(MPIX_Iov_plan_create(1, a, b, kDouble, nullptr) == ARG);
    CHECK(MPIX_Iov_plan_create_iovec(0, nullptr, nullptr, kDouble, nullptr) == ARG);
    CHECK(MPIX_Iov_plan_free(nullptr) == ARG);
    MPIX_Iov_plan none = nullptr;
    CHECK(MPIX_Iov_plan_free(&none) == OK);
    CHECK(MPIX_Iov_plan_info(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == ARG);
    CHECK(MPIX_Iov_plan_prepare(nullptr, 0) == ARG);
}

// the launch entries' checks that come before any device work, on pointers
// that are never dereferenced
void launch_errors()
{
    char *A = (char *) 0x100000, *B = (char *) 0x200000, *T = (char *) 0x300000;
    void *wild = (void *) -1;
    MPIX_Aint offs[2] = {96, -64}, cnts[2] = {4, 4};
    MPIX_Iov_plan p = nullptr, empty = nullptr;
    CHECK(MPIX_Iov_plan_create(2, offs, cnts, kDouble, &p) == OK);
    CHECK(MPIX_Iov_plan_create(0, nullptr, nullptr, kDouble, &empty) == OK);
    CHECK(MPIX_Reduce_local_plan_async(A, T, nullptr, kSum, nullptr) == ARG);
    CHECK(MPIX_Reduce_local_plan(A, T, nullptr, kSum) == ARG);
    CHECK(MPIX_Get_accumulate_local_plan_async(A, B, T, nullptr, kSum, nullptr) == ARG);
    CHECK(MPIX_Get_accumulate_local_plan(A, B, T, nullptr, kSum) == ARG);
    for (MPIX_Op op : {kBand, kNullOp}) {
        CHECK(MPIX_Reduce_local_plan_async(nullptr, nullptr, p, op, nullptr) == OP);
        CHECK(MPIX_Get_accumulate_local_plan(nullptr, nullptr, nullptr, p, op) == OP);
        CHECK(MPIX_Get_accumulate_local_plan_async(wild, wild, wild, empty, op, nullptr) == OP);
    }
    for (MPIX_Op op : {kSum, kNoOp}) {
        CHECK(MPIX_Reduce_local_plan_async(nullptr, wild, empty, op, nullptr) == OK);
        CHECK(MPIX_Reduce_local_plan(wild, nullptr, empty, op) == OK);
        CHECK(MPIX_Get_accumulate_local_plan_async(wild, nullptr, wild, empty, op, nullptr) == OK);
        CHECK(MPIX_Get_accumulate_local_plan(nullptr, wild, nullptr, empty, op) == OK);
    }
    CHECK(MPIX_Reduce_local_plan_async(nullptr, T, p, kSum, nullptr) == BUFFER);
    CHECK(MPIX_Reduce_local_plan(A, wild, p, kSum) == BUFFER);
    CHECK(MPIX_Get_accumulate_local_plan_async(A, nullptr, T, p, kSum, nullptr) == BUFFER);
    CHECK(MPIX_Get_accumulate_local_plan(nullptr, B, T, p, kSum) == BUFFER);
    // overlap with the bounding range [T - 64, T + 128), its gap included
    for (long z : {-64L, 0L, 50L, 127L, -127L}) {
        CHECK(MPIX_Get_accumulate_local_plan_async(A, T + z, T, p, kSum, nullptr) == BUFFER);
        CHECK(MPIX_Reduce_local_plan_async(T + z, T, p, kSum, nullptr) == BUFFER);
    }
    CHECK(MPIX_Redop_last_error() == BUFFER);
    CHECK(MPIX_Iov_plan_free(&p) == OK && MPIX_Iov_plan_free(&empty) == OK);
}

}  // namespace

int main()
{
    tables();
    create_errors();
    launch_errors();
    printf("plan_host_check: %d errors\n", g_errors);
    return g_errors ? 1 : 0;
}
