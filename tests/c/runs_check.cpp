// The derived layouts' host arithmetic (mpich_amd/csrc/redop_runs.h) on its
// own: no library, no HIP runtime, no device.  Built and run by
// tests/test_runs.py, once more under AddressSanitizer + UBSan.
//
//   runs_check fixture   one case per stdin line
//                          form size ext nseg nulls len off*len second*len
//                        (form 1: raw iovec; nulls bit 0 / 1: the offsets / the
//                        second array go in as NULL) -> one line per case with
//                        every word the header computes (dump(), below), which
//                        the test compares with tests/golden/run_tables.json
//   runs_check props     seeded random tables: the merged runs tile the packed
//                        order; every packed index maps through its residue
//                        group's (seg_off, prefix, src_off) to the byte a plain
//                        walk of the input runs gives, and so does locate(); the
//                        tile words bracket the run of every index, per group
//                        and in the packed-order table; scan_runs equals a
//                        128-bit brute force
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "redop_runs.h"

using mpix::PlanLayout;
using mpix::ResidueGroup;
using mpix::Run;
using mpix::RunScan;
using mpix::RunTable;

typedef __int128 i128;

static std::string str128(i128 v)
{
    if (v == 0)
        return "0";
    const bool neg = v < 0;
    unsigned __int128 u = neg ? -(unsigned __int128) v : (unsigned __int128) v;
    std::string s;
    while (u) {
        s.insert(s.begin(), (char) ('0' + (int) (u % 10)));
        u /= 10;
    }
    return neg ? "-" + s : s;
}

static void put_runs(std::ostream &o, const char *name, const std::vector<Run> &runs)
{
    o << ' ' << name << ' ' << runs.size();
    for (const Run &r : runs)
        o << ' ' << r.off << ' ' << r.n;
}

static void put_group(std::ostream &o, const char *name, const ResidueGroup &g)
{
    o << ' ' << name << ' ' << g.resid << ' ' << g.n << ' ' << g.total << " tab";
    for (int64_t k = 0; k < 3 * g.n + 1; ++k)
        o << ' ' << g.seg_off[k];
    if (g.tile) {
        o << " tile";
        for (uint64_t t = 0; t < (g.total + 255) / 256 + 1; ++t)
            o << ' ' << g.tile[t];
    }
}

// parse R [runs .. scan .. aligned A build R [plan .. merged .. group .. pk ..
// calltab ..]]: everything between the caller's arrays and the device words
static std::string dump(int form, uint64_t size, uint64_t ext, int64_t nseg, const int64_t *offs,
                        const int64_t *second)
{
    std::ostringstream o;
    std::vector<Run> runs;
    int rc = form ? mpix::runs_from_iovec(nseg, offs, second, size, ext, &runs)
                  : mpix::runs_from_iov(nseg, offs, second, &runs);
    o << "parse " << rc;
    if (rc != MPIX_REDOP_SUCCESS)
        return o.str();
    put_runs(o, "runs", runs);
    const RunScan sc = mpix::scan_runs(runs, ext);
    o << " scan " << sc.total << ' ' << str128(sc.lo) << ' ' << str128(sc.hi) << ' ' << sc.over;
    o << " aligned " << mpix::residues_aligned(runs, (int64_t) ext);
    const std::vector<Run> raw = runs;
    PlanLayout p;
    rc = p.build(runs, 7, ext);
    o << " build " << rc;
    if (rc != MPIX_REDOP_SUCCESS)
        return o.str();
    o << " plan " << p.total << ' ' << p.nrun << ' ' << p.lo << ' ' << p.hi << ' ' << p.one_off << ' '
      << p.table_bytes << ' ' << p.pk.size() << ' ' << p.groups() << ' ' << p.tile_pos();
    put_runs(o, "merged", runs);
    for (size_t g = 0; g < p.groups(); ++g)
        put_group(o, "group", p.group(g));
    if (!p.pk.empty()) {
        o << " pk";
        const int64_t *w = (const int64_t *) p.pk.data();
        for (int64_t k = 0; k < 2 * p.nrun + 1; ++k)
            o << ' ' << w[k];
        const mpix::PackedTab t(p.pk.data(), p.nrun);
        for (uint64_t k = 0; k < (p.total + 255) / 256 + 1; ++k)
            o << ' ' << t.tile[k];
    }
    if (p.total) {      // the per-call table of the iov entries: no merge
        RunTable rt;
        mpix::group_runs(raw, (int64_t) ext, &rt);
        for (size_t g = 0; g < rt.resid.size(); ++g)
            put_group(o, "calltab", ResidueGroup(rt, g, rt.tab.data()));
    }
    return o.str();
}

static int fixture()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int form, nulls;
        uint64_t size, ext;
        int64_t nseg;
        size_t len;
        if (!(in >> form >> size >> ext >> nseg >> nulls >> len))
            return 2;
        std::vector<int64_t> offs(len), second(len);
        for (auto &v : offs)
            in >> v;
        for (auto &v : second)
            in >> v;
        if (!in)
            return 2;
        printf("%s\n", dump(form, size, ext, nseg, (nulls & 1) ? nullptr : offs.data(),
                            (nulls & 2) ? nullptr : second.data())
                           .c_str());
    }
    return 0;
}

// ------------------------------------------------------------------ props
static uint64_t g_rng = 0x5EED0C01u;
static uint64_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}
static int64_t below(int64_t n) { return (int64_t) (rnd() % (uint64_t) n); }

#define CHECK(c)                                                                     \
    do {                                                                             \
        if (!(c)) {                                                                  \
            fprintf(stderr, "%s:%d: table %d: %s\n", __FILE__, __LINE__, g_iter, #c); \
            return 1;                                                                \
        }                                                                            \
    } while (0)
static int g_iter;

// tile[t], tile[t + 1] bracket the run of every index of tile t
static int brackets(const int64_t *prefix, const int32_t *tile, int64_t n, uint64_t total)
{
    CHECK((uint64_t) prefix[n] == total && prefix[0] == 0);
    int64_t q = 0;
    for (uint64_t i = 0; i < total; ++i) {
        while ((uint64_t) prefix[q + 1] <= i)
            ++q;
        CHECK(tile[i >> 8] <= q && q <= tile[(i >> 8) + 1]);
        CHECK(mpix::packed_run(prefix, tile, i) == q);
    }
    CHECK(tile[(total + 255) / 256] == n - 1);
    return 0;
}

static int one_table()
{
    static const int64_t exts[] = {1, 2, 4, 8, 16, 32};
    const int64_t e = exts[below(6)], align = e < 4 ? e : 4;
    const int nres = 1 + (int) below(4);
    int64_t resid[4];
    for (int r = 0; r < nres; ++r)
        resid[r] = below(e / align) * align;
    const bool ones = below(8) == 0;            // many runs in a tile
    const int nruns = ones ? 300 + (int) below(200) : 1 + (int) below(40);
    const int64_t longest = ones ? 1 : 1 + below(below(4) == 0 ? 1500 : 120);
    std::vector<Run> runs;
    int64_t el = below(2001) - 1000, res = resid[0];    // may start below the buffer pointer
    for (int k = 0; k < nruns; ++k) {
        const int64_t n = below(6) == 0 ? 0 : 1 + below(longest);
        if (below(3)) {                         // else: starts where the last one ended
            el += below(64) - 8;
            res = resid[below(nres)];
        }
        runs.push_back(Run{el * e + res, n});
        el += n;
    }
    // the plain walk: packed index -> byte offset
    std::vector<int64_t> byte_of;
    for (const Run &r : runs)
        for (int64_t j = 0; j < r.n; ++j)
            byte_of.push_back(r.off + j * e);
    const uint64_t total = byte_of.size();
    CHECK(mpix::residues_aligned(runs, e));
    std::vector<Run> merged = runs;
    PlanLayout p;
    CHECK(p.build(merged, 7, (uint64_t) e) == MPIX_REDOP_SUCCESS);
    CHECK(p.total == total && p.nrun == (int64_t) merged.size() && p.ext == (uint64_t) e);
    // the merged runs tile the packed order, none empty, no two mergeable
    uint64_t at = 0;
    for (size_t k = 0; k < merged.size(); ++k) {
        CHECK(merged[k].n > 0);
        CHECK(k == 0 || merged[k - 1].off + merged[k - 1].n * e != merged[k].off);
        for (int64_t j = 0; j < merged[k].n; ++j, ++at)
            CHECK(at < total && byte_of[at] == merged[k].off + j * e);
    }
    CHECK(at == total);
    for (uint64_t i = 0; i < total; ++i)
        CHECK(p.locate(i) == byte_of[i]);
    if (total) {
        int64_t lo = byte_of[0], hi = byte_of[0] + e;
        for (int64_t b : byte_of) {
            lo = b < lo ? b : lo;
            hi = b + e > hi ? b + e : hi;
        }
        CHECK(p.lo == lo && p.hi == hi);
    }
    if (p.nrun <= 1) {
        CHECK(p.groups() == 0 && p.table_bytes == 0 && p.pk.empty());
        CHECK(p.nrun == 0 || p.one_off == byte_of[0]);
        return 0;
    }
    // every packed index through its group's table, once
    std::vector<int> seen(total, 0);
    size_t words = 0;
    std::vector<char> dev(p.table_bytes);
    memcpy(dev.data(), p.rt.tab.data(), p.tile_pos());
    memcpy(dev.data() + p.tile_pos(), p.tile.data(), p.table_bytes - p.tile_pos());
    for (size_t g = 0; g < p.groups(); ++g) {
        const ResidueGroup gr = p.group(g);
        CHECK(gr.resid >= 0 && gr.resid < e && gr.n > 0);
        for (size_t h = 0; h < g; ++h)
            CHECK(p.rt.resid[h] != gr.resid);
        for (int64_t q = 0; q < gr.n; ++q) {
            const int64_t len = gr.prefix[q + 1] - gr.prefix[q];
            CHECK(len > 0);
            for (int64_t j = 0; j < len; ++j) {
                const uint64_t pi = (uint64_t) (gr.src_off[q] + j);
                CHECK(pi < total && !seen[pi]++);
                CHECK(gr.resid + (gr.seg_off[q] + j) * e == byte_of[pi]);
            }
        }
        if (brackets(gr.prefix, gr.tile, gr.n, gr.total))
            return 1;
        // the view over one allocation (a device's copy) addresses the same words
        const ResidueGroup dg = p.group(g, dev.data());
        CHECK(!memcmp(dg.seg_off, gr.seg_off, (size_t) (3 * gr.n + 1) * 8));
        CHECK(!memcmp(dg.tile, gr.tile, ((gr.total + 255) / 256 + 1) * 4));
        words += (size_t) (3 * gr.n + 1) * 8 + ((gr.total + 255) / 256 + 1) * 4;
    }
    CHECK(words == p.table_bytes);
    for (uint64_t i = 0; i < total; ++i)
        CHECK(seen[i] == 1);
    const mpix::PackedTab t(p.pk.data(), p.nrun);
    CHECK(p.pk.size() == mpix::packed_tab_bytes(p.nrun, total));
    for (int64_t k = 0; k < p.nrun; ++k)
        CHECK(t.off[k] == merged[k].off && t.prefix[k + 1] - t.prefix[k] == merged[k].n);
    return brackets(t.prefix, t.tile, p.nrun, total);
}

// scan_runs against sums kept in 128 bits throughout
static int one_scan()
{
    static const uint64_t exts[] = {1, 2, 4, 8, 16, 32};
    const uint64_t ext = exts[below(6)];
    const i128 top = (i128) 1 << 56;
    const int nruns = (int) below(6);
    std::vector<Run> runs;
    for (int k = 0; k < nruns; ++k) {
        int64_t n;
        switch (below(5)) {
        case 0: n = 0; break;
        case 1: n = (int64_t) (((uint64_t) 1 << 56) / ext) + below(3) - 1; break;
        case 2: n = (int64_t) (((uint64_t) 1 << 55) / ext) + below(3) - 1; break;
        case 3: n = (int64_t) (rnd() >> 1); break;
        default: n = 1 + below(1000);
        }
        const int64_t off = below(3) ? (int64_t) rnd() >> (8 + below(50)) : (int64_t) rnd();
        runs.push_back(Run{off, n});
    }
    i128 total = 0, lo = 0, hi = 0;
    bool over = false, any = false;
    for (const Run &r : runs) {
        if (r.n == 0)
            continue;
        if ((i128) r.n * ext > top || (total + r.n) * ext > top) {
            over = true;
            break;
        }
        total += r.n;
        const i128 a = r.off, b = a + (i128) r.n * ext;
        lo = !any || a < lo ? a : lo;
        hi = !any || b > hi ? b : hi;
        any = true;
    }
    const RunScan sc = mpix::scan_runs(runs, ext);
    CHECK(sc.over == over && (i128) sc.total == total && sc.lo == lo && sc.hi == hi);
    CHECK(sc.too_long(ext) == (over || hi - lo >= top || total * ext >= top));
    return 0;
}

static int props()
{
    const int tables = 3000, scans = 20000;
    for (g_iter = 0; g_iter < tables; ++g_iter)
        if (one_table())
            return 1;
    for (g_iter = 0; g_iter < scans; ++g_iter)
        if (one_scan())
            return 1;
    printf("tables: %d scans: %d\nruns props: ok\n", tables, scans);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "fixture"))
        return fixture();
    if (argc == 2 && !strcmp(argv[1], "props"))
        return props();
    fprintf(stderr, "usage: runs_check fixture|props\n");
    return 2;
}
