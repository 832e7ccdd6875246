// redop_runs.h -- derived (non-contiguous) targets as runs: the one copy of the
// host arithmetic between a caller's iov / iovec table and the words a kernel
// indexes with (the runs, their scan, merge, residue groups and tile indexes,
// and a committed plan's whole layout).  Pure host C++, no HIP call, so
// tests/c/runs_check.cpp builds against this header alone (tests/test_runs.py).
// redop_capi.cpp keeps what calls HIP and each entry's own order of answers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "mpix_redop.h"
#include "redop_dispatch.h"      // RunGroup; PackedTab through redop_packed.h

namespace mpix {

// One uop call of typerep_op_fallback: `n` elements at extent stride from
// byte offset `off` of inout (may be negative: lb < 0), combined with the
// next n elements of the packed source.
struct Run {
    int64_t off, n;
};

// The element runs of the flattened-iov forms (seg_counts in elements).
inline int runs_from_iov(MPIX_Aint nseg, const MPIX_Aint *seg_offsets, const MPIX_Aint *seg_counts,
                         std::vector<Run> *runs)
{
    if (nseg < 0)
        return MPIX_REDOP_ERR_COUNT;
    if (nseg > 0 && (!seg_offsets || !seg_counts))
        return MPIX_REDOP_ERR_BUFFER;
    runs->reserve((size_t) nseg);
    for (MPIX_Aint s = 0; s < nseg; ++s) {
        if (seg_counts[s] < 0)
            return MPIX_REDOP_ERR_COUNT;
        runs->push_back(Run{seg_offsets[s], seg_counts[s]});
    }
    return MPIX_REDOP_SUCCESS;
}

// The element runs of the raw-iovec forms (iov_lens in bytes) of a basic type
// of `size` data bytes per element at `ext` stride; ext == 0: the caller's
// handle names no such type, answered after the table pointers' checks.
inline int runs_from_iovec(MPIX_Aint nseg, const MPIX_Aint *iov_offsets, const MPIX_Aint *iov_lens,
                           uint64_t size, uint64_t ext, std::vector<Run> *runs)
{
    if (nseg < 0)
        return MPIX_REDOP_ERR_COUNT;
    if (nseg > 0 && (!iov_offsets || !iov_lens))
        return MPIX_REDOP_ERR_BUFFER;
    if (ext == 0)
        return MPIX_REDOP_ERR_TYPE;
    // typerep_op.c:115-149: segments are gathered until they hold one
    // element's data (pairtypes split by their padding); each call covers
    // curr_len / size elements laid out at extent stride from target_ptr,
    // and a partial element left at the end of a segment starts the next one
    const bool pairtype = size < ext;
    runs->reserve((size_t) nseg);
    MPIX_Aint curr = 0, target = 0;
    for (MPIX_Aint i = 0; i < nseg; ++i) {
        if (iov_lens[i] < 0)
            return MPIX_REDOP_ERR_COUNT;
        if (pairtype) {
            if (curr == 0)
                target = iov_offsets[i];
            curr += iov_lens[i];
            if (curr < (MPIX_Aint) size)
                continue;
        } else {
            target = iov_offsets[i];
            curr = iov_lens[i];
        }
        MPIX_Aint n = curr / (MPIX_Aint) size;
        MPIX_Aint data = n * (MPIX_Aint) size;
        runs->push_back(Run{target, n});
        if (pairtype) {
            curr -= data;
            if (curr > 0)
                target = iov_offsets[i] + (iov_lens[i] - curr);
        } else if (curr != data) {
            return MPIX_REDOP_ERR_ARG;            // the reference's MPIR_Assert (:147)
        }
    }
    return MPIX_REDOP_SUCCESS;
}

// Total elements and the target's bounding byte range [lo, hi): lowest run
// start to highest run end, zero-length runs aside.  `over`: a run, or the
// running total, passed 2^56 / ext elements (a packed operand would reach 2^56
// bytes); the scan stops at that run.  128-bit bounds: off + n * ext may pass
// 64 bits in a table about to be refused (n * ext itself is at most 2^56).
struct RunScan {
    uint64_t total;
    __int128 lo, hi;
    bool over;
    // ERR_COUNT: over, or the packed operands or the bounding range reach 2^56 bytes
    bool too_long(uint64_t ext) const
    {
        const __int128 span_cap = (__int128) 1 << 56;
        return over || hi - lo >= span_cap || (__int128) total * ext >= span_cap;
    }
};

inline RunScan scan_runs(const std::vector<Run> &runs, uint64_t ext)
{
    const uint64_t cap = ((uint64_t) 1 << 56) / ext;
    RunScan sc{0, 0, 0, false};
    bool any = false;
    for (const Run &r : runs) {
        if (r.n == 0)
            continue;
        if ((uint64_t) r.n > cap || sc.total + (uint64_t) r.n > cap) {
            sc.over = true;
            break;
        }
        sc.total += (uint64_t) r.n;
        const __int128 a = r.off, b = a + (__int128) ((uint64_t) r.n * ext);
        if (!any || a < sc.lo)
            sc.lo = a;
        if (!any || b > sc.hi)
            sc.hi = b;
        any = true;
    }
    return sc;
}

// Residues must keep the 4-byte (for smaller types, the extent's) alignment
// the element loads need.  Every run counts, an empty one too.
inline bool residues_aligned(const std::vector<Run> &runs, int64_t e)
{
    const int64_t align = e < 4 ? e : 4;
    for (const Run &r : runs)
        if ((((r.off % e) + e) % e) % align)
            return false;
    return true;
}

// Merge in call order, in place: run k+1 starting where run k ends continues it
// (its packed elements follow run k's by construction); zero-length runs drop
// out, so one between two such runs does not keep them apart.
inline void merge_runs(std::vector<Run> &runs, int64_t e)
{
    size_t m = 0;
    for (size_t k = 0; k < runs.size(); ++k) {
        const Run r = runs[k];
        if (r.n == 0)
            continue;
        if (m > 0 && (__int128) runs[m - 1].off + (__int128) runs[m - 1].n * e == (__int128) r.off)
            runs[m - 1].n += r.n;
        else
            runs[m++] = r;
    }
    runs.resize(m);
}

// The runs of one call grouped by their offset modulo the extent (zero-length
// runs dropped).  Group g indexes the target in whole elements from
// target + resid[g]; its table [seg_off n][prefix n+1][src_off n] (n =
// nrun[g]) starts at tab[base[g]]: element offset of each run, elements of the
// group before it (prefix[n] = gtotal[g]), and its first element's index in
// the packed operands, which follow the call's run order.
struct RunTable {
    std::vector<int64_t> resid, gtotal, tab;
    std::vector<size_t> base, nrun;
};

// Group g of a run table, its arrays read from `tab`: the host table
// (rt.tab.data()) or a device copy of it.  `tile`: a plan's tile index of the
// group (PlanLayout::group); a per-call table has none.
struct ResidueGroup : RunGroup {
    int64_t n;          // runs
    uint64_t total;     // packed elements
    int64_t resid;
    const int32_t *tile;
    ResidueGroup(const RunTable &rt, size_t g, const int64_t *tab, const int32_t *tile = nullptr)
        : RunGroup(tab + rt.base[g], (int64_t) rt.nrun[g]), n((int64_t) rt.nrun[g]),
          total((uint64_t) rt.gtotal[g]), resid(rt.resid[g]), tile(tile) {}
};

inline void group_runs(const std::vector<Run> &runs, int64_t e, RunTable *rt)
{
    std::vector<std::vector<size_t>> groups;
    for (size_t k = 0; k < runs.size(); ++k) {
        if (runs[k].n == 0)
            continue;
        int64_t r = ((runs[k].off % e) + e) % e;
        size_t g = 0;
        while (g < rt->resid.size() && rt->resid[g] != r)
            ++g;
        if (g == rt->resid.size()) {
            rt->resid.push_back(r);
            groups.emplace_back();
        }
        groups[g].push_back(k);
    }
    std::vector<int64_t> src_of(runs.size());
    {
        int64_t src = 0;
        for (size_t k = 0; k < runs.size(); ++k) {
            src_of[k] = src;
            src += runs[k].n;
        }
    }
    size_t need = 0;
    for (const auto &g : groups)
        need += 3 * g.size() + 1;
    rt->tab.resize(need);
    rt->base.resize(groups.size());
    rt->nrun.resize(groups.size());
    rt->gtotal.resize(groups.size());
    size_t at = 0;
    for (size_t g = 0; g < groups.size(); ++g) {
        const size_t n = groups[g].size();
        rt->base[g] = at;
        rt->nrun[g] = n;
        int64_t pre = 0;
        for (size_t q = 0; q < n; ++q) {
            const Run &r = runs[groups[g][q]];
            rt->tab[at + q] = (r.off - rt->resid[g]) / e;
            rt->tab[at + n + q] = pre;
            rt->tab[at + 2 * n + 1 + q] = src_of[groups[g][q]];
            pre += r.n;
        }
        rt->tab[at + 2 * n] = pre;
        rt->gtotal[g] = pre;
        at += 3 * n + 1;
    }
}

// The tile index of `n` runs whose packed elements start at prefix[0 .. n)
// (prefix[n] = total): out[t] = the run that holds packed index 256 t, closed
// by out[ntile] = n - 1; ntile + 1 words, ntile = ceil(total / 256).
inline void tile_index(const int64_t *prefix, int64_t n, uint64_t total, int32_t *out)
{
    const uint64_t ntile = (total + 255) / 256;
    int64_t s = 0;
    for (uint64_t t = 0; t < ntile; ++t) {
        while (s + 1 < n && (uint64_t) prefix[s + 1] <= t * 256)
            ++s;
        out[t] = (int32_t) s;
    }
    out[ntile] = (int32_t) (n - 1);
}

// What MPI_Type_commit is to a datatype: the runs of one (table, basic type),
// merged, grouped by residue and indexed per tile once.  Immutable after build.
struct PlanLayout {
    uint32_t it = 0;
    uint64_t ext = 0;
    uint64_t total = 0;             // packed elements
    int64_t nrun = 0;               // runs after the merge
    int64_t lo = 0, hi = 0;         // the target's bounding byte range [lo, hi)
    int64_t one_off = 0;            // nrun == 1: the run's byte offset
    RunTable rt;                    // group_runs of the merged runs
    std::vector<int32_t> tile;      // every group's tile index, group g from tile_base[g]
    std::vector<size_t> tile_base;
    size_t table_bytes = 0;         // device bytes: rt.tab, then tile (0: nothing to upload)
    // the packed-order table (redop_packed.h) over all merged runs in call
    // order, as one device holds it: prefix, off, tile (empty for nrun <= 1)
    std::vector<char> pk;

    // Merge (in place), group and index the runs of a table whose type is
    // resolved.  A table of zero elements is a valid plan whatever its offsets,
    // as the entries succeed on it; else every run's residue counts, then the caps.
    int build(std::vector<Run> &runs, uint32_t type, uint64_t extent)
    {
        const int64_t e = (int64_t) extent;
        const RunScan sc = scan_runs(runs, extent);
        if (sc.over || sc.total != 0) {
            if (!residues_aligned(runs, e))
                return MPIX_REDOP_ERR_ARG;
            if (sc.too_long(extent))
                return MPIX_REDOP_ERR_COUNT;
        }
        merge_runs(runs, e);
        const size_t m = runs.size();
        it = type;
        ext = extent;
        total = sc.total;
        nrun = (int64_t) m;
        lo = (int64_t) sc.lo;
        hi = (int64_t) sc.hi;
        if (m == 1)
            one_off = runs[0].off;
        if (m <= 1)         // a single run takes the contiguous path: no table
            return MPIX_REDOP_SUCCESS;
        pk.resize(packed_tab_bytes((int64_t) m, total));
        int64_t *prefix = (int64_t *) pk.data(), *off = prefix + m + 1;
        int64_t pre = 0;
        for (size_t k = 0; k < m; ++k) {
            prefix[k] = pre;
            off[k] = runs[k].off;
            pre += runs[k].n;
        }
        prefix[m] = pre;
        tile_index(prefix, (int64_t) m, total, (int32_t *) (off + m));
        group_runs(runs, e, &rt);
        for (size_t g = 0; g < groups(); ++g) {
            tile_base.push_back(tile.size());
            tile.resize(tile.size() + (size_t) (((uint64_t) rt.gtotal[g] + 255) / 256) + 1);
            const ResidueGroup gr = group(g);
            tile_index(gr.prefix, gr.n, gr.total, tile.data() + tile_base[g]);
        }
        table_bytes = tile_pos() + tile.size() * sizeof(int32_t);
        return MPIX_REDOP_SUCCESS;
    }

    size_t groups() const { return rt.resid.size(); }

    // Byte position of the tile words in the device allocation: behind rt.tab.
    size_t tile_pos() const { return rt.tab.size() * sizeof(int64_t); }

    // Group g over the host tables ...
    ResidueGroup group(size_t g) const
    {
        return ResidueGroup(rt, g, rt.tab.data(), tile.data() + tile_base[g]);
    }

    // ... and over a device copy of them (`dev`: table_bytes bytes).  seg_off
    // is the group's whole table, as the plan kernels take it.
    ResidueGroup group(size_t g, const char *dev) const
    {
        return ResidueGroup(rt, g, (const int64_t *) dev,
                            (const int32_t *) (dev + tile_pos()) + tile_base[g]);
    }

    // Every group over a device copy, in order, until f answers an error.
    template <class F>
    int each_group(const char *dev, F f) const
    {
        int rc = MPIX_REDOP_SUCCESS;
        for (size_t g = 0; g < groups() && rc == MPIX_REDOP_SUCCESS; ++g)
            rc = f(group(g, dev));
        return rc;
    }

    // Byte offset, relative to the buffer pointer, of packed element p < total.
    int64_t locate(uint64_t p) const
    {
        if (nrun == 1)
            return one_off + (int64_t) p * (int64_t) ext;
        const PackedTab t(pk.data(), nrun);
        return packed_byte(t.prefix, t.off, t.tile, p, (int64_t) ext);
    }
};

}  // namespace mpix
