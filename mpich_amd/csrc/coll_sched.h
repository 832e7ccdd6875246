// coll_sched.h -- the index arithmetic of libmpix_coll's schedules and nothing
// else: block layouts, the non-power-of-two pair fold, the halving walk over a
// window of blocks and its reverse, the pull tree's slot -> source rank map,
// the multipath and pipelined cuts, and the workspace / schedule choices.  No
// HIP or RCCL include and no communicator, so tests/c/coll_sched_check.cpp
// builds it with g++ alone (as redop_hostpath.h / redop_fixup.h are).
#ifndef MPIX_COLL_SCHED_H_INCLUDED
#define MPIX_COLL_SCHED_H_INCLUDED

#include <stddef.h>

#include <vector>

#include "mpix_coll.h"

namespace coll_sched {

inline size_t round256(size_t b) { return (b + 255) & ~(size_t) 255; }

inline int pof2_of(int n)
{
    int p = 1;
    while (p * 2 <= n)
        p *= 2;
    return p;
}

inline int bitrev(int r, int pof2)
{
    int out = 0;
    for (int b = pof2 >> 1; b; b >>= 1) {
        out = (out << 1) | (r & 1);
        r >>= 1;
    }
    return out;
}

// A vector of `total` elements cut into n consecutive blocks: block i is
// [disps[i], disps[i + 1]), so disps has n + 1 entries and disps[n] = total.
struct Blocks {
    std::vector<size_t> disps;
    size_t total = 0;

    explicit Blocks(const std::vector<size_t> &cnts) : disps(cnts.size() + 1, 0)
    {
        for (size_t i = 0; i < cnts.size(); ++i)
            disps[i + 1] = disps[i] + cnts[i];
        total = disps[cnts.size()];
    }
    int n() const { return (int) disps.size() - 1; }
    size_t cnt(int i) const { return disps[i + 1] - disps[i]; }
    // elements in blocks [lo, hi)
    size_t range(int lo, int hi) const { return disps[hi] - disps[lo]; }

    // count / n each, one more for the first count % n
    // (allreduce_intra_reduce_scatter_allgather.c:118-127)
    static Blocks even(size_t count, int n)
    {
        Blocks b(n);
        for (int i = 0; i < n; ++i)
            b.disps[i + 1] = b.disps[i] + count / n + ((size_t) i < count % n ? 1 : 0);
        b.total = count;
        return b;
    }
    // ceil(count / P) each, the last ones short or empty (allreduce_intra_ring.c:34-42)
    static Blocks ring(size_t count, int P)
    {
        Blocks b(P);
        const size_t each = (count + P - 1) / P;
        for (int i = 0; i < P; ++i)
            b.disps[i + 1] = b.disps[i] + each > count ? count : b.disps[i] + each;
        b.total = count;
        return b;
    }

private:
    explicit Blocks(int n) : disps(n + 1, 0) {}
};

// The non-power-of-two fold: the ranks below 2 * rem pair up (2i, 2i + 1), one
// of each pair hands its whole vector to the other and drops out, and the
// pof2 ranks left renumber themselves 0 .. pof2 - 1.  The reduce-scatter and
// the allreduces keep the ODD rank of a pair (…recursive_halving.c:110-137),
// reduce_scatter_gather the EVEN one (reduce_intra_reduce_scatter_gather.c:110-134).
struct Fold {
    int pof2, rem;
    bool keep_odd;
    bool paired;    // this rank is one of a pair; its partner is rank ^ 1
    int newrank;    // -1: folded away

    Fold(int rank, int size, bool keep_odd_)
        : pof2(pof2_of(size)), rem(size - pof2_of(size)), keep_odd(keep_odd_),
          paired(rank < 2 * rem), newrank(newrank_of(rank))
    {
    }
    int newrank_of(int rank) const
    {
        if (rank >= 2 * rem)
            return rank - rem;
        return (rank % 2 == 1) == keep_odd ? rank / 2 : -1;
    }
    int real(int nr) const { return nr < rem ? nr * 2 + (keep_odd ? 1 : 0) : nr + rem; }
    // counts of the new ranks' blocks: a kept rank also carries its dropped
    // neighbour's (…recursive_halving.c:145-160; keep_odd)
    std::vector<size_t> newcnts(const std::vector<size_t> &cnts) const
    {
        std::vector<size_t> out(pof2);
        for (int i = 0; i < pof2; ++i) {
            const int old_i = real(i);
            out[i] = old_i < 2 * rem ? cnts[old_i] + cnts[old_i - 1] : cnts[old_i];
        }
        return out;
    }
};

// The halving walk.  A rank holds a window [lo, hi) of blocks; a step with
// its partner splits it in the middle: the lower rank of the pair keeps the
// low half and sends the high one, the upper rank the reverse.  Recursive
// halving (partner newrank ^ pof2/2, ^ pof2/4, ...) ends on block newrank,
// the allreduce's and reduce's form (partner newrank ^ 1, ^ 2, ...) on block
// bitrev(newrank): the same walk, only the partner bit differs.  The reverse
// (allgather / gather, partners in the opposite order) sends the window and
// receives its sibling of the same width: above it for the lower rank.
struct Window {
    int lo, hi;
};
struct Step {
    int send_lo, send_hi, recv_lo, recv_hi;
};

inline Step halve(Window *w, bool lower)
{
    const int mid = w->lo + (w->hi - w->lo) / 2;
    const Step st = lower ? Step{mid, w->hi, w->lo, mid} : Step{w->lo, mid, mid, w->hi};
    *w = Window{st.recv_lo, st.recv_hi};
    return st;
}

inline Step regrow(Window *w, bool lower)
{
    const int n = w->hi - w->lo;
    const Step st = lower ? Step{w->lo, w->hi, w->hi, w->hi + n} : Step{w->lo, w->hi, w->lo - n, w->lo};
    *w = lower ? Window{w->lo, w->hi + n} : Window{w->lo - n, w->hi};
    return st;
}

// Slot `slot` of the pull tree of new rank `newrank`: the rank whose block is
// read there, -1 for an absent slot.  Without a fold (rem == 0) there are
// pof2 slots and slot t is new rank newrank ^ t, or newrank ^ bitrev(t) where
// the tree follows recursive halving's decreasing masks.  With one there are
// 2 * pof2: the pair (2t, 2t + 1) is that new rank v's fold -- inout the odd
// rank 2v + 1, in the even 2v -- or v's own input alone.
inline int tree_slots(int pof2, int rem) { return rem ? 2 * pof2 : pof2; }

inline int tree_slot_source(int newrank, int slot, int pof2, int rem, bool bit_reversed)
{
    const int t = rem ? slot / 2 : slot;
    const int v = newrank ^ (bit_reversed ? bitrev(t, pof2) : t);
    if (!rem)
        return v;
    const int j = slot % 2;
    return v < rem ? (j ? 2 * v : 2 * v + 1) : (j ? -1 : v + rem);
}

// True when the multipath recursive halving applies: P a power of two >= 4
// and equal blocks (every rank's half has the same size at every step, so a
// relay knows what it forwards without a size exchange).
inline bool multipath_shape(const std::vector<size_t> &cnts, int size)
{
    if (size < 4 || (size & (size - 1)))
        return false;
    for (size_t n : cnts)
        if (n != cnts[0])
            return false;
    return true;
}

// relay masks of a step with mask m: one of every pair {a, a ^ m}, a != m
// (the smaller), so first hops (r ^ a) and second hops (r ^ a ^ m) together
// use each of the other P - 2 links once
inline std::vector<int> relay_masks(int m, int size)
{
    std::vector<int> A;
    for (int a = 1; a < size; ++a)
        if (a != m && a < (a ^ m))
            A.push_back(a);
    return A;
}

inline size_t multipath_relay_bytes(size_t recvcount, size_t ext, int size)
{
    return (size_t) (size / 2 - 1) * round256(recvcount * ext);
}

// multipath_exchange's cut of D elements into n parts, part j = [lo(j),
// lo(j + 1)), each moved in C chunks: >= 4 MiB each, at most 8 (one when small)
struct PartCut {
    size_t D, n, C;
    PartCut(size_t D_, size_t n_, size_t ext) : D(D_), n(n_)
    {
        C = ((lo(1) - lo(0)) * ext) >> 22;
        C = C < 1 ? 1 : (C > 8 ? 8 : C);
    }
    size_t lo(size_t j) const { return D * j / n; }
    void piece(size_t j, size_t k, size_t *off, size_t *len) const    // chunk k of part j
    {
        const size_t pl = lo(j + 1) - lo(j);
        const size_t a = pl * k / C, b = pl * (k + 1) / C;
        *off = lo(j) + a;
        *len = b - a;
    }
};

// The pipelined pairwise's chunk count for a largest block of maxblk bytes:
// chunks of >= 4 MiB of it, at most 8; below 8 MiB (fewer than two) the plain
// schedule runs.  The count must be the same on every rank (both ends of a
// message cut it alike), so it follows the largest block.  Chunk k of an
// n-element message is [pipe_lo(n, k, nch), pipe_lo(n, k + 1, nch)).
constexpr size_t kPipeChunks = 8;
inline size_t pipe_chunks(size_t maxblk)
{
    const size_t nch = maxblk >> 22;
    return nch > kPipeChunks ? kPipeChunks : nch;
}
inline size_t pipe_lo(size_t n, size_t k, size_t nch) { return n * k / nch; }

// generic.json:277-291 / :316-341: recursive halving below 512 KiB of total
// message, pairwise above (commutative ops)
inline int rs_choose(int algorithm, size_t total_bytes)
{
    if (algorithm != MPIX_RSB_AUTO)
        return algorithm;
    return total_bytes < (512u << 10) ? MPIX_RSB_RECURSIVE_HALVING : MPIX_RSB_PAIRWISE;
}

inline int rsb_choose(int algorithm, size_t recvcount, size_t ext, int size)
{
    return rs_choose(algorithm, recvcount * ext * size);
}

// scratch bytes of a schedule: total = all ranks' elements, mine = this
// rank's result elements
inline size_t rs_workspace(size_t total, size_t mine, size_t ext, int size, int algo)
{
    if (size == 1)
        return 0;
    switch (algo) {
        case MPIX_RSB_RECURSIVE_HALVING:
            return 2 * round256(total * ext);
        case MPIX_RSB_RECURSIVE_HALVING_MULTIPATH:   // + the relay slots (total = size * mine)
            return 2 * round256(total * ext) +
                   (total == mine * (size_t) size ? multipath_relay_bytes(mine, ext, size) : 0);
        case MPIX_RSB_PAIRWISE:
        case MPIX_RSB_PAIRWISE_PIPELINED:
            return (size - 1) * round256(mine * ext);
        case MPIX_RSB_PAIRWISE_SEQUENTIAL:
            return round256(mine * ext);
        case MPIX_RSB_RECURSIVE_HALVING_PULL:       // P > 16 runs RECURSIVE_HALVING
            return size > 16 ? 2 * round256(total * ext) : 0;
        default:
            return 0;
    }
}

inline size_t rsb_workspace(size_t recvcount, size_t ext, int size, int algo)
{
    return rs_workspace(recvcount * size, recvcount, ext, size, algo);
}

// MPI_Reduce: tmp_buf, plus the accumulator a non-root rank has no recvbuf for
inline size_t reduce_workspace(size_t nb, bool is_root)
{
    return round256(nb) + (is_root ? 0 : round256(nb));
}

}  // namespace coll_sched

#endif
