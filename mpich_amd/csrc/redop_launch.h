// redop_launch.h -- what a launcher of redop_kernels.h decides before it
// launches: which kernel form runs, on which grid and block, with which head /
// packets / tail split.  Pure host C++17: no HIP include, no device code, so
// tests/c/launch_plan_check.cpp replays every decision on the CPU against
// tests/golden/launch_plans.json.  The compile-time facts of an instantiation
// unit come in as LaunchFacts (the .hip side passes its own macros; this
// header reads none of them).
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace mpix {

// Runtime parameters some combiners need (Fortran .TRUE./.FALSE.,
// src/include/mpii_fortlogical.h:15,28), and the completion word of a
// synchronous call: when `done` is set, the contiguous launcher guarantees
// that done_seq is stored to it once the combine is complete and visible to
// the host -- by the kernel itself when it runs as at most kSignalMaxGrid
// workgroups (the last one to finish, counted on done_ctr, stores it: no
// end-of-kernel + stream-packet round trip), else by a stream write after it.
struct Params {
    long long ftrue;
    long long ffalse;
    uint32_t *done = nullptr;       // pinned, fine-grained host word
    uint32_t *done_ctr = nullptr;   // device word, 0 between launches
    uint32_t done_seq = 0;
    // blocks from this index on store write-through (sc0 sc1: the line leaves
    // the XCD's L2 at once instead of staying dirty until the end-of-kernel
    // write-back); 0xffffffff = none (LaunchCfg::wt_tail)
    uint32_t wt_from = 0xffffffffu;
    uint32_t wt_every = 0;      // and blocks b with b % wt_every == wt_phase (0 = none)
    uint32_t wt_phase = 0;
    uint32_t wt_xcd = 0;        // and every block running on an XCD whose bit is set
    // split combiners (is_split, redop_kernels.h): one 64-bit word per 64
    // units, bit j set when unit 64 w + j left its fast path (fixup_acquire)
    uint64_t *fixup = nullptr;
};

struct LaunchCfg {
    int block;          // threads per block (multiple of 64)
    int max_grid;       // 0 = no cap (one tile per block)
    int wt_tail;        // contiguous kernel: the last wt_tail blocks store write-through
    int wt_every;       // ... and blocks b with b % wt_every == wt_phase
    int wt_phase;
    int wt_xcd;         // ... and blocks on the XCDs (HW_REG_XCC_ID) of this bit mask
};

// Most blocks one dispatch of `block`-thread workgroups may have: HIP caps a
// dispatch at UINT32_MAX work-items (gridDim.x * blockDim.x), so with one-wave
// blocks that is 2^26 - 1 blocks, not 2^31.  Every kernel
// launched through grid_for strides over the rest.
constexpr uint64_t max_blocks(uint64_t block)
{
    return 0xffffffffull / (block ? block : 1);
}

inline unsigned grid_for(uint64_t work_per_block_units, uint64_t n, int max_grid, uint64_t block)
{
    uint64_t g = (n + work_per_block_units - 1) / work_per_block_units;
    if (g == 0)
        g = 1;
    if (max_grid > 0 && g > (uint64_t) max_grid)
        g = (uint64_t) max_grid;
    if (g > max_blocks(block))
        g = max_blocks(block);
    return (unsigned) g;
}

// The store policy (LaunchCfg::wt_*) of a launch of `grid` blocks.
inline void set_store_policy(Params &p, const LaunchCfg &cfg, unsigned grid)
{
    if (cfg.wt_tail > 0)
        p.wt_from = grid > (unsigned) cfg.wt_tail ? grid - (unsigned) cfg.wt_tail : 0u;
    p.wt_every = cfg.wt_every > 0 ? (unsigned) cfg.wt_every : 0u;
    p.wt_phase = (unsigned) cfg.wt_phase;
    p.wt_xcd = (unsigned) cfg.wt_xcd & 0xffu;
}

// What an instantiation unit was compiled with: is_split<C>, MPIX_REDOP_UNROLL,
// MPIX_REDOP_UNROLL32, MPIX_REDOP_BLOCK32, MPIX_REDOP_VBLOCK, kSignalMaxGrid,
// kMultiLds.
struct LaunchFacts {
    bool is_split;
    unsigned unroll, unroll32, block32, vblock, signal_max_grid, multi_lds;
};

// The split of `count` units of `unit` <= 16 bytes by the target's 16-byte
// phase: `head` elements up to the first 16-byte boundary of the target, npk
// packets of 16 / unit elements, ntail elements from tail_start on.  Every
// packet kernel and every batch segment is split by this one function, so a
// segment's bits are those of a call of its own.  Units are powers of two, so
// nothing here divides: a launcher's host time is a few hundred nanoseconds.
struct PacketSplit {
    uint64_t head, npk, tail_start;
    uint32_t ntail;
};

inline PacketSplit packet_split(uintptr_t target, uint64_t count, unsigned unit)
{
    const unsigned lg = (unsigned) __builtin_ctz(unit);     // a packet has E = 16 >> lg elements
    uint64_t head = ((16 - (target & 15)) & 15) >> lg;
    if (head > count)
        head = count;
    const uint64_t npk = (count - head) >> (4 - lg);
    const uint64_t tail_start = head + (npk << (4 - lg));
    return PacketSplit{head, npk, tail_start, (uint32_t) (count - tail_start)};
}

// whether every address is a multiple of `unit`
inline bool on_grid(unsigned unit, uintptr_t a, uintptr_t b = 0, uintptr_t c = 0)
{
    return ((a | b | c) & (unit - 1)) == 0;
}

enum class Form : uint8_t {
    // contiguous (and multi-input: PacketsAin / Elem) forms
    PacketsAin,         // 16-byte packets, `in` on the target's phase
    PacketsUin,         // ... `in` only element-aligned (unaligned packet loads)
    Elem,               // element-wise grid-stride
    Packets32,          // 32-byte units, both operands 16-byte aligned (k_contig32)
    // vector target
    VectorS2,           // (bl, st) = (1, 2), the target on the 2 x unit grid
    Vector1,            // bl == 1
    Vector,
    // tree fold: KMAX slots x packets per lane
    Tree2x2,
    Tree4x2,
    Tree8x1,
    Tree16x1,
    TreeElem,
    TreePair32,         // out = slot 0 OP slot 1 on 32-byte units (k_contig32)
    // fused get-accumulate
    GetaccAligned,      // origin and result on the target's phase
    GetaccUnaligned,
    GetaccElem,
};

struct LaunchPlan {
    Form form;
    bool signals;       // the kernel itself stores the completion word
    unsigned grid, block;
    uint32_t lds;       // dynamic LDS bytes
    uint32_t pres;      // tree: the slots that hold an operand
    PacketSplit split;  // the packet forms'; zero for the others
};

namespace plan_detail {
inline LaunchPlan elem(Form form, uint64_t n, const LaunchCfg &cfg)
{
    return LaunchPlan{form, false, grid_for((uint64_t) cfg.block * 4, n, cfg.max_grid, cfg.block),
                      (unsigned) cfg.block, 0, 0, PacketSplit{}};
}
// k_contig32: one tile of block32 x unroll32 units per block
inline LaunchPlan packets32(Form form, uint64_t count, const LaunchCfg &cfg, const LaunchFacts &f)
{
    return LaunchPlan{form, false,
                      grid_for((uint64_t) f.block32 * f.unroll32, count, cfg.max_grid, f.block32),
                      f.block32, 0, 0, PacketSplit{}};
}
}  // namespace plan_detail

// launch_contig.  32-byte units (the long double / binary128 pairs and
// complex): packets when both operands are on the 16-byte grid, else
// element-wise.  Smaller units: packets whenever both operands are
// element-aligned, `in` read with unaligned loads when it is off the target's
// phase.  Up to signal_max_grid workgroups with a counter word (one without)
// store the completion word themselves.
inline LaunchPlan plan_contig(uintptr_t ai, uintptr_t ao, unsigned unit, uint64_t count,
                              const LaunchCfg &cfg, const LaunchFacts &f, bool done, bool done_ctr)
{
    if (unit > 16)
        return ((ai | ao) & 15) == 0 ? plan_detail::packets32(Form::Packets32, count, cfg, f)
                                     : plan_detail::elem(Form::Elem, count, cfg);
    if (!on_grid(unit, ai, ao))
        return plan_detail::elem(Form::Elem, count, cfg);
    LaunchPlan p{};
    p.form = (ai & 15) == (ao & 15) ? Form::PacketsAin : Form::PacketsUin;
    p.split = packet_split(ao, count, unit);
    p.block = (unsigned) cfg.block;
    p.grid = grid_for((uint64_t) cfg.block * f.unroll, p.split.npk, cfg.max_grid, cfg.block);
    p.signals = done && p.grid <= (done_ctr ? f.signal_max_grid : 1u);
    return p;
}

// launch_multi: packets (one per lane per input) when the target is
// element-aligned and every input shares its 16-byte phase, else element-wise.
// k >= 2 inputs: unused LDS of multi_lds bytes per 64 threads caps the waves
// per SIMD, unless that would pass 64 KiB per block (kMultiLds, redop_kernels.h)
inline LaunchPlan plan_multi(const uintptr_t *ins, int k, uintptr_t ao, unsigned unit,
                             uint64_t count, const LaunchCfg &cfg, const LaunchFacts &f)
{
    bool aligned = unit <= 16 && on_grid(unit, ao);
    for (int q = 0; q < k; ++q)
        aligned = aligned && (ins[q] & 15) == (ao & 15);
    if (!aligned)
        return plan_detail::elem(Form::Elem, count, cfg);
    LaunchPlan p{};
    p.form = Form::PacketsAin;
    p.split = packet_split(ao, count, unit);
    p.block = (unsigned) cfg.block;
    p.grid = grid_for((uint64_t) cfg.block, p.split.npk, cfg.max_grid, cfg.block);
    if (k >= 2) {
        const uint64_t lds = (uint64_t) f.multi_lds * ((unsigned) cfg.block / 64u);
        p.lds = lds > 65536 ? 0 : (uint32_t) lds;
    }
    return p;
}

// launch_tree: a zero slot is absent (it has no say in the form).  32-byte
// units: out = slot 0 OP slot 1, all three 16-byte aligned, is k_contig32 with
// slot 0 in the inout role (recursive halving's combine_to); not for a split
// combiner whose output is slot 1: k_contig32 stores the inout role's value
// (slot 0's) into every unit it declines, and k_fixup32 would then read that
// where it expects slot 1's (out over slot 0 stores slot 0's value over
// itself).  Other shapes, and slots off the output's phase, go element-wise.
// Packets in one-wave blocks without a grid cap, the form by slot count: a k
// between 2, 4, 8, 16 runs the next larger form, whose uniform branches skip
// the slots >= k (the measurements: redop_kernels.h, launch_tree).
constexpr unsigned kTreeBlock = 64;

inline LaunchPlan plan_tree(const uintptr_t *ins, int k, uintptr_t ao, unsigned unit,
                            uint64_t count, const LaunchCfg &cfg, const LaunchFacts &f)
{
    bool aligned = unit <= 16 && on_grid(unit, ao);
    uint32_t pres = 0;
    for (int q = 0; q < k; ++q) {
        if (!ins[q])
            continue;
        pres |= 1u << q;
        aligned = aligned && (ins[q] & 15) == (ao & 15);
    }
    LaunchPlan p{};
    if (unit > 16 && k == 2 && pres == 3u && !(f.is_split && ao == ins[1]) &&
        ((ao | ins[0] | ins[1]) & 15) == 0) {
        p = plan_detail::packets32(Form::TreePair32, count, cfg, f);
    } else if (aligned) {
        p.form = k <= 2 ? Form::Tree2x2 : k <= 4 ? Form::Tree4x2 : k <= 8 ? Form::Tree8x1
                                                                          : Form::Tree16x1;
        p.split = packet_split(ao, count, unit);
        p.block = kTreeBlock;
        p.grid = grid_for(k <= 4 ? kTreeBlock * 2 : kTreeBlock, p.split.npk, 0, kTreeBlock);
    } else {
        p.form = Form::TreeElem;
        p.block = 256;
        p.grid = grid_for(256 * 4, count, 0, 256);
    }
    p.pres = pres;
    return p;
}

// launch_vector over n = count * bl > 0 packed elements: bl == st is
// contiguous after all (plan_contig's forms); (1, 2) goes to k_vector_s2, which
// loads {payload, gap} as one 2 x unit word, only on a target aligned to that
// word, in vblock-thread blocks.
inline LaunchPlan plan_vector(uintptr_t ai, uintptr_t ao, unsigned unit, uint64_t n, uint64_t bl,
                              uint64_t st, const LaunchCfg &cfg, const LaunchFacts &f, bool done,
                              bool done_ctr)
{
    if (bl == st)
        return plan_contig(ai, ao, unit, n, cfg, f, done, done_ctr);
    if (unit <= 16 && bl == 1 && st == 2 && on_grid(2 * unit, ao))
        return LaunchPlan{Form::VectorS2, false, grid_for(f.vblock, n, cfg.max_grid, f.vblock),
                          f.vblock, 0, 0, PacketSplit{}};
    return plan_detail::elem(bl == 1 ? Form::Vector1 : Form::Vector, n, cfg);
}

// launch_getacc: packets (one per lane) when origin, result and target are
// element-aligned, origin and result through unaligned 16-byte accesses unless
// both share the target's phase; 32-byte units element-wise.
inline LaunchPlan plan_getacc(uintptr_t ai, uintptr_t ar, uintptr_t ao, unsigned unit,
                              uint64_t count, const LaunchCfg &cfg)
{
    if (unit > 16 || !on_grid(unit, ai, ar, ao))
        return plan_detail::elem(Form::GetaccElem, count, cfg);
    LaunchPlan p{};
    p.form = (ai & 15) == (ao & 15) && (ar & 15) == (ao & 15) ? Form::GetaccAligned
                                                              : Form::GetaccUnaligned;
    p.split = packet_split(ao, count, unit);
    p.block = (unsigned) cfg.block;
    p.grid = grid_for((uint64_t) cfg.block, p.split.npk, cfg.max_grid, cfg.block);
    return p;
}

// launch_batch: the segments packed into as few k_batch (units <= 16 bytes,
// cfg.block threads, tiles of block x unroll packets) or k_batch32 (block32
// threads, tiles of block32 x unroll32 units) launches as hold them, each
// segment owning one block per tile from blk0 on.  next() yields, in order,
//   Own    segment i as a call of its own (launch_contig): operands off the
//          element grid (32-byte units: off the 16-byte grid), more tiles than
//          one grid holds, and every segment of a split combiner;
//   Seg    segment i in table slot n at block blk0, with its split (32-byte
//          units: npk = its units) and whether `in` shares the target's phase;
//   Flush  launch the n segments packed so far as `blocks` blocks (before a
//          segment that would pass max_blocks, and at the end); a Seg's
//          `blocks` are its own.
// Segments of zero count are skipped.
struct BatchStep {
    enum Kind : uint8_t { Own, Seg, Flush } kind;
    bool ain;
    int i, n;
    uint32_t blk0;
    uint64_t blocks;
    PacketSplit split;
};

class BatchPacker {
public:
    BatchPacker(const uintptr_t *ins, const uintptr_t *ios, const uint64_t *counts, int k,
                unsigned unit, const LaunchCfg &cfg, const LaunchFacts &f)
        : ins_(ins), ios_(ios), counts_(counts), k_(k), unit_(unit), split_(f.is_split),
          block_(unit > 16 ? f.block32 : (unsigned) cfg.block),
          tile_((uint64_t) block_ * (unit > 16 ? f.unroll32 : f.unroll))
    {
    }

    unsigned block() const { return block_; }

    // inlined into the launcher's loop: with the unit a constant there, a
    // step costs what the launcher's own loop body did
    __attribute__((always_inline)) bool next(BatchStep &st)
    {
        for (; i_ < k_; ++i_) {
            const uint64_t count = counts_[i_];
            if (!count)
                continue;
            const uintptr_t ai = ins_[i_], ao = ios_[i_];
            PacketSplit sp{0, count, count, 0};     // 32-byte units
            bool own = split_, ain = true;
            own = own || !on_grid(unit_ > 16 ? 16 : unit_, ai, ao);
            if (unit_ <= 16 && !own) {
                sp = packet_split(ao, count, unit_);
                ain = (ai & 15) == (ao & 15);
            }
            uint64_t nb = (sp.npk + tile_ - 1) / tile_;
            if (nb == 0)
                nb = 1;     // a segment of head / tail elements only
            if (own || nb > max_blocks(block_)) {
                st = BatchStep{BatchStep::Own, false, i_++, 0, 0, 0, PacketSplit{}};
                return true;
            }
            if (blocks_ + nb > max_blocks(block_))
                return flush(st);       // then this segment again, at block 0
            st = BatchStep{BatchStep::Seg, ain, i_++, n_++, (uint32_t) blocks_, nb, sp};
            blocks_ += nb;
            return true;
        }
        return n_ ? flush(st) : false;
    }

private:
    bool flush(BatchStep &st)
    {
        st = BatchStep{BatchStep::Flush, false, 0, n_, 0, blocks_, PacketSplit{}};
        n_ = 0;
        blocks_ = 0;
        return true;
    }

    const uintptr_t *ins_, *ios_;
    const uint64_t *counts_;
    int k_;
    unsigned unit_;
    bool split_;
    unsigned block_;
    uint64_t tile_;
    int i_ = 0, n_ = 0;
    uint64_t blocks_ = 0;
};

}  // namespace mpix
