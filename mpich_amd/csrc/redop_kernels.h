// redop_kernels.h -- streaming kernels for the local reduction (gfx950).
//
// The combine is a pure HBM stream: per element 2 loads + 1 store and O(1)
// integer/fp work, so the kernels are built around the memory system, not
// the ALUs (no MFMA, no LDS on the contiguous path):
//   * both operands are read as 16-byte packets (global_load_dwordx4), each
//     lane keeping MPIX_REDOP_UNROLL packets per operand in flight before the
//     first combine, so a 256-thread block has 256*U*32 B outstanding (U = 1
//     since round 5: the latency is covered by waves, not by each wave's
//     loads -- 8 waves per SIMD at 1 GiB fp32 SUM ran 4.0 % faster than U = 4,
//     every config-3 row 2.8-8.2 % faster; tools/contig_u_probe.hip,
//     tools/gpu_u_ab.sh, profiles/r05_unroll_ab.json);
//   * inout is written back with 16-byte stores to the lines it just read;
//   * each packet holds 16/sizeof(unit) elements, combined in registers;
//   * elements before the first 16-byte boundary of inout (head) and after
//     the last full packet (tail) are done element-wise by block 0;
//   * if in and inout disagree modulo 16 bytes, `in` is read with unaligned
//     16-byte loads (gfx950 global loads take element-aligned addresses);
//     only buffers that are not even element-aligned fall back to an
//     element-wise grid-stride kernel.
// Launch geometry: one tile of blockDim*U packets per block, grid =
// ceil(npk / tile) (optionally capped, then grid-stride).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "redop_ops.h"

#ifndef MPIX_REDOP_UNROLL
#define MPIX_REDOP_UNROLL 1
#endif
#ifndef MPIX_REDOP_UNROLL32
// 32-byte units: 64-unit runs per lane per operand -- one since round 5 (two
// before): C_LONG_DOUBLE_COMPLEX and COMPLEX32 SUM +6-7 %, the pair types'
// MINLOC / MAXLOC and the complex PROD even (tools/gpu_u_ab.sh,
// profiles/r05_unroll32_ab.json)
#define MPIX_REDOP_UNROLL32 1
#endif
#ifndef MPIX_REDOP_NT_LOAD
#define MPIX_REDOP_NT_LOAD 1
#endif
#ifndef MPIX_REDOP_NT_STORE
#define MPIX_REDOP_NT_STORE 1
#endif
#ifndef MPIX_REDOP_GROUPED_LOADS
#define MPIX_REDOP_GROUPED_LOADS 1
#endif

namespace mpix {

typedef unsigned int v4u __attribute__((ext_vector_type(4)));

template <bool NT> __device__ __forceinline__ v4u ld16(const v4u *p)
{
    if constexpr (NT)
        return __builtin_nontemporal_load(p);
    else
        return *p;
}

template <bool NT> __device__ __forceinline__ void st16(v4u *p, v4u v)
{
    if constexpr (NT)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}

// the XCD this wave runs on (0-7; a hardware register, read-only)
__device__ __forceinline__ unsigned xcc_id()
{
    unsigned x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
    return x;
}

// write-through 16-byte store (global_store_dwordx4 ... sc0 sc1)
__device__ __forceinline__ void st16_wt(v4u *p, v4u v)
{
    typedef __attribute__((address_space(1))) v4u gv4u;
    *(volatile gv4u *) (gv4u *) p = v;
}

// the store policy of this block (Params::wt_*): write-through or not,
// uniform per block
__device__ __forceinline__ bool wt_block(const Params &prm)
{
    bool wt = blockIdx.x >= prm.wt_from ||
              (prm.wt_every && blockIdx.x % prm.wt_every == prm.wt_phase);
    if (prm.wt_xcd)
        wt = wt || ((prm.wt_xcd >> (xcc_id() & 7)) & 1);
    return wt;
}

template <bool NT> __device__ __forceinline__ void st16_pol(v4u *p, v4u v, bool wt)
{
    if (wt)
        st16_wt(p, v);
    else
        st16<NT>(p, v);
}

// 16-byte load from an address that is only element-aligned: gfx950 global
// loads accept unaligned addresses, so this is still one global_load_dwordx4.
__device__ __forceinline__ v4u ld16u(const char *p)
{
    v4u v;
    __builtin_memcpy(&v, p, 16);
    return v;
}

// 1-byte combiners may provide apply4(dword, dword): four elements at once
template <class C, class = void> struct HasApply4 {
    static constexpr bool value = false;
};
template <class C>
struct HasApply4<C, decltype((void) C::apply4(0u, 0u))> {
    static constexpr bool value = sizeof(typename C::unit) == 1;
};

// ... or apply4p(dword, dword, prm) when they need the runtime parameters
template <class C, class = void> struct HasApply4P {
    static constexpr bool value = false;
};
template <class C>
struct HasApply4P<C, decltype((void) C::apply4p(0u, 0u, *(const Params *) nullptr))> {
    static constexpr bool value = sizeof(typename C::unit) == 1;
};

template <class C> __device__ __forceinline__ v4u combine16(v4u a, v4u b, const Params &prm)
{
    if constexpr (HasApply4P<C>::value) {
        v4u r;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            r[e] = C::apply4p(a[e], b[e], prm);
        return r;
    }
    if constexpr (HasApply4<C>::value) {
        v4u r;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            r[e] = C::apply4(a[e], b[e]);
        return r;
    }
    using T = typename C::unit;
    constexpr int E = 16 / sizeof(T);
    struct alignas(16) Pk { T u[E]; };
    static_assert(sizeof(Pk) == 16, "unit must divide 16 bytes");
    Pk pa = __builtin_bit_cast(Pk, a);
    Pk pb = __builtin_bit_cast(Pk, b);
#pragma unroll
    for (int e = 0; e < E; ++e)
        pa.u[e] = C::apply(pa.u[e], pb.u[e], prm);
    return __builtin_bit_cast(v4u, pa);
}

// AIN: `in` has the same 16-byte phase as `io` (packet loads); otherwise it
// is only element-aligned and its packets are read with unaligned loads
// (still one dwordx4 per lane; the lines are shared with the neighbours').
// GRP: issue all U `inout` packet loads, then all U `in` loads (instead of
// alternating them per packet)
// The body of one contiguous combine as block `bid` of `nblk` (k_contig: the
// launch's own block; k_batch: a block of its segment).
template <class C, int U, bool NTL, bool NTS, bool AIN, bool GRP>
__device__ __forceinline__ void
contig_body(const typename C::unit *__restrict__ in, typename C::unit *__restrict__ io,
            uint64_t head, uint64_t npk, uint64_t tail_start, uint32_t ntail, const Params &prm,
            uint64_t bid, uint64_t nblk, uint64_t nt)
{
    const v4u *__restrict__ vin = reinterpret_cast<const v4u *>(in + head);
    const char *__restrict__ cin = reinterpret_cast<const char *>(in + head);
    v4u *__restrict__ vio = reinterpret_cast<v4u *>(io + head);
    const uint64_t tile = nt * U;
    const uint64_t stride = nblk * tile;
    auto ldin = [&](uint64_t k) -> v4u {
        if constexpr (AIN)
            return ld16<NTL>(vin + k);
        else
            return ld16u(cin + 16 * k);
    };
    const bool wt = wt_block(prm);
    auto st = [&](v4u *p, v4u v) { st16_pol<NTS>(p, v, wt); };
    for (uint64_t i = bid * tile + threadIdx.x; i < npk; i += stride) {
        if (i + (U - 1) * nt < npk) {
            v4u a[U], b[U];
            if constexpr (GRP) {
#pragma unroll
                for (int u = 0; u < U; ++u)
                    a[u] = ld16<NTL>(vio + i + u * nt);
#pragma unroll
                for (int u = 0; u < U; ++u)
                    b[u] = ldin(i + u * nt);
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    a[u] = ld16<NTL>(vio + i + u * nt);
                    b[u] = ldin(i + u * nt);
                }
            }
            // every load of the tile is issued before the first combine: left
            // alone, the scheduler sinks the last loads of the wider combiners
            // (1-byte ints, fp16 complex) below the first packet's combine, so
            // fewer bytes are in flight per wave (tools/isa_seq.py)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < U; ++u)
                st(vio + i + u * nt, combine16<C>(a[u], b[u], prm));
        } else {
            for (int u = 0; u < U; ++u) {
                uint64_t k = i + u * nt;
                if (k < npk)
                    st16<NTS>(vio + k, combine16<C>(ld16<NTL>(vio + k), ldin(k), prm));
            }
        }
    }
    if (bid == 0) {
        for (uint64_t t = threadIdx.x; t < head; t += nt)
            io[t] = C::apply(io[t], in[t], prm);
        for (uint64_t t = threadIdx.x; t < ntail; t += nt)
            io[tail_start + t] = C::apply(io[tail_start + t], in[tail_start + t], prm);
    }
}

// The grid and block sizes come in as arguments (nblk, nt): a kernel that
// reads gridDim / blockDim gets the runtime's hidden-argument block appended
// to its kernel arguments (360 instead of 112 bytes here), which the host
// writes on every launch.
template <class C, int U, bool NTL, bool NTS, bool AIN = true, bool GRP = MPIX_REDOP_GROUPED_LOADS>
__global__ void __launch_bounds__(1024)
k_contig(const typename C::unit *__restrict__ in, typename C::unit *__restrict__ io,
         uint64_t head, uint64_t npk, uint64_t tail_start, uint32_t ntail, Params prm,
         uint32_t nblk, uint32_t nt)
{
    contig_body<C, U, NTL, NTS, AIN, GRP>(in, io, head, npk, tail_start, ntail, prm, blockIdx.x,
                                          nblk, nt);
    if (prm.done) {     // small synchronous call (launch_contig sets it)
        __threadfence();            // every wave: its stores complete
        __syncthreads();
        if (threadIdx.x == 0) {
            bool last = true;
            if (nblk > 1) {         // the last workgroup to arrive signals
                last = atomicAdd(prm.done_ctr, 1u) == nblk - 1;
                if (last)
                    *prm.done_ctr = 0;
            }
            if (last) {
                __threadfence_system();     // L2 written back for the host
                __hip_atomic_store(prm.done, prm.done_seq, __ATOMIC_RELEASE,
                                   __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// Batch of independent contiguous combines in one launch
// (MPIX_Reduce_local_batch_async): segment s owns blocks [blk0, blk0 + nblk)
// of the grid, one tile each, laid out exactly as a k_contig launch of that
// segment alone would lay them out (same head / packets / tail split, same
// per-element combine), so the bits are those of one call per segment.
constexpr int kMaxBatch = kMaxBatchSegs;
struct BatchSeg {
    const void *in;
    void *io;
    uint64_t npk;
    uint8_t head, ntail, ain, pad[5];
};
struct BatchTab {
    uint32_t blk0[kMaxBatch];   // first block of each segment, ascending, blk0[0] = 0
    BatchSeg s[kMaxBatch];
};
static_assert(kMaxBatch <= 64, "one wave looks the segment up");

template <class C, int U, bool NTL, bool NTS>
__global__ void __launch_bounds__(1024)
k_batch(BatchTab tab, int nseg, Params prm, uint32_t nblk, uint32_t nt)
{
    using T = typename C::unit;
    constexpr uint64_t E = 16 / sizeof(T);
    const uint32_t b = blockIdx.x;
    // the segment of this block, the last with blk0 <= b: lane i of every
    // wave reads blk0[i], one ballot counts them (no serial scan of the table)
    const uint32_t lane = threadIdx.x & 63;
    const bool le = lane < (uint32_t) nseg && tab.blk0[lane] <= b;
    const int q = __popcll(__ballot(le)) - 1;
    const BatchSeg &g = tab.s[q];
    const uint32_t first = tab.blk0[q];
    const uint32_t next = q + 1 < nseg ? tab.blk0[q + 1] : nblk;
    const T *in = static_cast<const T *>(g.in);
    T *io = static_cast<T *>(g.io);
    const uint64_t tail_start = g.head + g.npk * E;
    if (g.ain)
        contig_body<C, U, NTL, NTS, true, MPIX_REDOP_GROUPED_LOADS>(
            in, io, g.head, g.npk, tail_start, g.ntail, prm, b - first, next - first, nt);
    else
        contig_body<C, U, NTL, NTS, false, MPIX_REDOP_GROUPED_LOADS>(
            in, io, g.head, g.npk, tail_start, g.ntail, prm, b - first, next - first, nt);
}

// Multi-input combine: inout = OP(...OP(OP(inout, in[0]), in[1])..., in[k-1]),
// i.e. k back-to-back MPIR_Reduce_local calls in that order -- the same
// association, so the same bits -- in ONE pass over HBM: (k+2) x bytes
// instead of 3k x bytes.  Used by the pairwise reduce-scatter, whose k
// received blocks arrive together.
constexpr int kMaxMulti = 16;
template <typename T> struct MultiIn {
    const T *p[kMaxMulti];
};

template <class C, int U>
__global__ void __launch_bounds__(1024)
k_contig_multi(MultiIn<typename C::unit> ins, int k, typename C::unit *__restrict__ io,
               uint64_t head, uint64_t npk, uint64_t tail_start, uint32_t ntail, Params prm,
               uint32_t nblk, uint32_t nthreads)
{
    v4u *__restrict__ vio = reinterpret_cast<v4u *>(io + head);
    const uint64_t nt = nthreads;
    const uint64_t tile = nt * U;
    const uint64_t stride = (uint64_t) nblk * tile;
    const bool wt = wt_block(prm);
    // one input packet live beside the accumulator: input q is loaded, then
    // combined, then input q + 1 (round 6; the round-5 form loaded q + 1
    // before combining q, and its copy forced a full wait anyway), with the
    // launch capping the waves per SIMD (launch_multi, kMultiLds)
    // (tools/multi_fold_probe.hip, profiles/r06_multi_fold_caps2.json)
    for (uint64_t i = (uint64_t) blockIdx.x * tile + threadIdx.x; i < npk; i += stride) {
        v4u acc[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (i + u * nt < npk)
                acc[u] = ld16<true>(vio + i + u * nt);
        for (int q = 0; q < k; ++q) {
            const v4u *__restrict__ vin = reinterpret_cast<const v4u *>(ins.p[q] + head);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (i + u * nt < npk)
                    acc[u] = combine16<C>(acc[u], ld16<true>(vin + i + u * nt), prm);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (i + u * nt < npk)
                st16_pol<true>(vio + i + u * nt, acc[u], wt);
    }
    if (blockIdx.x == 0) {
        for (uint64_t t = threadIdx.x; t < head; t += nt) {
            typename C::unit a = io[t];
            for (int q = 0; q < k; ++q)
                a = C::apply(a, ins.p[q][t], prm);
            io[t] = a;
        }
        for (uint64_t t = threadIdx.x; t < ntail; t += nt) {
            typename C::unit a = io[tail_start + t];
            for (int q = 0; q < k; ++q)
                a = C::apply(a, ins.p[q][tail_start + t], prm);
            io[tail_start + t] = a;
        }
    }
}

template <class C>
__global__ void __launch_bounds__(1024)
k_elem_multi(MultiIn<typename C::unit> ins, int k, typename C::unit *__restrict__ io, uint64_t n,
             Params prm, uint32_t nblk, uint32_t nt)
{
    const uint64_t stride = (uint64_t) nblk * nt;
    for (uint64_t i = (uint64_t) blockIdx.x * nt + threadIdx.x; i < n; i += stride) {
        typename C::unit a = io[i];
        for (int q = 0; q < k; ++q)
            a = C::apply(a, ins.p[q][i], prm);
        io[i] = a;
    }
}

// Tree combine: k = 2^L slots folded pairwise by levels, level m = 1, 2, 4,
// ...: slot s (bit m clear) = OP(inout = slot s, in = slot s + m), result =
// slot 0, written to `out` (which may be slot 0's buffer).  With the slots
// holding the peers of rank r in the order r ^ bitrev(s) this is the
// recursive-halving association of rank r's block (…recursive_halving.c:
// 164-229: each step the partner's partial is `in`, the own partial
// `inout`), computed in one pass that reads the k blocks (over xGMI for the
// peers') and writes one.  `pres` marks the slots that hold an operand: an
// absent slot's partner passes through unchanged (the reference's fold of a
// non-power-of-two world, where half of the first level has no partner).
// Unused slots (s >= k) are compile-time registers whose loads and combines
// are skipped by uniform branches, so one instantiation serves every k.
template <int KMAX, class V, class F>
__device__ __forceinline__ void tree_fold(V *v, int k, uint32_t pres, F f)
{
#pragma unroll
    for (int m = 1; m < KMAX; m <<= 1) {
#pragma unroll
        for (int q = 0; q < KMAX; q += 2 * m)
            if (q + m < k) {
                const bool a = (pres >> q) & 1u, b = (pres >> (q + m)) & 1u;
                if (a && b)
                    v[q] = f(v[q], v[q + m]);
                else if (b)
                    v[q] = v[q + m];
            }
        pres |= pres >> m;
    }
}

template <class C, int KMAX, int U>
__global__ void __launch_bounds__(256)
k_contig_tree(MultiIn<typename C::unit> ins, int k, uint32_t pres, typename C::unit *__restrict__ out,
              uint64_t head, uint64_t npk, uint64_t tail_start, uint32_t ntail, Params prm)
{
    using T = typename C::unit;
    v4u *vout = reinterpret_cast<v4u *>(out + head);
    // gridDim / blockDim kept here: the same kernel with the sizes as
    // arguments measured 2.5 % slower at k = 4 and 8 (tools/multi_probe.py)
    const uint64_t nt = blockDim.x;
    const uint64_t stride = (uint64_t) gridDim.x * nt * U;
    auto cv = [&](v4u a, v4u b) { return combine16<C>(a, b, prm); };
    auto ce = [&](T a, T b) { return C::apply(a, b, prm); };
    const bool wt = wt_block(prm);
    for (uint64_t i = (uint64_t) blockIdx.x * nt * U + threadIdx.x; i < npk; i += stride) {
        v4u v[U][KMAX];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int q = 0; q < KMAX; ++q)
                if (q < k && ((pres >> q) & 1u) && i + u * nt < npk)
                    v[u][q] = ld16<true>(reinterpret_cast<const v4u *>(ins.p[q] + head) + i + u * nt);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (i + u * nt >= npk)
                continue;
            tree_fold<KMAX>(v[u], k, pres, cv);
            st16_pol<true>(vout + i + u * nt, v[u][0], wt);
        }
    }
    if (blockIdx.x == 0) {
        auto one = [&](uint64_t t) {
            T v[KMAX];
#pragma unroll
            for (int q = 0; q < KMAX; ++q)
                if (q < k && ((pres >> q) & 1u))
                    v[q] = ins.p[q][t];
            tree_fold<KMAX>(v, k, pres, ce);
            out[t] = v[0];
        };
        for (uint64_t t = threadIdx.x; t < head; t += nt)
            one(t);
        for (uint64_t t = threadIdx.x; t < ntail; t += nt)
            one(tail_start + t);
    }
}

// The same fold as a compile-time recursion over slot ranges [LO, LO + LEN):
// left half = inout, right half = in, an absent half passes the other through
// -- tree_fold's association exactly, with at most log2(KMAX) + 1 partial
// results live instead of KMAX slots (the 32-byte units would not fit the
// registers otherwise).  Returns whether any slot of the range is present.
template <int LO, int LEN, class T, class L, class F>
__device__ __forceinline__ bool tree_fold_rec(T &out, int k, uint32_t pres, L &load, F &f)
{
    if constexpr (LEN == 1) {
        if (LO < k && ((pres >> LO) & 1u)) {
            out = load(LO);
            return true;
        }
        return false;
    } else {
        T a, b;
        const bool ha = tree_fold_rec<LO, LEN / 2>(a, k, pres, load, f);
        if (LO + LEN / 2 >= k) {
            out = a;
            return ha;
        }
        const bool hb = tree_fold_rec<LO + LEN / 2, LEN / 2>(b, k, pres, load, f);
        out = (ha && hb) ? f(a, b) : (hb ? b : a);
        return ha || hb;
    }
}

// The tree fold in tree_fold_rec's order (pairs (0,1), (2,3), their sum, ...)
// with U packets per lane: the slots are loaded as the recursion reaches
// them, so the compiler may keep fewer of them live (more waves per SIMD)
// instead of issuing all KMAX x U loads up front as k_contig_tree does.
template <int U> struct PkU {
    v4u x[U];
};

template <class C, int KMAX, int U>
__global__ void __launch_bounds__(256)
k_contig_tree_rec(MultiIn<typename C::unit> ins, int k, uint32_t pres,
                  typename C::unit *__restrict__ out, uint64_t head, uint64_t npk,
                  uint64_t tail_start, uint32_t ntail, Params prm)
{
    using T = typename C::unit;
    v4u *vout = reinterpret_cast<v4u *>(out + head);
    const uint64_t nt = blockDim.x;
    const uint64_t stride = (uint64_t) gridDim.x * nt * U;
    const bool wt = wt_block(prm);
    for (uint64_t i = (uint64_t) blockIdx.x * nt * U + threadIdx.x; i < npk; i += stride) {
        auto load = [&](int q) {
            PkU<U> v;
            const v4u *p = reinterpret_cast<const v4u *>(ins.p[q] + head) + i;
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (i + u * nt < npk)
                    v.x[u] = ld16<true>(p + u * nt);
            return v;
        };
        auto f = [&](PkU<U> a, const PkU<U> &b) {
#pragma unroll
            for (int u = 0; u < U; ++u)
                a.x[u] = combine16<C>(a.x[u], b.x[u], prm);
            return a;
        };
        PkU<U> r;
        tree_fold_rec<0, KMAX>(r, k, pres, load, f);
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (i + u * nt < npk)
                st16_pol<true>(vout + i + u * nt, r.x[u], wt);
    }
    if (blockIdx.x == 0) {
        auto ce = [&](T a, T b) { return C::apply(a, b, prm); };
        auto one = [&](uint64_t t) {
            auto ld = [&](int q) { return ins.p[q][t]; };
            T r;
            tree_fold_rec<0, KMAX>(r, k, pres, ld, ce);
            out[t] = r;
        };
        for (uint64_t t = threadIdx.x; t < head; t += nt)
            one(t);
        for (uint64_t t = threadIdx.x; t < ntail; t += nt)
            one(tail_start + t);
    }
}

// the same fold element by element, for operands not sharing a 16-byte phase
// (and every 32-byte unit)
template <class C>
__global__ void __launch_bounds__(256)
k_elem_tree(MultiIn<typename C::unit> ins, int k, uint32_t pres, typename C::unit *__restrict__ out,
            uint64_t n, Params prm)
{
    using T = typename C::unit;
    auto ce = [&](T a, T b) { return C::apply(a, b, prm); };
    const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
        if constexpr (sizeof(T) > 16) {
            auto load = [&](int q) { return ins.p[q][t]; };
            T r;
            tree_fold_rec<0, kMaxMulti>(r, k, pres, load, ce);
            out[t] = r;
        } else {
            T v[kMaxMulti];
#pragma unroll
            for (int q = 0; q < kMaxMulti; ++q)
                if (q < k && ((pres >> q) & 1u))
                    v[q] = ins.p[q][t];
            tree_fold<kMaxMulti>(v, k, pres, ce);
            out[t] = v[0];
        }
    }
}

template <class C>
__global__ void __launch_bounds__(1024)
k_elem(const typename C::unit *__restrict__ in, typename C::unit *__restrict__ io, uint64_t n,
       Params prm, uint32_t nblk, uint32_t nt)
{
    const uint64_t stride = (uint64_t) nblk * nt;
    for (uint64_t i = (uint64_t) blockIdx.x * nt + threadIdx.x; i < n; i += stride)
        io[i] = C::apply(io[i], in[i], prm);
}

// 32-byte units (long double / binary128 pairs and complex), both operands
// 16-byte aligned.  Loads and stores stay k_contig's: lane l of a wave reads
// packets l and 64 + l of the wave's 128-packet (64-unit) run, so every
// instruction moves 1 KiB of whole lines (a unit per lane, its two packets 32
// bytes apart, would move half lines per instruction).  Adjacent lanes then
// swap one packet (DPP, no LDS): the even lane of a pair holds unit m of the
// run, the odd lane unit 32 + m; after the combine the same swap restores the
// packet layout for the stores.  U runs per lane per operand in flight, all
// loads of the tile before the first combine, the store policy per block.
// Full tiles only; the last partial tile goes a unit per lane.
struct alignas(16) Pk32 {
    v4u lo, hi;
};
#ifndef MPIX_REDOP_BLOCK32
#define MPIX_REDOP_BLOCK32 64       // k_contig32 / k_batch32 block
#endif
#ifdef MPIX_C32_WAVES_N
#define MPIX_C32_WAVES __attribute__((amdgpu_waves_per_eu(MPIX_C32_WAVES_N)))
#else
#define MPIX_C32_WAVES
#endif

// Split combiners (C::kSplit, the soft complex products): C::apply_fast(a, b,
// prm, ok) runs only the normal-operand fast paths and sets ok false when any
// of them declines (its result is then unspecified); the contiguous 32-byte
// kernel leaves such a unit as it was, records it in Params::fixup (one 64-bit word per 64 units, written
// for every group) and k_fixup32 combines the recorded units with the full
// C::apply in a second launch.  The general paths stay out of the streaming
// kernel, whose registers -- and so its waves per SIMD -- are the fast path's
// (QuadCProd: 107 VGPRs with the general paths inline, 70 without; it is
// VALU- and latency-bound).
template <class C, class = void> struct is_split : std::false_type {};
template <class C> struct is_split<C, std::void_t<decltype(C::kSplit)>>
    : std::integral_constant<bool, C::kSplit> {};

// the 64-bit lane mask of contig32's gathered layout (lane 2m holds unit m of
// the run, lane 2m + 1 unit 32 + m) in unit order
__device__ __forceinline__ uint64_t lanes_to_units(uint64_t m)
{
    auto even = [](uint64_t x) {
        x &= 0x5555555555555555ull;
        x = (x | (x >> 1)) & 0x3333333333333333ull;
        x = (x | (x >> 2)) & 0x0f0f0f0f0f0f0f0full;
        x = (x | (x >> 4)) & 0x00ff00ff00ff00ffull;
        x = (x | (x >> 8)) & 0x0000ffff0000ffffull;
        return (x | (x >> 16)) & 0x00000000ffffffffull;
    };
    return even(m) | (even(m >> 1) << 32);
}

// ok ? r : a, a component at a time (a select of the two aggregates compiles
// to a pointer select over stack copies: scratch)
__device__ __forceinline__ Pk32 select_pk(bool ok, const Pk32 &r, const Pk32 &a)
{
    Pk32 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        o.lo[e] = ok ? r.lo[e] : a.lo[e];
        o.hi[e] = ok ? r.hi[e] : a.hi[e];
    }
    return o;
}

// v from the other lane of each adjacent pair (quad_perm [1,0,3,2])
__device__ __forceinline__ v4u swap_pair(v4u v)
{
    v4u r;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        r[e] = (unsigned) __builtin_amdgcn_mov_dpp((int) v[e], 0xB1, 0xF, 0xF, false);
    return r;
}

// Tile t (tile = nt * U units) of one 32-byte combine: a full tile through
// the packet loads and the lane swap, the last partial tile a unit per lane.
// Block-uniform: every lane of the block takes the same branch (the swap
// needs whole waves).
template <class C, int U, bool NTL, bool NTS>
__device__ __forceinline__ void contig32_tile(const typename C::unit *in, const typename C::unit *io,
                                              typename C::unit *out, uint64_t n, uint64_t t,
                                              uint64_t nt, bool wt, const Params &prm)
{
    using T = typename C::unit;
    static_assert(sizeof(T) == 32, "32-byte units");
    const v4u *vin = reinterpret_cast<const v4u *>(in);
    const v4u *vio = reinterpret_cast<const v4u *>(io);     // the inout role (read)
    v4u *vout = reinterpret_cast<v4u *>(out);               // io itself, or the tree's output
    constexpr bool split = is_split<C>::value;
    bool ok = true;
    auto f = [&](const Pk32 &a, const Pk32 &b) {
        if constexpr (split)
            return __builtin_bit_cast(Pk32, C::apply_fast(__builtin_bit_cast(T, a),
                                                          __builtin_bit_cast(T, b), prm, ok));
        else
            return __builtin_bit_cast(Pk32, C::apply(__builtin_bit_cast(T, a),
                                                     __builtin_bit_cast(T, b), prm));
    };
    // one fixup word per 64 units (every group written: the buffer is reused)
    auto record = [&](uint64_t unit0, uint64_t mask) {
        if constexpr (split)
            if ((threadIdx.x & 63) == 0)
                prm.fixup[unit0 >> 6] = mask;
    };
    const uint64_t tile = nt * U;
    // (the split combiners too: a unit per lane for every tile, two 16-byte
    // loads 16 bytes apart, saves the swaps' selects and DPP moves but ran
    // COMPLEX32 PROD 4.97 -> 4.51 and C_LONG_DOUBLE_COMPLEX PROD 6.24 -> 4.47
    // TB/s, profiles/r06_soft_rows_ab6.jsonl)
#ifndef MPIX_C32_LDS
#define MPIX_C32_LDS 1
#endif
    if ((t + 1) * tile <= n) {
        if constexpr (split && MPIX_C32_LDS) {
            // the split combiners are issue-bound: the packets go through LDS
            // (unit m of the run = packets 2m, 2m + 1 to lane m), which costs
            // no VALU, instead of the DPP swap and its selects; the lane's
            // unit is then in run order, so its ballot is the fixup word
            __shared__ v4u lds[MPIX_REDOP_BLOCK32 / 64][2][128];
            const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
            v4u *la = lds[wave][0], *lb = lds[wave][1];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint64_t run0 = t * tile + u * nt + wave * 64;
                const uint64_t q = 2 * run0 + lane;
                const v4u a0 = ld16<NTL>(vio + q), a1 = ld16<NTL>(vio + q + 64);
                const v4u b0 = ld16<NTL>(vin + q), b1 = ld16<NTL>(vin + q + 64);
                la[lane] = a0;
                la[lane + 64] = a1;
                lb[lane] = b0;
                lb[lane + 64] = b1;
                __syncthreads();
                const Pk32 r = f(Pk32{la[2 * lane], la[2 * lane + 1]},
                                 Pk32{lb[2 * lane], lb[2 * lane + 1]});
                __syncthreads();
                if (ok) {       // a declined unit stays as it was (k_fixup32 reads it)
                    la[2 * lane] = r.lo;
                    la[2 * lane + 1] = r.hi;
                }
                __syncthreads();
                st16_pol<NTS>(vout + q, la[lane], wt);
                st16_pol<NTS>(vout + q + 64, la[lane + 64], wt);
                record(run0, __ballot(!ok));
                __syncthreads();
            }
        } else {
            const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
            const bool odd = lane & 1;
            // the unit a lane holds after the swap: run unit lane/2 (even) or 32 + lane/2 (odd)
            auto gather = [&](v4u p0, v4u p1) {
                const v4u y = swap_pair(odd ? p0 : p1);
                return odd ? Pk32{y, p1} : Pk32{p0, y};
            };
            v4u a0[U], a1[U], b0[U], b1[U];
            // run u of this wave: units [t*tile + u*nt + wave*64, +64) = packets from q
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint64_t q = 2 * (t * tile + u * nt + wave * 64) + lane;
                a0[u] = ld16<NTL>(vio + q);
                a1[u] = ld16<NTL>(vio + q + 64);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint64_t q = 2 * (t * tile + u * nt + wave * 64) + lane;
                b0[u] = ld16<NTL>(vin + q);
                b1[u] = ld16<NTL>(vin + q + 64);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const Pk32 ga = gather(a0[u], a1[u]);
                Pk32 r = f(ga, gather(b0[u], b1[u]));
                if constexpr (split)
                    r = select_pk(ok, r, ga);   // a declined unit stays as it was
                const v4u y = swap_pair(odd ? r.lo : r.hi);
                const uint64_t q = 2 * (t * tile + u * nt + wave * 64) + lane;
                st16_pol<NTS>(vout + q, odd ? y : r.lo, wt);
                st16_pol<NTS>(vout + q + 64, odd ? r.hi : y, wt);
                if constexpr (split)
                    record(t * tile + u * nt + wave * 64, lanes_to_units(__ballot(!ok)));
            }
        }
    } else {
        const uint64_t end = (t + 1) * tile < n ? (t + 1) * tile : n;    // this tile only
        for (uint64_t k = t * tile + threadIdx.x; k < end; k += nt) {
            const Pk32 a{ld16<NTL>(vio + 2 * k), ld16<NTL>(vio + 2 * k + 1)};
            Pk32 r = f(a, Pk32{ld16<NTL>(vin + 2 * k), ld16<NTL>(vin + 2 * k + 1)});
            if constexpr (split)
                r = select_pk(ok, r, a);    // a declined unit stays as it was
            st16_pol<NTS>(vout + 2 * k, r.lo, wt);
            st16_pol<NTS>(vout + 2 * k + 1, r.hi, wt);
            if constexpr (split)        // a unit per lane: the mask is in unit order
                record(k - (threadIdx.x & 63), __ballot(!ok));
        }
    }
}

template <class C, int U, bool NTL, bool NTS>
__global__ void __launch_bounds__(256) MPIX_C32_WAVES
k_contig32(const typename C::unit *in, const typename C::unit *io, typename C::unit *out, uint64_t n,
           Params prm, uint32_t nblk, uint32_t nthreads)
{
    const uint64_t tile = (uint64_t) nthreads * U;
    const uint64_t ntiles = (n + tile - 1) / tile;
    const bool wt = wt_block(prm);
    for (uint64_t t = blockIdx.x; t < ntiles; t += nblk)
        contig32_tile<C, U, NTL, NTS>(in, io, out, n, t, nthreads, wt, prm);
}

// The second launch of a split combiner: every unit the fast kernel recorded
// in the fixup words (it left them unchanged in `out`), combined with the full
// C::apply from the untouched operands (`io` is `out` in place, or the tree's
// separate inout role).  A wave loads 64 consecutive words (one per lane),
// skips them at once when all are zero (the usual case), and otherwise walks
// them in order: word j's units are combined by the lanes whose bit is set,
// lane l taking unit 64 (base + j) + l, so the loads and stores of a densely
// marked word are coalesced (a lane per word, walking its own 64 units, had
// each load hit 64 lines 2 KiB apart: real values stored as complex, where
// every unit declines, ran at 1.6 TB/s; profiles/r06_soft_zero_im.json).
template <class C>
__global__ void __launch_bounds__(256)
k_fixup32(const typename C::unit *in, const typename C::unit *io, typename C::unit *out, uint64_t n,
          Params prm, uint32_t nblk)
{
    const uint64_t nw = (n + 63) / 64;
    const unsigned lane = threadIdx.x & 63;
    for (uint64_t wb = (uint64_t) blockIdx.x * 256 + (threadIdx.x & ~63u); wb < nw;
         wb += (uint64_t) nblk * 256) {
        const uint64_t mine = wb + lane < nw ? prm.fixup[wb + lane] : 0;
        if (__ballot(mine != 0) == 0)
            continue;
        for (int j = 0; j < 64; ++j) {
            const uint32_t lo = (uint32_t) __builtin_amdgcn_readlane((int) (uint32_t) mine, j);
            const uint32_t hi = (uint32_t) __builtin_amdgcn_readlane((int) (uint32_t) (mine >> 32), j);
            const uint64_t m = ((uint64_t) hi << 32) | lo;
            if (m == 0)
                continue;
            const uint64_t u = (wb + j) * 64 + lane;
            if (((m >> lane) & 1) && u < n)
                out[u] = C::apply(io[u], in[u], prm);
        }
    }
}

// The batch entry's form for 32-byte units: segment s owns blocks [blk0,
// blk0 + its tiles), one tile each (BatchSeg::npk holds its count in units),
// each tile combined as k_contig32 combines it.
template <class C, int U, bool NTL, bool NTS>
__global__ void __launch_bounds__(256)
k_batch32(BatchTab tab, int nseg, Params prm, uint32_t nt)
{
    using T = typename C::unit;
    const uint32_t b = blockIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    const bool le = lane < (uint32_t) nseg && tab.blk0[lane] <= b;
    const int q = __popcll(__ballot(le)) - 1;
    const BatchSeg &g = tab.s[q];
    contig32_tile<C, U, NTL, NTS>(static_cast<const T *>(g.in), static_cast<const T *>(g.io),
                                  static_cast<T *>(g.io), g.npk, b - tab.blk0[q], nt,
                                  wt_block(prm), prm);
}

// Vector target (typerep_op.c:115-150 for MPI_Type_vector(count, bl, stride)):
// packed source element j = b*bl + k lands on target element b*stride + k.
// Thread per source element: the source stream is fully coalesced, the
// target reads/writes are coalesced within each block run; gap elements are
// never loaded or stored.
template <class C>
__global__ void __launch_bounds__(1024)
k_vector(const typename C::unit *__restrict__ in, typename C::unit *__restrict__ io, uint64_t n,
         uint64_t bl, uint64_t st, Params prm, uint32_t nblk, uint32_t nt)
{
    const uint64_t stride = (uint64_t) nblk * nt;
    for (uint64_t j = (uint64_t) blockIdx.x * nt + threadIdx.x; j < n; j += stride) {
        uint64_t b = j / bl, k = j - b * bl;
        uint64_t t = b * st + k;
        io[t] = C::apply(io[t], in[j], prm);
    }
}

// bl == 1 specialisation: no division
template <class C>
__global__ void __launch_bounds__(1024)
k_vector1(const typename C::unit *__restrict__ in, typename C::unit *__restrict__ io, uint64_t n,
          uint64_t st, Params prm, uint32_t nblk, uint32_t nt)
{
    const uint64_t stride = (uint64_t) nblk * nt;
    for (uint64_t j = (uint64_t) blockIdx.x * nt + threadIdx.x; j < n; j += stride)
        io[j * st] = C::apply(io[j * st], in[j], prm);
}

// (bl, stride) = (1, 2), config 5: each lane loads the whole 2-element target
// pair {payload, gap} as one vector load (the line is fetched whole anyway,
// and one 16-B load per lane issues half the requests of two 8-B ones), then
// stores the payload element only; plain (non-temporal-free) policy so the
// half-line stores merge with the lines still held in L2 (measured: +10 %
// over 8-B target loads, non-temporal -25 %; profiles/r01_tune_vector.txt).
template <int N> struct RawOf;
template <> struct RawOf<2> { typedef unsigned short type; };
template <> struct RawOf<4> { typedef unsigned int type; };
template <> struct RawOf<8> { typedef unsigned int type __attribute__((ext_vector_type(2))); };
template <> struct RawOf<16> { typedef unsigned int type __attribute__((ext_vector_type(4))); };
template <> struct RawOf<32> { typedef unsigned int type __attribute__((ext_vector_type(8))); };

// Payload store of the stride-2 vector target, write-through (global_store
// sc0 sc1: the half-written line leaves L2 at once instead of waiting dirty
// for eviction) for 1..8-byte units: +1.9 % at the 2.5 GiB traffic floor of
// config 5, same FETCH/WRITE bytes (profiles/r02_tune_vector2.txt,
// tools/tune_vector2.hip S1 vs S0).  A relaxed system-scope atomic store is
// only the cache policy here: no ordering is asked of it.
template <typename T>
__device__ __forceinline__ void st_payload_wt(T *p, const T &v)
{
    if constexpr (sizeof(T) == 8) {
        unsigned long long u;
        __builtin_memcpy(&u, &v, 8);
        __hip_atomic_store(reinterpret_cast<unsigned long long *>(p), u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    } else if constexpr (sizeof(T) == 4) {
        unsigned int u;
        __builtin_memcpy(&u, &v, 4);
        __hip_atomic_store(reinterpret_cast<unsigned int *>(p), u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    } else {
        *p = v;
    }
}

// Packed-source load of the stride-2 vector target, non-temporal for 4- and
// 8-byte units (read once, never revisited): with the write-through payload
// store +3.9 % over the default-policy source load at the same traffic
// (profiles/r02_tune_vector2b.txt, tools/tune_vector2.hip S6 vs S1).
template <typename T>
__device__ __forceinline__ T ld_source_nt(const T *p)
{
    if constexpr (sizeof(T) == 8) {
        unsigned long long u = __builtin_nontemporal_load(reinterpret_cast<const unsigned long long *>(p));
        T v;
        __builtin_memcpy(&v, &u, 8);
        return v;
    } else if constexpr (sizeof(T) == 4) {
        unsigned int u = __builtin_nontemporal_load(reinterpret_cast<const unsigned int *>(p));
        T v;
        __builtin_memcpy(&v, &u, 4);
        return v;
    } else {
        return *p;
    }
}

template <class C>
__global__ void __launch_bounds__(256)
k_vector_s2(const typename C::unit *__restrict__ in, typename C::unit *__restrict__ io, uint64_t n,
            Params prm, uint32_t nblk, uint32_t nt)
{
    using T = typename C::unit;
    using R = typename RawOf<2 * sizeof(T)>::type;
    const uint64_t stride = (uint64_t) nblk * nt;
    for (uint64_t j = (uint64_t) blockIdx.x * nt + threadIdx.x; j < n; j += stride) {
        T t;
        if (j + 1 < n) {
            R raw = reinterpret_cast<const R *>(io)[j];
            __builtin_memcpy(&t, &raw, sizeof(T));
        } else {    // the last pair would reach one element past the type's span
            t = io[2 * j];
        }
        st_payload_wt(io + 2 * j, C::apply(t, ld_source_nt(in + j), prm));
    }
}

// General derived target given as its flattened iov (typerep_op.c:100-150):
// run s covers seg_off[s] (element offset into inout) .. + its count; its
// source elements start at src_off[s] of the packed source (runs are
// consumed in order, so src_off is the running prefix unless the host split
// the runs by alignment class).  prefix[s] = elements before run s in this
// launch (prefix[nseg] = total).  Thread per packed element; every kernel over
// such a table is one of the two loops below with a way to find the lane's run
// and what to do with target element t and packed element p.

// last s in [lo, hi] with prefix[s] <= j
__device__ __forceinline__ int64_t iov_search(const int64_t *__restrict__ prefix, int64_t lo,
                                              int64_t hi, uint64_t j)
{
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if ((uint64_t) prefix[mid] <= j)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// The run of packed index j < total = prefix[nseg]: LOOKUP 0 = a binary search
// per lane over the whole prefix table; 1 = one wave-uniform search for the
// wave's first index, which serves every lane when the wave's last index lies
// in the same run, else the lanes search from that run on.  Every caller runs
// 256-thread blocks over j = block * 256 + thread + i * (nblk * 256), so the
// active lanes of a wave hold consecutive indices from j & ~63.
template <int LOOKUP>
__device__ __forceinline__ int64_t iov_run(const int64_t *__restrict__ prefix, int64_t nseg,
                                           uint64_t j, uint64_t total)
{
    if constexpr (LOOKUP == 0) {
        return iov_search(prefix, 0, nseg - 1, j);
    } else {
        const uint64_t w = j & ~(uint64_t) 63;
        const uint64_t first =
            ((uint64_t) __builtin_amdgcn_readfirstlane((uint32_t) (w >> 32)) << 32) |
            __builtin_amdgcn_readfirstlane((uint32_t) w);
        const uint64_t last = first + 63 < total ? first + 63 : total - 1;
        const int64_t s = iov_search(prefix, 0, nseg - 1, first);       // wave-uniform
        if ((uint64_t) prefix[s + 1] > last)
            return s;
        return iov_search(prefix, s, nseg - 1, j);
    }
}

// The run of packed index j = 256 t + thread < total of a committed plan
// (below): LOOKUP 0 = the per-tile index, 1 = iov_run<1>.
template <int LOOKUP>
__device__ __forceinline__ int64_t plan_run(const int64_t *__restrict__ prefix,
                                            const int32_t *__restrict__ tile, int64_t nseg,
                                            uint64_t t, uint64_t j, uint64_t total)
{
    if constexpr (LOOKUP == 0) {
        const int64_t lo = tile[t], hi = tile[t + 1];       // block-uniform
        if (lo == hi)
            return lo;
        return iov_search(prefix, lo, hi, j);
    } else {
        return iov_run<1>(prefix, nseg, j, total);
    }
}

// Packed index j of run s: target element t, packed element p
struct RunAt {
    int64_t t, p;
};
__device__ __forceinline__ RunAt run_at(const int64_t *__restrict__ seg_off,
                                        const int64_t *__restrict__ prefix,
                                        const int64_t *__restrict__ src_off, int64_t s, uint64_t j)
{
    const int64_t k = (int64_t) (j - (uint64_t) prefix[s]);
    return RunAt{seg_off[s] + k, src_off[s] + k};
}

// Every kernel over a table runs 256-thread blocks (launch_runs) in one of two
// loops: a grid-stride over the packed indices with iov_run, or a tile of 256
// per iteration with plan_run, whose tile index is then block-uniform.  The
// loop and its element stay written out in each kernel: behind a function
// boundary (a functor, a lambda, a helper) the compiler narrows the load and the
// store of the padded 32-byte pair (MPI_LONG_DOUBLE_INT) to its members, and
// those partial stores measured 1-3 % slower.

template <class C>
__global__ void __launch_bounds__(256)
k_iov(const typename C::unit *__restrict__ in, typename C::unit *__restrict__ io,
      const int64_t *__restrict__ seg_off, const int64_t *__restrict__ prefix,
      const int64_t *__restrict__ src_off, int64_t nseg, uint64_t total, Params prm,
      uint32_t nblk)
{
    const uint64_t stride = (uint64_t) nblk * 256;
    for (uint64_t j = (uint64_t) blockIdx.x * 256 + threadIdx.x; j < total; j += stride) {
        const RunAt r = run_at(seg_off, prefix, src_off, iov_run<0>(prefix, nseg, j, total), j);
        io[r.t] = C::apply(io[r.t], in[r.p], prm);
    }
}

// ---------------------------------------------------------------------------
// The launchers: each asks redop_launch.h for its plan (the form, the grid and
// block, the split), switches on the form and launches.  The rules, and the
// bug reports behind them, are at the plan functions.

// One-wave blocks for the stride-2 vector target (plan_vector) and the 32-byte
// units (plan_contig's Packets32) too
// (round 5, tools/gpu_u_ab.sh against 256 threads, profiles/r05_block64_vec32.json):
// config 5 0.449 -> 0.433 ms; LONG_DOUBLE_INT MINLOC / MAXLOC 6.74-6.78 ->
// 7.06-7.09 TB/s, the complex long double / binary128 rows even to +2 %
#ifndef MPIX_REDOP_VBLOCK
#define MPIX_REDOP_VBLOCK 64        // the stride-2 vector target's block
#endif
// k_contig32's block (its __launch_bounds__)
constexpr unsigned kContig32Block = MPIX_REDOP_BLOCK32;

// LDS per 64 threads of a multi-input fold block (plan_multi): 160 KiB per CU
// / 6656 B = 24 one-wave blocks = 6 waves per SIMD (the kernel itself uses no
// LDS)
constexpr unsigned kMultiLds = 6656;

// what this unit's launchers of combiner C were compiled with
template <class C> constexpr LaunchFacts launch_facts()
{
    return LaunchFacts{is_split<C>::value, MPIX_REDOP_UNROLL,  MPIX_REDOP_UNROLL32,
                       MPIX_REDOP_BLOCK32, MPIX_REDOP_VBLOCK, kSignalMaxGrid,
                       kMultiLds};
}

inline uintptr_t addr(const void *p) { return reinterpret_cast<uintptr_t>(p); }

// k_contig32 over 16-byte-aligned 32-byte units (`io` read in the inout
// role, the result to `out`: io itself, or the tree's output) on the plan's
// grid; a split combiner adds its fixup launch
template <class C>
hipError_t launch_contig32(const typename C::unit *in, const typename C::unit *io,
                           typename C::unit *out, uint64_t count, unsigned grid, const Params &prm,
                           const LaunchCfg &cfg, hipStream_t s)
{
    constexpr int U32 = MPIX_REDOP_UNROLL32;
    Params p = prm;
    p.done = nullptr;
    set_store_policy(p, cfg, grid);
    // a split combiner holds its stream's word buffer over both launches: no
    // other caller's pair comes between them on `s`, and the buffer is not
    // freed under them
    FixupLease lease;
    if constexpr (is_split<C>::value) {
        lease = fixup_acquire(s, (count + 63) / 64 * sizeof(uint64_t));
        if (!lease.words)
            return hipErrorOutOfMemory;
        p.fixup = lease.words;
    }
    hipLaunchKernelGGL((k_contig32<C, U32, MPIX_REDOP_NT_LOAD, MPIX_REDOP_NT_STORE>), dim3(grid),
                       dim3(kContig32Block), 0, s, in, io, out, count, p, grid, kContig32Block);
    if constexpr (is_split<C>::value) {
        // a word per lane: the scan is one load per lane, mostly of zeros
        const unsigned g2 = grid_for(256, (count + 63) / 64, 0, 256);
        hipLaunchKernelGGL((k_fixup32<C>), dim3(g2), dim3(256), 0, s, in, io, out, count, p, g2);
    }
    const hipError_t e = hipGetLastError();
    if constexpr (is_split<C>::value)
        fixup_release(lease);
    return e;
}

// The launch of a plan_contig plan (launch_vector's too, for bl == st)
template <class C>
hipError_t run_contig(const LaunchPlan &pl, const void *in, void *io, uint64_t count,
                      const Params &prm, const LaunchCfg &cfg, hipStream_t s)
{
    using T = typename C::unit;
    const T *tin = static_cast<const T *>(in);
    T *tio = static_cast<T *>(io);
    const PacketSplit &sp = pl.split;
    switch (pl.form) {
        case Form::Packets32:
            if constexpr (sizeof(T) > 16) {
                hipError_t e = launch_contig32<C>(tin, tio, tio, count, pl.grid, prm, cfg, s);
                if (e != hipSuccess)
                    return e;
            }
            break;
        case Form::PacketsAin:
        case Form::PacketsUin:
            if constexpr (sizeof(T) <= 16) {
                Params p = prm;
                if (!pl.signals)
                    p.done = nullptr;
                set_store_policy(p, cfg, pl.grid);
                if (pl.form == Form::PacketsAin)
                    hipLaunchKernelGGL(
                        (k_contig<C, MPIX_REDOP_UNROLL, MPIX_REDOP_NT_LOAD, MPIX_REDOP_NT_STORE, true>),
                        dim3(pl.grid), dim3(pl.block), 0, s, tin, tio, sp.head, sp.npk,
                        sp.tail_start, sp.ntail, p, pl.grid, pl.block);
                else
                    hipLaunchKernelGGL(
                        (k_contig<C, MPIX_REDOP_UNROLL, MPIX_REDOP_NT_LOAD, MPIX_REDOP_NT_STORE, false>),
                        dim3(pl.grid), dim3(pl.block), 0, s, tin, tio, sp.head, sp.npk,
                        sp.tail_start, sp.ntail, p, pl.grid, pl.block);
            }
            break;
        default:
            hipLaunchKernelGGL((k_elem<C>), dim3(pl.grid), dim3(pl.block), 0, s, tin, tio, count, prm,
                               pl.grid, pl.block);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && prm.done && !pl.signals)
        e = hipStreamWriteValue32(s, (void *) prm.done, prm.done_seq, 0);
    return e;
}

// Contiguous launcher: the packet, the 32-byte packet or the element-wise kernel.
template <class C>
hipError_t launch_contig(const void *in, void *io, uint64_t count, const Params &prm,
                         const LaunchCfg &cfg, hipStream_t s)
{
    const LaunchPlan pl = plan_contig(addr(in), addr(io), sizeof(typename C::unit), count, cfg,
                                      launch_facts<C>(), prm.done, prm.done_ctr);
    return run_contig<C>(pl, in, io, count, prm, cfg, s);
}

template <class C>
hipError_t launch_multi(const void *const *ins, int k, void *io, uint64_t count, const Params &prm,
                        const LaunchCfg &cfg, hipStream_t s)
{
    using T = typename C::unit;
    MultiIn<T> mi{};
    uintptr_t ai[kMaxMulti];
    for (int q = 0; q < k; ++q) {
        mi.p[q] = static_cast<const T *>(ins[q]);
        ai[q] = addr(ins[q]);
    }
    T *tio = static_cast<T *>(io);
    const LaunchPlan pl = plan_multi(ai, k, addr(io), sizeof(T), count, cfg, launch_facts<C>());
    if (pl.form == Form::PacketsAin) {
        // one packet per lane per input: 6.16 / 6.20 TB/s at k = 7 (256 MiB /
        // 1 GiB, store policy on) against 6.04 / 5.83 with two; 4 measured no
        // better than 2 (tools/tree8_probe.hip, tools/multi_probe.py)
        // plan_multi's LDS for k >= 2 inputs: unused LDS per block caps the
        // waves per SIMD at 6 (24 one-wave blocks per CU): with k + 2 streams
        // per wave fewer waves in flight run faster -- 256 MiB fp32, one-wave
        // blocks, store policy on: k = 3 6.53 -> 6.91, k = 7 6.53 -> 6.92,
        // k = 15 6.38 -> 6.65 TB/s against the round-5 form; the headline
        // kernel (k = 1) loses with any cap (7.04 -> 6.73) and keeps none
        // (profiles/r06_multi_fold_caps2.json)
        if constexpr (sizeof(T) <= 16) {
            Params p = prm;
            set_store_policy(p, cfg, pl.grid);
            hipLaunchKernelGGL((k_contig_multi<C, 1>), dim3(pl.grid), dim3(pl.block), pl.lds, s, mi,
                               k, tio, pl.split.head, pl.split.npk, pl.split.tail_start,
                               pl.split.ntail, p, pl.grid, pl.block);
        }
    } else {
        hipLaunchKernelGGL((k_elem_multi<C>), dim3(pl.grid), dim3(pl.block), 0, s, mi, k, tio, count,
                           prm, pl.grid, pl.block);
    }
    return hipGetLastError();
}

// out = tree fold of ins[0..k-1] (k a power of two, 2..16; k_contig_tree);
// a NULL slot is absent (its partner passes through)
template <class C>
hipError_t launch_tree(const void *const *ins, int k, void *out, uint64_t count, const Params &prm,
                       const LaunchCfg &cfg, hipStream_t s)
{
    using T = typename C::unit;
    MultiIn<T> mi{};
    uintptr_t ai[kMaxMulti];
    for (int q = 0; q < k; ++q) {
        mi.p[q] = static_cast<const T *>(ins[q]);
        ai[q] = addr(ins[q]);
    }
    T *tout = static_cast<T *>(out);
    const LaunchPlan pl = plan_tree(ai, k, addr(out), sizeof(T), count, cfg, launch_facts<C>());
    const PacketSplit &sp = pl.split;
    // plan_tree's forms by slot count (tools/tree8_probe.hip,
    // profiles/r05_tree_forms.json; fp32 SUM at 256 MiB / 1 GiB per operand,
    // store policy on):
    //   k = 2   the fold order, 2 packets per lane     6.81 / 6.94 TB/s
    //           (all 4 x 2 loads up front: 6.44 / 6.84)
    //   k = 4   all 4 x 2 loads up front               6.40 / 6.61
    //           (the fold order, 1 packet: 6.34 / 6.53)
    //   k = 8   the fold order, 1 packet per lane      6.47 / 6.36
    //           (8 x 2 up front 5.79 / 5.43, 16 x 1 up front 5.68 / 5.22)
    //   k = 16  the fold order, 1 packet per lane      6.37 / 5.92
    //           (16 x 1 up front 5.86 / 5.50)
    // Loading slots only as the fold reaches them keeps 39 VGPRs live at
    // k = 8 (8 waves per SIMD) against 111 for the up-front form (4), and
    // with nine streams the waves, not each wave's bytes in flight, carry
    // the rate.  The store policy: +5 % at k = 2, +3.8 % at k = 4, neutral
    // above.
    // One-wave (64-thread) blocks (kTreeBlock), as the contiguous kernel:
    // k = 2 / 4 / 8 / 16 at 6.84-6.96 / 6.48-6.61 / 6.58-6.67 / 6.06-6.45 TB/s
    // against 6.64-6.76 / 6.36-6.43 / 6.25-6.28 / 5.82-6.43 with 256 threads
    // (r05_tree_forms.json, last run).
    // The public entry takes k = 2, 4, 8, 16 only (the collectives pad an odd
    // world's fold with absent slots).
    switch (pl.form) {
        case Form::TreePair32:
            if constexpr (sizeof(T) > 16)
                return launch_contig32<C>(mi.p[1], mi.p[0], tout, count, pl.grid, prm, cfg, s);
            break;
        case Form::TreeElem:
            hipLaunchKernelGGL((k_elem_tree<C>), dim3(pl.grid), dim3(pl.block), 0, s, mi, k, pl.pres,
                               tout, count, prm);
            break;
        default:
            if constexpr (sizeof(T) <= 16) {
                Params p = prm;
                set_store_policy(p, cfg, pl.grid);
                auto launch = [&](auto kernel) {
                    hipLaunchKernelGGL(kernel, dim3(pl.grid), dim3(pl.block), 0, s, mi, k, pl.pres,
                                       tout, sp.head, sp.npk, sp.tail_start, sp.ntail, p);
                };
                if (pl.form == Form::Tree2x2)   // out = a OP b (recursive halving's combine_to)
                    launch(k_contig_tree_rec<C, 2, 2>);
                else if (pl.form == Form::Tree4x2)
                    launch(k_contig_tree<C, 4, 2>);
                else if (pl.form == Form::Tree8x1)      // the P = 8 pull's fold
                    launch(k_contig_tree_rec<C, 8, 1>);
                else
                    launch(k_contig_tree_rec<C, kMaxMulti, 1>);
            }
    }
    return hipGetLastError();
}

template <class C>
hipError_t launch_vector(const void *in, void *io, uint64_t count, uint64_t bl, uint64_t st,
                         const Params &prm, const LaunchCfg &cfg, hipStream_t s)
{
    using T = typename C::unit;
    const uint64_t n = count * bl;
    if (n == 0)
        return hipSuccess;
    const LaunchPlan pl = plan_vector(addr(in), addr(io), sizeof(T), n, bl, st, cfg,
                                      launch_facts<C>(), prm.done, prm.done_ctr);
    const T *tin = static_cast<const T *>(in);
    T *tio = static_cast<T *>(io);
    switch (pl.form) {
        case Form::VectorS2:
            if constexpr (sizeof(T) <= 16)
                hipLaunchKernelGGL((k_vector_s2<C>), dim3(pl.grid), dim3(pl.block), 0, s, tin, tio, n,
                                   prm, pl.grid, pl.block);
            break;
        case Form::Vector1:
            hipLaunchKernelGGL((k_vector1<C>), dim3(pl.grid), dim3(pl.block), 0, s, tin, tio, n, st,
                               prm, pl.grid, pl.block);
            break;
        case Form::Vector:
            hipLaunchKernelGGL((k_vector<C>), dim3(pl.grid), dim3(pl.block), 0, s, tin, tio, n, bl, st,
                               prm, pl.grid, pl.block);
            break;
        default:        // bl == st: contiguous after all
            return run_contig<C>(pl, in, io, n, prm, cfg, s);
    }
    return hipGetLastError();
}

// The launch of every kernel over a run table: nothing
// for an empty table, else 256-thread blocks of four packed elements per
// thread, striding beyond the grid cap; the grid size is the kernel's last
// argument after `args`.
template <class K, class... A>
hipError_t launch_runs(K kernel, int64_t nseg, uint64_t total, const LaunchCfg &cfg, hipStream_t s,
                       A... args)
{
    if (total == 0 || nseg == 0)
        return hipSuccess;
    const unsigned grid = grid_for(256ull * 4, total, cfg.max_grid, 256);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, s, args..., grid);
    return hipGetLastError();
}

// ... and its Params: these kernels signal no completion word and run the full
// C::apply (no fixup words)
inline Params run_params(const Params &prm)
{
    Params p = prm;
    p.done = nullptr;
    p.fixup = nullptr;
    return p;
}

template <class C>
hipError_t launch_iov(const void *in, void *io, const int64_t *d_seg_off, const int64_t *d_prefix,
                      const int64_t *d_src_off, int64_t nseg, uint64_t total, const Params &prm,
                      const LaunchCfg &cfg, hipStream_t s)
{
    using T = typename C::unit;
    return launch_runs(k_iov<C>, nseg, total, cfg, s, static_cast<const T *>(in),
                       static_cast<T *>(io), d_seg_off, d_prefix, d_src_off, nseg, total,
                       run_params(prm));
}

// k independent contiguous combines (no operand range of one overlapping a
// target of another; the caller checked) in one k_batch launch; segments of
// zero count are skipped, segments whose operands are not element-aligned go
// to launch_contig's element-wise kernel, as do all of a 32-byte unit type
template <class C>
hipError_t launch_batch(const void *const *ins, void *const *ios, const uint64_t *counts, int k,
                        const Params &prm, const LaunchCfg &cfg, hipStream_t s)
{
    using T = typename C::unit;
    Params p = prm;
    p.done = nullptr;
    uintptr_t ai[kMaxBatch], ao[kMaxBatch];
    for (int i = 0; i < k; ++i) {
        ai[i] = addr(ins[i]);
        ao[i] = addr(ios[i]);
    }
    BatchPacker pack(ai, ao, counts, k, sizeof(T), cfg, launch_facts<C>());
    BatchTab tab;
    for (BatchStep st; pack.next(st);) {
        hipError_t e = hipSuccess;
        switch (st.kind) {
            case BatchStep::Own:    // launch_contig (a split combiner: with its fixup)
                e = launch_contig<C>(ins[st.i], ios[st.i], counts[st.i], p, cfg, s);
                break;
            case BatchStep::Seg:
                tab.blk0[st.n] = st.blk0;
                tab.s[st.n] = BatchSeg{ins[st.i], ios[st.i], st.split.npk, (uint8_t) st.split.head,
                                       (uint8_t) st.split.ntail, (uint8_t) st.ain, {0, 0, 0, 0, 0}};
                break;
            case BatchStep::Flush: {
                Params q = p;
                const unsigned grid = (unsigned) st.blocks;
                set_store_policy(q, cfg, grid);
                if constexpr (is_split<C>::value)
                    ;   // every segment a call of its own
                else if constexpr (sizeof(T) > 16)
                    hipLaunchKernelGGL((k_batch32<C, MPIX_REDOP_UNROLL32, MPIX_REDOP_NT_LOAD,
                                                  MPIX_REDOP_NT_STORE>),
                                       dim3(grid), dim3(pack.block()), 0, s, tab, st.n, q,
                                       pack.block());
                else
                    hipLaunchKernelGGL((k_batch<C, MPIX_REDOP_UNROLL, MPIX_REDOP_NT_LOAD,
                                                MPIX_REDOP_NT_STORE>),
                                       dim3(grid), dim3(pack.block()), 0, s, tab, st.n, q, grid,
                                       pack.block());
                e = hipGetLastError();
            }
        }
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

// ---------------------------------------------------------------------------
// Fused get-accumulate (MPIX_Get_accumulate_local*): result = target as it
// was, target = target OP origin, the target read once -- 4 x bytes where the
// reference's copy followed by the op (posix_rma.h:366-375) moves 5 x.  The
// combiners are the reduction's own, with the target in the inout role, so the
// target's bits are those of the reduce entry.  No shared state: the split
// combiners run their full C::apply element-wise and never touch the fixup
// words.

// The result takes the type map only (MPIR_Localcopy): the struct pairs with
// padding get their value and their int stored member by member, so the
// result's own padding bytes stay as they were.
template <class T> struct FetchStore {
    static __device__ __forceinline__ void st(T *dst, const T &v) { *dst = v; }
    static constexpr bool whole = true;
};
#define MPIX_FETCH_MEMBERS(T)                                                  \
    template <> struct FetchStore<T> {                                         \
        static __device__ __forceinline__ void st(T *dst, const T &v)          \
        {                                                                      \
            dst->v = v.v;                                                      \
            dst->l = v.l;                                                      \
        }                                                                      \
        static constexpr bool whole = false;                                   \
    }
MPIX_FETCH_MEMBERS(DoubleIntBody);
MPIX_FETCH_MEMBERS(LongIntBody);
MPIX_FETCH_MEMBERS(ShortInt);
MPIX_FETCH_MEMBERS(LongDoubleInt);     // the long double's 16 bytes and the int
#undef MPIX_FETCH_MEMBERS

// Cache policy of the packet store to `result`, a line written once and not
// read again by this call: 0 non-temporal, 1 plain, 2 write-through, 3 the
// policy of the block's target store (st16_pol).  The choice is measured
// (tools/getacc_rows.py, DESIGN.md "Fused get-accumulate").
#ifndef MPIX_GETACC_RESULT_STORE
#define MPIX_GETACC_RESULT_STORE 0
#endif

// 16-byte store to `result`; !ALN: the address is only element-aligned
// (ld16u's counterpart, still one global_store_dwordx4)
typedef v4u v4u_unaligned __attribute__((aligned(1)));
template <bool ALN, int POL> __device__ __forceinline__ void st16_result(char *p, v4u v, bool wt)
{
    using V = std::conditional_t<ALN, v4u, v4u_unaligned>;
    typedef __attribute__((address_space(1))) V gV;
    V *q = reinterpret_cast<V *>(p);
    if (POL == 2 || (POL == 3 && wt))
        *(volatile gV *) (gV *) q = v;
    else if constexpr (POL == 1)
        *q = v;
    else
        __builtin_nontemporal_store(v, q);
}

// Packet kernel, units of at most 16 bytes, all three operands element-aligned:
// contig_body's head / packets / tail split by the target's 16-byte phase, one
// packet per lane.  ALN: origin and result share that phase (packet accesses);
// otherwise either is only element-aligned and both go through unaligned
// 16-byte accesses.  Both loads are issued before the combine.
template <class C, bool NTL, bool NTS, bool ALN>
__global__ void __launch_bounds__(1024)
k_getacc(const typename C::unit *__restrict__ in, typename C::unit *__restrict__ res,
         typename C::unit *__restrict__ io, uint64_t head, uint64_t npk, uint64_t tail_start,
         uint32_t ntail, Params prm, uint32_t nblk, uint32_t nt)
{
    using T = typename C::unit;
    constexpr int E = 16 / sizeof(T);
    const v4u *__restrict__ vin = reinterpret_cast<const v4u *>(in + head);
    const char *__restrict__ cin = reinterpret_cast<const char *>(in + head);
    char *__restrict__ cres = reinterpret_cast<char *>(res + head);
    v4u *__restrict__ vio = reinterpret_cast<v4u *>(io + head);
    const uint64_t stride = (uint64_t) nblk * nt;
    const bool wt = wt_block(prm);
    for (uint64_t i = (uint64_t) blockIdx.x * nt + threadIdx.x; i < npk; i += stride) {
        const v4u a = ld16<NTL>(vio + i);
        v4u b;
        if constexpr (ALN)
            b = ld16<NTL>(vin + i);
        else
            b = ld16u(cin + 16 * i);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (FetchStore<T>::whole) {
            st16_result<ALN, MPIX_GETACC_RESULT_STORE>(cres + 16 * i, a, wt);
        } else {
            struct alignas(16) Pk { T u[E]; };
            const Pk pa = __builtin_bit_cast(Pk, a);
#pragma unroll
            for (int e = 0; e < E; ++e)
                FetchStore<T>::st(res + head + i * E + e, pa.u[e]);
        }
        st16_pol<NTS>(vio + i, combine16<C>(a, b, prm), wt);
    }
    if (blockIdx.x == 0) {
        auto one = [&](uint64_t t) {
            const T a = io[t];
            FetchStore<T>::st(res + t, a);
            io[t] = C::apply(a, in[t], prm);
        };
        for (uint64_t t = threadIdx.x; t < head; t += nt)
            one(t);
        for (uint64_t t = threadIdx.x; t < ntail; t += nt)
            one(tail_start + t);
    }
}

// Element-wise: operands that are not element-aligned, and every 32-byte unit
// (the x87 / binary128 pairs and complex types; a split combiner's full apply)
template <class C>
__global__ void __launch_bounds__(1024)
k_getacc_elem(const typename C::unit *__restrict__ in, typename C::unit *__restrict__ res,
              typename C::unit *__restrict__ io, uint64_t n, Params prm, uint32_t nblk, uint32_t nt)
{
    using T = typename C::unit;
    const uint64_t stride = (uint64_t) nblk * nt;
    for (uint64_t i = (uint64_t) blockIdx.x * nt + threadIdx.x; i < n; i += stride) {
        const T a = io[i];
        FetchStore<T>::st(res + i, a);
        io[i] = C::apply(a, in[i], prm);
    }
}

// Vector target (MPI_Type_vector(count, bl, st)), origin and result packed:
// packed element j = b*bl + k pairs with target element b*st + k; gap elements
// are neither loaded nor stored.
template <class C>
__global__ void __launch_bounds__(1024)
k_getacc_vector(const typename C::unit *__restrict__ in, typename C::unit *__restrict__ res,
                typename C::unit *__restrict__ io, uint64_t n, uint64_t bl, uint64_t st, Params prm,
                uint32_t nblk, uint32_t nt)
{
    using T = typename C::unit;
    const uint64_t stride = (uint64_t) nblk * nt;
    for (uint64_t j = (uint64_t) blockIdx.x * nt + threadIdx.x; j < n; j += stride) {
        uint64_t t = j * st;
        if (bl != 1) {      // uniform
            const uint64_t b = j / bl;
            t = b * st + (j - b * bl);
        }
        const T a = io[t];
        FetchStore<T>::st(res + j, a);
        io[t] = C::apply(a, in[j], prm);
    }
}

template <class C>
hipError_t launch_getacc(const void *in, void *res, void *io, uint64_t count, const Params &prm,
                         const LaunchCfg &cfg, hipStream_t s)
{
    using T = typename C::unit;
    const T *tin = static_cast<const T *>(in);
    T *tres = static_cast<T *>(res), *tio = static_cast<T *>(io);
    Params p = prm;
    p.done = nullptr;       // the fetch entries wait on the stream
    p.fixup = nullptr;
    const LaunchPlan pl = plan_getacc(addr(in), addr(res), addr(io), sizeof(T), count, cfg);
    const PacketSplit &sp = pl.split;
    if (pl.form == Form::GetaccElem) {
        hipLaunchKernelGGL((k_getacc_elem<C>), dim3(pl.grid), dim3(pl.block), 0, s, tin, tres, tio,
                           count, p, pl.grid, pl.block);
    } else if constexpr (sizeof(T) <= 16) {
        set_store_policy(p, cfg, pl.grid);
        if (pl.form == Form::GetaccAligned)
            hipLaunchKernelGGL((k_getacc<C, MPIX_REDOP_NT_LOAD, MPIX_REDOP_NT_STORE, true>),
                               dim3(pl.grid), dim3(pl.block), 0, s, tin, tres, tio, sp.head, sp.npk,
                               sp.tail_start, sp.ntail, p, pl.grid, pl.block);
        else
            hipLaunchKernelGGL((k_getacc<C, MPIX_REDOP_NT_LOAD, MPIX_REDOP_NT_STORE, false>),
                               dim3(pl.grid), dim3(pl.block), 0, s, tin, tres, tio, sp.head, sp.npk,
                               sp.tail_start, sp.ntail, p, pl.grid, pl.block);
    }
    return hipGetLastError();
}

template <class C>
hipError_t launch_getacc_vector(const void *in, void *res, void *io, uint64_t count, uint64_t bl,
                                uint64_t st, const Params &prm, const LaunchCfg &cfg,
                                hipStream_t s)
{
    using T = typename C::unit;
    const uint64_t n = count * bl;
    if (n == 0)
        return hipSuccess;
    if (bl == st)       // contiguous after all
        return launch_getacc<C>(in, res, io, n, prm, cfg, s);
    Params p = prm;
    p.done = nullptr;
    p.fixup = nullptr;
    const unsigned grid = grid_for((uint64_t) cfg.block * 4, n, cfg.max_grid, cfg.block);
    hipLaunchKernelGGL((k_getacc_vector<C>), dim3(grid), dim3(cfg.block), 0, s,
                       static_cast<const T *>(in), static_cast<T *>(res), static_cast<T *>(io), n, bl,
                       st, p, grid, (uint32_t) cfg.block);
    return hipGetLastError();
}

template <class C> struct MakeGetacc {
    static constexpr GetaccEntry get()
    {
        return GetaccEntry{&launch_getacc<C>, &launch_getacc_vector<C>};
    }
};

// ---------------------------------------------------------------------------
// The fetch form over an iov target (MPIX_Get_accumulate_local_iov[ec]_async):
// k_iov's run table, origin and result packed.  Launch-local packed index j
// lies in run s = the last one with prefix[s] <= j; with k = j - prefix[s] the
// target element is seg_off[s] + k and the packed element of BOTH origin and
// result is src_off[s] + k (the call's run order, not this residue group's).

// How a lane finds its run (iov_run): k_iov's search per lane, or the
// wave-uniform one.  The choice is measured (tools/getacc_rows.py iov,
// DESIGN.md "Fused get-accumulate").
#ifndef MPIX_GETACC_IOV_LOOKUP
#define MPIX_GETACC_IOV_LOOKUP 1
#endif

// MPI_NO_OP and MPI_REPLACE as type-map copies: GATHER the target's element
// into the packed result, SCATTER the packed origin's over the target.  T is
// the unit's body (a raw unit of its extent, or the padded pair), not a
// combiner.
template <class T, bool GATHER, bool SCATTER>
__device__ __forceinline__ void typemap_copy(const T *__restrict__ in, T *__restrict__ res,
                                             T *__restrict__ io, const RunAt &r)
{
    if constexpr (GATHER) {
        const T a = io[r.t];
        FetchStore<T>::st(res + r.p, a);
    }
    if constexpr (SCATTER) {
        const T b = in[r.p];
        FetchStore<T>::st(io + r.t, b);
    }
}

// Thread per packed element: the old target element is loaded once, stored to
// the result through FetchStore (type map only) and combined.  32-byte units
// and the split combiners run their full C::apply, as in k_getacc_elem: no
// fixup words, no shared state.
template <class C>
__global__ void __launch_bounds__(256)
k_getacc_iov(const typename C::unit *__restrict__ in, typename C::unit *__restrict__ res,
             typename C::unit *__restrict__ io, const int64_t *__restrict__ seg_off,
             const int64_t *__restrict__ prefix, const int64_t *__restrict__ src_off, int64_t nseg,
             uint64_t total, Params prm, uint32_t nblk)
{
    using T = typename C::unit;
    const uint64_t stride = (uint64_t) nblk * 256;
    for (uint64_t j = (uint64_t) blockIdx.x * 256 + threadIdx.x; j < total; j += stride) {
        const RunAt r = run_at(seg_off, prefix, src_off, iov_run<MPIX_GETACC_IOV_LOOKUP>(prefix, nseg, j, total), j);
        const T a = io[r.t];
        FetchStore<T>::st(res + r.p, a);
        io[r.t] = C::apply(a, in[r.p], prm);
    }
}

// one launch per residue group however many runs it has
template <class T, bool REPLACE>
__global__ void __launch_bounds__(256)
k_getacc_iov_copy(const T *__restrict__ in, T *__restrict__ res, T *__restrict__ io,
                  const int64_t *__restrict__ seg_off, const int64_t *__restrict__ prefix,
                  const int64_t *__restrict__ src_off, int64_t nseg, uint64_t total, uint32_t nblk)
{
    const uint64_t stride = (uint64_t) nblk * 256;
    for (uint64_t j = (uint64_t) blockIdx.x * 256 + threadIdx.x; j < total; j += stride) {
        const RunAt r = run_at(seg_off, prefix, src_off, iov_run<MPIX_GETACC_IOV_LOOKUP>(prefix, nseg, j, total), j);
        typemap_copy<T, true, REPLACE>(in, res, io, r);
    }
}

template <class C>
hipError_t launch_getacc_iov(const void *in, void *res, void *io, const int64_t *d_seg_off,
                             const int64_t *d_prefix, const int64_t *d_src_off, int64_t nseg,
                             uint64_t total, const Params &prm, const LaunchCfg &cfg, hipStream_t s)
{
    using T = typename C::unit;
    return launch_runs(k_getacc_iov<C>, nseg, total, cfg, s, static_cast<const T *>(in),
                       static_cast<T *>(res), static_cast<T *>(io), d_seg_off, d_prefix, d_src_off,
                       nseg, total, run_params(prm));
}

template <class T>
hipError_t launch_getacc_iov_copy_as(bool replace, const void *in, void *res, void *io,
                                     const int64_t *d_seg_off, const int64_t *d_prefix,
                                     const int64_t *d_src_off, int64_t nseg, uint64_t total,
                                     const LaunchCfg &cfg, hipStream_t s)
{
    return launch_runs(replace ? k_getacc_iov_copy<T, true> : k_getacc_iov_copy<T, false>, nseg,
                       total, cfg, s, static_cast<const T *>(in), static_cast<T *>(res),
                       static_cast<T *>(io), d_seg_off, d_prefix, d_src_off, nseg, total);
}

// The unit body of a type map of `extent` bytes: the whole extent
// (value_bytes == 0) or a value of value_bytes at 0 and an int at loc_off (the
// padded pairs, copied member by member through FetchStore).  f(T{}) for that
// body T; hipErrorInvalidValue for a layout without a kernel.
namespace {
// a 32-byte unit (the x87 / binary128 complex types) at the 16-byte alignment
// of their combiners' units
struct alignas(16) Raw32 {
    v4u lo, hi;
};
}  // namespace

template <class F>
hipError_t with_copy_body(uint32_t extent, uint32_t value_bytes, uint32_t loc_off, F f)
{
    if (value_bytes) {
        if (extent == 16 && value_bytes == 8 && loc_off == 8)
            return f(DoubleIntBody{});      // MPI_LONG_INT has the same map
        if (extent == 8 && value_bytes == 2 && loc_off == 4)
            return f(ShortInt{});
        if (extent == 32 && value_bytes == 16 && loc_off == 16)
            return f(LongDoubleInt{});
        return hipErrorInvalidValue;
    }
    switch (extent) {
        case 1: return f(uint8_t{});
        case 2: return f(RawOf<2>::type{});
        case 4: return f(RawOf<4>::type{});
        case 8: return f(RawOf<8>::type{});
        case 16: return f(RawOf<16>::type{});
        case 32: return f(Raw32{});
        default: return hipErrorInvalidValue;
    }
}

template <class C> struct MakeGetaccIov {
    static constexpr GetaccIovEntry get() { return GetaccIovEntry{&launch_getacc_iov<C>}; }
};

// ---------------------------------------------------------------------------
// Committed iov plans (MPIX_Iov_plan_*, MPIX_*_local_plan*): the run table of
// k_iov / k_getacc_iov, resident on the device, with one more table per
// residue group: tile[t] = the run that holds packed index 256 t, closed by
// tile[ntile] = nseg - 1.  One loop iteration of a 256-thread block covers
// exactly tile t = block + i * nblk, so both bounds are loads from a
// block-uniform address (scalar loads), and a lane's run lies in
// [tile[t], tile[t + 1]]: no search when the two are equal, else a search of
// `prefix` between them only.

// How a lane finds its run (plan_run): the per-tile index, or iov_run<1>'s
// wave-uniform search over the whole prefix table.  The choice is measured
// (tools/getacc_rows.py plan, DESIGN.md "Committed iov plans").
#ifndef MPIX_PLAN_LOOKUP
#define MPIX_PLAN_LOOKUP 0
#endif

// k_iov's element: inout element = inout element OP packed source element.
template <class C>
__global__ void __launch_bounds__(256)
k_plan_reduce(const typename C::unit *__restrict__ in, typename C::unit *__restrict__ io,
              const int64_t *__restrict__ seg_off, const int64_t *__restrict__ prefix,
              const int64_t *__restrict__ src_off, const int32_t *__restrict__ tile, int64_t nseg,
              uint64_t total, Params prm, uint32_t nblk)
{
    for (uint64_t t = blockIdx.x; t * 256 < total; t += nblk) {
        const uint64_t j = t * 256 + threadIdx.x;
        if (j >= total)
            break;
        const RunAt r = run_at(seg_off, prefix, src_off,
                               plan_run<MPIX_PLAN_LOOKUP>(prefix, tile, nseg, t, j, total), j);
        io[r.t] = C::apply(io[r.t], in[r.p], prm);
    }
}

// k_getacc_iov's element
template <class C>
__global__ void __launch_bounds__(256)
k_plan_getacc(const typename C::unit *__restrict__ in, typename C::unit *__restrict__ res,
              typename C::unit *__restrict__ io, const int64_t *__restrict__ seg_off,
              const int64_t *__restrict__ prefix, const int64_t *__restrict__ src_off,
              const int32_t *__restrict__ tile, int64_t nseg, uint64_t total, Params prm,
              uint32_t nblk)
{
    using T = typename C::unit;
    for (uint64_t t = blockIdx.x; t * 256 < total; t += nblk) {
        const uint64_t j = t * 256 + threadIdx.x;
        if (j >= total)
            break;
        const RunAt r = run_at(seg_off, prefix, src_off,
                               plan_run<MPIX_PLAN_LOOKUP>(prefix, tile, nseg, t, j, total), j);
        const T a = io[r.t];
        FetchStore<T>::st(res + r.p, a);
        io[r.t] = C::apply(a, in[r.p], prm);
    }
}

// The type-map copies over a plan, k_getacc_iov_copy's unit bodies: gather
// (the fetch form's MPI_NO_OP), swap (its MPI_REPLACE) and scatter (the reduce
// form's MPI_REPLACE: the packed source's type map over the runs, no result).
enum PlanCopy { kPlanGather = 0, kPlanSwap = 1, kPlanScatter = 2 };

template <class T, int MODE>
__global__ void __launch_bounds__(256)
k_plan_copy(const T *__restrict__ in, T *__restrict__ res, T *__restrict__ io,
            const int64_t *__restrict__ seg_off, const int64_t *__restrict__ prefix,
            const int64_t *__restrict__ src_off, const int32_t *__restrict__ tile, int64_t nseg,
            uint64_t total, uint32_t nblk)
{
    for (uint64_t t = blockIdx.x; t * 256 < total; t += nblk) {
        const uint64_t j = t * 256 + threadIdx.x;
        if (j >= total)
            break;
        const RunAt r = run_at(seg_off, prefix, src_off,
                               plan_run<MPIX_PLAN_LOOKUP>(prefix, tile, nseg, t, j, total), j);
        typemap_copy<T, MODE != kPlanScatter, MODE != kPlanGather>(in, res, io, r);
    }
}

// One residue group's device table as the host lays it out (RunGroup,
// redop_dispatch.h); the group's tile index is passed beside it.
template <class C>
hipError_t launch_plan_reduce(const void *in, void *io, const int64_t *d_tab,
                              const int32_t *d_tile, int64_t nseg, uint64_t total,
                              const Params &prm, const LaunchCfg &cfg, hipStream_t s)
{
    using T = typename C::unit;
    const RunGroup g(d_tab, nseg);
    return launch_runs(k_plan_reduce<C>, nseg, total, cfg, s, static_cast<const T *>(in),
                       static_cast<T *>(io), g.seg_off, g.prefix, g.src_off, d_tile, nseg, total,
                       run_params(prm));
}

template <class C>
hipError_t launch_plan_getacc(const void *in, void *res, void *io, const int64_t *d_tab,
                              const int32_t *d_tile, int64_t nseg, uint64_t total,
                              const Params &prm, const LaunchCfg &cfg, hipStream_t s)
{
    using T = typename C::unit;
    const RunGroup g(d_tab, nseg);
    return launch_runs(k_plan_getacc<C>, nseg, total, cfg, s, static_cast<const T *>(in),
                       static_cast<T *>(res), static_cast<T *>(io), g.seg_off, g.prefix, g.src_off,
                       d_tile, nseg, total, run_params(prm));
}

template <class T>
hipError_t launch_plan_copy_as(int mode, const void *in, void *res, void *io, const int64_t *d_tab,
                               const int32_t *d_tile, int64_t nseg, uint64_t total,
                               const LaunchCfg &cfg, hipStream_t s)
{
    auto kernel = mode == kPlanGather    ? k_plan_copy<T, kPlanGather>
                  : mode == kPlanSwap    ? k_plan_copy<T, kPlanSwap>
                  : mode == kPlanScatter ? k_plan_copy<T, kPlanScatter>
                                         : nullptr;
    if (!kernel)
        return hipErrorInvalidValue;
    const RunGroup g(d_tab, nseg);
    return launch_runs(kernel, nseg, total, cfg, s, static_cast<const T *>(in),
                       static_cast<T *>(res), static_cast<T *>(io), g.seg_off, g.prefix, g.src_off,
                       d_tile, nseg, total);
}

template <class C> struct MakePlan {
    static constexpr PlanEntry get()
    {
        return PlanEntry{&launch_plan_reduce<C>, &launch_plan_getacc<C>};
    }
};

// ---------------------------------------------------------------------------
// A datatype on every side (MPIX_[Get_]accumulate_local_typed*): k_plan_*'s
// tile loop over one residue group of the TARGET plan gives the lane its target
// element and its packed index p; element p of the origin and of the result is
// then found through that side's packed-order table (packed_run,
// redop_packed.h: two per-lane loads of its tile index, a search only where a
// tile spans several runs) at base + off[s] + (p - prefix[s]) elements.  What
// a side lacks is a null kernel argument, a branch every lane takes alike:
//   seg_off == nullptr    the target is one run: target element j, p = j
//   o_prefix / r_prefix   == nullptr: that operand's element p lies at base + p
//                         (packed, or one run whose offset the host added)
// -- not template parameters: eight variants per combiner would multiply the
// build of about a hundred combiners.  Byte offsets keep the alignment plan
// creation guarantees (4-byte residues, 2 for 2-byte types), which is what the
// target's own residue already asks of these loads and stores.

// element p of an operand with (prefix != nullptr) or without a table
template <class T>
__device__ __forceinline__ T *typed_at(T *base, const int64_t *__restrict__ prefix,
                                       const int64_t *__restrict__ off,
                                       const int32_t *__restrict__ tile, uint64_t p)
{
    if (!prefix)
        return base + p;
    const int64_t s = packed_run(prefix, tile, p);
    typedef __attribute__((__may_alias__)) char Byte;
    return reinterpret_cast<T *>((Byte *) base + off[s]) + (p - (uint64_t) prefix[s]);
}

// target element = target element OP origin element
template <class C>
__global__ void __launch_bounds__(256)
k_typed_acc(const typename C::unit *__restrict__ in, typename C::unit *__restrict__ io,
            const int64_t *__restrict__ seg_off, const int64_t *__restrict__ prefix,
            const int64_t *__restrict__ src_off, const int32_t *__restrict__ tile, int64_t nseg,
            const int64_t *__restrict__ o_prefix, const int64_t *__restrict__ o_off,
            const int32_t *__restrict__ o_tile, uint64_t total, Params prm, uint32_t nblk)
{
    using T = typename C::unit;
    for (uint64_t t = blockIdx.x; t * 256 < total; t += nblk) {
        const uint64_t j = t * 256 + threadIdx.x;
        if (j >= total)
            break;
        RunAt r{(int64_t) j, (int64_t) j};
        if (seg_off)
            r = run_at(seg_off, prefix, src_off,
                       plan_run<MPIX_PLAN_LOOKUP>(prefix, tile, nseg, t, j, total), j);
        const T *pi = typed_at(in, o_prefix, o_off, o_tile, (uint64_t) r.p);
        io[r.t] = C::apply(io[r.t], *pi, prm);
    }
}

// ... and result element = the target element as it was, type map only
template <class C>
__global__ void __launch_bounds__(256)
k_typed_getacc(const typename C::unit *__restrict__ in, typename C::unit *__restrict__ res,
               typename C::unit *__restrict__ io, const int64_t *__restrict__ seg_off,
               const int64_t *__restrict__ prefix, const int64_t *__restrict__ src_off,
               const int32_t *__restrict__ tile, int64_t nseg,
               const int64_t *__restrict__ o_prefix, const int64_t *__restrict__ o_off,
               const int32_t *__restrict__ o_tile, const int64_t *__restrict__ r_prefix,
               const int64_t *__restrict__ r_off, const int32_t *__restrict__ r_tile,
               uint64_t total, Params prm, uint32_t nblk)
{
    using T = typename C::unit;
    for (uint64_t t = blockIdx.x; t * 256 < total; t += nblk) {
        const uint64_t j = t * 256 + threadIdx.x;
        if (j >= total)
            break;
        RunAt r{(int64_t) j, (int64_t) j};
        if (seg_off)
            r = run_at(seg_off, prefix, src_off,
                       plan_run<MPIX_PLAN_LOOKUP>(prefix, tile, nseg, t, j, total), j);
        const T *pi = typed_at(in, o_prefix, o_off, o_tile, (uint64_t) r.p);
        T *pr = typed_at(res, r_prefix, r_off, r_tile, (uint64_t) r.p);
        const T a = io[r.t];
        FetchStore<T>::st(pr, a);
        io[r.t] = C::apply(a, *pi, prm);
    }
}

// MPI_NO_OP / MPI_REPLACE: k_plan_copy's modes and unit bodies (MPI_Get into a
// derived result, the swap, MPI_Put from a derived origin)
template <class T, int MODE>
__global__ void __launch_bounds__(256)
k_typed_copy(const T *__restrict__ in, T *__restrict__ res, T *__restrict__ io,
             const int64_t *__restrict__ seg_off, const int64_t *__restrict__ prefix,
             const int64_t *__restrict__ src_off, const int32_t *__restrict__ tile, int64_t nseg,
             const int64_t *__restrict__ o_prefix, const int64_t *__restrict__ o_off,
             const int32_t *__restrict__ o_tile, const int64_t *__restrict__ r_prefix,
             const int64_t *__restrict__ r_off, const int32_t *__restrict__ r_tile,
             uint64_t total, uint32_t nblk)
{
    for (uint64_t t = blockIdx.x; t * 256 < total; t += nblk) {
        const uint64_t j = t * 256 + threadIdx.x;
        if (j >= total)
            break;
        RunAt r{(int64_t) j, (int64_t) j};
        if (seg_off)
            r = run_at(seg_off, prefix, src_off,
                       plan_run<MPIX_PLAN_LOOKUP>(prefix, tile, nseg, t, j, total), j);
        if constexpr (MODE != kPlanScatter) {
            const T a = io[r.t];
            FetchStore<T>::st(typed_at(res, r_prefix, r_off, r_tile, (uint64_t) r.p), a);
        }
        if constexpr (MODE != kPlanGather) {
            const T b = *typed_at(in, o_prefix, o_off, o_tile, (uint64_t) r.p);
            FetchStore<T>::st(io + r.t, b);
        }
    }
}

// The target group's table: RunGroup of d_tab, or all null for a one-run target
// (nseg = 1 then, so that launch_runs launches).
struct TypedGroup {
    const int64_t *seg_off = nullptr, *prefix = nullptr, *src_off = nullptr;
    int64_t nseg = 1;
    explicit TypedGroup(const TypedRuns &r)
    {
        if (r.d_tab) {
            const RunGroup g(r.d_tab, r.nseg);
            seg_off = g.seg_off, prefix = g.prefix, src_off = g.src_off, nseg = r.nseg;
        }
    }
};

template <class C>
hipError_t launch_typed_acc(const void *in, void *io, const TypedRuns &r, const Params &prm,
                            const LaunchCfg &cfg, hipStream_t s)
{
    using T = typename C::unit;
    const TypedGroup g(r);
    return launch_runs(k_typed_acc<C>, g.nseg, r.total, cfg, s, static_cast<const T *>(in),
                       static_cast<T *>(io), g.seg_off, g.prefix, g.src_off, r.d_tile, g.nseg,
                       r.origin.prefix, r.origin.off, r.origin.tile, r.total, run_params(prm));
}

template <class C>
hipError_t launch_typed_getacc(const void *in, void *res, void *io, const TypedRuns &r,
                               const Params &prm, const LaunchCfg &cfg, hipStream_t s)
{
    using T = typename C::unit;
    const TypedGroup g(r);
    return launch_runs(k_typed_getacc<C>, g.nseg, r.total, cfg, s, static_cast<const T *>(in),
                       static_cast<T *>(res), static_cast<T *>(io), g.seg_off, g.prefix, g.src_off,
                       r.d_tile, g.nseg, r.origin.prefix, r.origin.off, r.origin.tile,
                       r.result.prefix, r.result.off, r.result.tile, r.total, run_params(prm));
}

template <class T>
hipError_t launch_typed_copy_as(int mode, const void *in, void *res, void *io, const TypedRuns &r,
                                const LaunchCfg &cfg, hipStream_t s)
{
    auto kernel = mode == kPlanGather    ? k_typed_copy<T, kPlanGather>
                  : mode == kPlanSwap    ? k_typed_copy<T, kPlanSwap>
                  : mode == kPlanScatter ? k_typed_copy<T, kPlanScatter>
                                         : nullptr;
    if (!kernel)
        return hipErrorInvalidValue;
    const TypedGroup g(r);
    return launch_runs(kernel, g.nseg, r.total, cfg, s, static_cast<const T *>(in),
                       static_cast<T *>(res), static_cast<T *>(io), g.seg_off, g.prefix, g.src_off,
                       r.d_tile, g.nseg, r.origin.prefix, r.origin.off, r.origin.tile,
                       r.result.prefix, r.result.off, r.result.tile, r.total);
}

template <class C> struct MakeTyped {
    static constexpr TypedEntry get()
    {
        return TypedEntry{&launch_typed_acc<C>, &launch_typed_getacc<C>};
    }
};

// ---------------------------------------------------------------------------
// MPI_Compare_and_swap's local step on one element of 1, 2, 4, 8 or 16 bytes
// (posix_rma.h:605-608): plain loads and stores, stream-ordered like every
// other entry; the four addresses need no alignment.
template <class U>
__global__ void __launch_bounds__(64)
k_cas(const void *origin, const void *compare, void *result, void *target)
{
    typedef U UU __attribute__((aligned(1)));
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    const U t = *static_cast<const UU *>(target);
    const U c = *static_cast<const UU *>(compare);
    const U o = *static_cast<const UU *>(origin);
    *static_cast<UU *>(result) = t;
    if (t == c)
        *static_cast<UU *>(target) = o;
}

// The launchers of combiner C as one table entry of each family: the makers
// redop_tables.h builds the (type, op) tables over.
template <class C> struct MakeEntry {
    static constexpr Entry get()
    {
        return Entry{&launch_contig<C>, &launch_vector<C>, &launch_multi<C>, &launch_iov<C>,
                     &launch_tree<C>, &launch_batch<C>};
    }
};

}  // namespace mpix
