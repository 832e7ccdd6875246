// redop_atomic.h -- the element-atomic accumulate family (AtomicEntry,
// MPIX_[Get_]accumulate_local_atomic*, MPIX_Compare_and_swap_local_atomic*).
//
// For every element the read-modify-write target = target OP origin is one
// atomic step at device (agent) scope on the aligned 32- or 64-bit word that
// holds the element, so calls from any stream, thread or process that has the
// target mapped on this device never lose each other's updates.  The combine
// is the reduction's own C::apply with the target in the inout role: a caller
// that runs alone leaves the bits MPIX_Get_accumulate_local_async leaves.
//
// General form, a compare-exchange loop: relaxed atomic load of the word,
// new = bits(C::apply(value(old), in)), compare-exchange; on failure retry
// with the word the exchange returned.  The loop compares BIT PATTERNS, never
// floating-point values, so a NaN in the target cannot keep it spinning, and
// it is lock-free: an exchange fails only because another one succeeded.
// When new == old in bits the exchange is skipped and the load is the
// linearisation point (MAX / MIN / the LOC ops that do not win, MPI_NO_OP).
//
// 1- and 2-byte units: one lane per aligned dword of the target, not per
// element -- the lane combines the 4 or 2 elements of its dword into the old
// word and issues one exchange, so no two lanes of a call contend for a word.
// In the head and tail dwords only the bytes inside [target, target + count)
// change; the others are carried over from `old`, and the exchange fails and
// retries when a neighbour changed them meanwhile.
//
// Native read-modify-write where the instruction is the combiner by
// construction: integer SUM, BAND, BOR, BXOR, MAX, MIN at 32 and 64 bits and
// MPI_REPLACE of an unpadded unit (global_atomic_add / and / or / xor / smax /
// umax / smin / umin / swap, without return in the non-fetch form).  Every
// floating-point op, SUM included, stays on the loop.
#pragma once

#include "redop_kernels.h"

namespace mpix {

#define MPIX_ATOM_LOAD(p) __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define MPIX_ATOM_CAS(p, expected, desired)                                             \
    __hip_atomic_compare_exchange_strong(p, expected, desired, __ATOMIC_RELAXED,        \
                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// the unsigned integer of N bytes: the exchanged word (4, 8) or a sub-dword
// element's bits (1, 2)
template <int N> struct AtomBits;
template <> struct AtomBits<1> { using type = uint8_t; };
template <> struct AtomBits<2> { using type = uint16_t; };
template <> struct AtomBits<4> { using type = uint32_t; };
template <> struct AtomBits<8> { using type = uint64_t; };

// MPI_NO_OP and MPI_REPLACE as combiners over a unit body T (a raw unit of the
// extent, or the padded pair): the fetch keeps the target, the swap lays the
// origin's type map over it (FetchStore: a padded pair's padding stays the
// target's).
template <class T> struct AtomFetch {
    using unit = T;
    static constexpr bool kReadsOrigin = false;
    static __device__ __forceinline__ T apply(T a, T, const Params &) { return a; }
};
template <class T> struct AtomSwap {
    using unit = T;
    static __device__ __forceinline__ T apply(T a, T b, const Params &)
    {
        if constexpr (!FetchStore<T>::whole) {
            a.v = b.v;
            a.l = b.l;
            return a;
        } else {
            return b;
        }
    }
};

template <class C, class = void> struct atom_reads_origin : std::true_type {};
template <class C> struct atom_reads_origin<C, std::void_t<decltype(C::kReadsOrigin)>>
    : std::integral_constant<bool, C::kReadsOrigin> {};

// How a combiner's step is issued on a 4- or 8-byte unit
enum AtomKind { kAtomLoop, kAtomAdd, kAtomAnd, kAtomOr, kAtomXor, kAtomMax, kAtomMin, kAtomXchg };
template <typename T> constexpr bool atom_native_int = sizeof(T) == 4 || sizeof(T) == 8;
template <class C> struct AtomKindOf { static constexpr int value = kAtomLoop; };
#define MPIX_ATOM_NATIVE(COMB, KIND)                                                \
    template <typename T> struct AtomKindOf<COMB<T>> {                              \
        static constexpr int value = atom_native_int<T> ? KIND : kAtomLoop;         \
    }
MPIX_ATOM_NATIVE(ISum, kAtomAdd);
MPIX_ATOM_NATIVE(IBand, kAtomAnd);
MPIX_ATOM_NATIVE(IBor, kAtomOr);
MPIX_ATOM_NATIVE(IBxor, kAtomXor);
MPIX_ATOM_NATIVE(IMax, kAtomMax);
MPIX_ATOM_NATIVE(IMin, kAtomMin);
#undef MPIX_ATOM_NATIVE
template <typename T> struct AtomKindOf<AtomSwap<T>> {
    static constexpr int value = (FetchStore<T>::whole && atom_native_int<T>) ? kAtomXchg : kAtomLoop;
};

// the native step on an integer element: the element's value before it
template <int K, bool FETCH, typename T> __device__ __forceinline__ T atom_native(T *p, T b)
{
    constexpr int O = __ATOMIC_RELAXED, S = __HIP_MEMORY_SCOPE_AGENT;
    if constexpr (K == kAtomAdd) {
        return __hip_atomic_fetch_add(p, b, O, S);
    } else if constexpr (K == kAtomAnd) {
        return __hip_atomic_fetch_and(p, b, O, S);
    } else if constexpr (K == kAtomOr) {
        return __hip_atomic_fetch_or(p, b, O, S);
    } else if constexpr (K == kAtomXor) {
        return __hip_atomic_fetch_xor(p, b, O, S);
    } else if constexpr (K == kAtomMax) {
        return __hip_atomic_fetch_max(p, b, O, S);
    } else if constexpr (K == kAtomMin) {
        return __hip_atomic_fetch_min(p, b, O, S);
    } else if constexpr (FETCH) {
        return __hip_atomic_exchange(p, b, O, S);
    } else {
        __hip_atomic_store(p, b, O, S);     // MPI_REPLACE without a result: a store
        return b;
    }
}

// 4- and 8-byte units, one lane per element; consecutive lanes take
// consecutive elements, so a wave's atomics cover one contiguous 256 or 512
// bytes.  `res` is read only by FETCH, `in` only by combiners that read it.
template <class C, bool FETCH>
__global__ void __launch_bounds__(1024)
k_acc_atomic(const typename C::unit *__restrict__ in, typename C::unit *__restrict__ res,
             typename C::unit *io, uint64_t n, Params prm, uint32_t nblk, uint32_t nt)
{
    using T = typename C::unit;
    using W = typename AtomBits<sizeof(T)>::type;
    constexpr int K = AtomKindOf<C>::value;
    const uint64_t stride = (uint64_t) nblk * nt;
    for (uint64_t i = (uint64_t) blockIdx.x * nt + threadIdx.x; i < n; i += stride) {
        T b{};
        if constexpr (atom_reads_origin<C>::value)
            b = in[i];
        W old;
        if constexpr (K == kAtomLoop) {
            W *w = reinterpret_cast<W *>(io + i);
            old = MPIX_ATOM_LOAD(w);
            for (;;) {
                const W nw = __builtin_bit_cast(W, C::apply(__builtin_bit_cast(T, old), b, prm));
                if (nw == old || MPIX_ATOM_CAS(w, &old, nw))
                    break;
            }
        } else {
            old = __builtin_bit_cast(W, atom_native<K, FETCH>(io + i, b));
        }
        if constexpr (FETCH)
            FetchStore<T>::st(res + i, __builtin_bit_cast(T, old));
    }
}

// 1- and 2-byte units, one lane per aligned dword of the target.  Slot k of
// dword d is element d * E + k - ph, where ph is the first element's slot in
// dword 0 (the target's phase); slots outside [ph, ph + n) keep old's bytes.
// Origin and result are packed and only element-aligned: element-wise access.
template <class C, bool FETCH>
__global__ void __launch_bounds__(1024)
k_acc_atomic_sub(const typename C::unit *__restrict__ in, typename C::unit *__restrict__ res,
                 uint32_t *base, uint32_t ph, uint64_t n, uint64_t ndw, Params prm, uint32_t nblk,
                 uint32_t nt)
{
    using T = typename C::unit;
    using U = typename AtomBits<sizeof(T)>::type;
    constexpr int E = 4 / sizeof(T), B = 8 * sizeof(T);
    constexpr uint32_t kOnes = (uint32_t) (U) ~(U) 0;
    const uint64_t stride = (uint64_t) nblk * nt;
    for (uint64_t d = (uint64_t) blockIdx.x * nt + threadIdx.x; d < ndw; d += stride) {
        const uint64_t s0 = d * E;
        uint32_t bw = 0, mask = 0;
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const uint64_t s = s0 + k;
            if (s >= ph && s - ph < n) {
                mask |= kOnes << (B * k);
                if constexpr (atom_reads_origin<C>::value)
                    bw |= (uint32_t) __builtin_bit_cast(U, in[s - ph]) << (B * k);
            }
        }
        uint32_t *w = base + d;
        uint32_t old = MPIX_ATOM_LOAD(w);
        for (;;) {
            uint32_t nw = 0;
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const T a = __builtin_bit_cast(T, (U) (old >> (B * k)));
                const T b = __builtin_bit_cast(T, (U) (bw >> (B * k)));
                nw |= (uint32_t) __builtin_bit_cast(U, C::apply(a, b, prm)) << (B * k);
            }
            nw = (nw & mask) | (old & ~mask);
            if (nw == old || MPIX_ATOM_CAS(w, &old, nw))
                break;
        }
        if constexpr (FETCH) {
#pragma unroll
            for (int k = 0; k < E; ++k)
                if ((mask >> (B * k)) & 1u)
                    FetchStore<T>::st(res + (s0 + k - ph), __builtin_bit_cast(T, (U) (old >> (B * k))));
        }
    }
}

// `io` is aligned to the unit (the entries refuse a target that is not).
template <class C, bool FETCH>
hipError_t launch_atomic(const void *in, void *res, void *io, uint64_t count, const Params &prm,
                         const LaunchCfg &cfg, hipStream_t s)
{
    using T = typename C::unit;
    static_assert(sizeof(T) == 1 || sizeof(T) == 2 || sizeof(T) == 4 || sizeof(T) == 8,
                  "no atomic wider than 8 bytes");
    if (count == 0)
        return hipSuccess;
    Params p = prm;
    p.done = nullptr;       // the entries wait on the stream
    p.fixup = nullptr;
    if constexpr (sizeof(T) >= 4) {
        const unsigned grid = grid_for((uint64_t) cfg.block, count, cfg.max_grid, cfg.block);
        hipLaunchKernelGGL((k_acc_atomic<C, FETCH>), dim3(grid), dim3(cfg.block), 0, s,
                           static_cast<const T *>(in), static_cast<T *>(res), static_cast<T *>(io),
                           count, p, grid, (uint32_t) cfg.block);
    } else {
        constexpr uint64_t E = 4 / sizeof(T);
        const uintptr_t a = reinterpret_cast<uintptr_t>(io);
        const uint32_t ph = (uint32_t) ((a & 3) / sizeof(T));
        const uint64_t ndw = (ph + count + E - 1) / E;
        const unsigned grid = grid_for((uint64_t) cfg.block, ndw, cfg.max_grid, cfg.block);
        hipLaunchKernelGGL((k_acc_atomic_sub<C, FETCH>), dim3(grid), dim3(cfg.block), 0, s,
                           static_cast<const T *>(in), static_cast<T *>(res),
                           reinterpret_cast<uint32_t *>(a & ~(uintptr_t) 3), ph, count, ndw, p, grid,
                           (uint32_t) cfg.block);
    }
    return hipGetLastError();
}

template <class C>
hipError_t launch_acc_atomic(const void *in, void *io, uint64_t count, const Params &prm,
                             const LaunchCfg &cfg, hipStream_t s)
{
    return launch_atomic<C, false>(in, nullptr, io, count, prm, cfg, s);
}

// Every combiner of the table gets an entry; one whose unit has no atomic gets
// null launchers.
template <class C> struct MakeAtomic {
    static constexpr AtomicEntry get()
    {
        if constexpr (sizeof(typename C::unit) <= 8)
            return AtomicEntry{&launch_acc_atomic<C>, &launch_atomic<C, true>};
        else
            return AtomicEntry{nullptr, nullptr};
    }
};

// MPI_Compare_and_swap on one aligned integer element: a single
// compare-exchange at 4 and 8 bytes; at 1 and 2 bytes the dword loop, which
// exchanges only while the element equals `compare` and carries the dword's
// other bytes over.  *result = the element before the step.
template <class U>
__global__ void __launch_bounds__(64)
k_cas_atomic(const void *origin, const void *compare, void *result, void *target)
{
    typedef U UU __attribute__((aligned(1)));
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    const U c = *static_cast<const UU *>(compare);
    const U o = *static_cast<const UU *>(origin);
    U old;
    if constexpr (sizeof(U) >= 4) {
        old = c;
        (void) MPIX_ATOM_CAS(static_cast<U *>(target), &old, o);
    } else {
        const uintptr_t a = reinterpret_cast<uintptr_t>(target);
        uint32_t *w = reinterpret_cast<uint32_t *>(a & ~(uintptr_t) 3);
        const unsigned sh = 8 * (unsigned) (a & 3);
        const uint32_t m = (uint32_t) (U) ~(U) 0 << sh;
        uint32_t ow = MPIX_ATOM_LOAD(w);
        for (;;) {
            if ((U) (ow >> sh) != c)
                break;
            const uint32_t nw = (ow & ~m) | ((uint32_t) o << sh);
            if (nw == ow || MPIX_ATOM_CAS(w, &ow, nw))
                break;
        }
        old = (U) (ow >> sh);
    }
    *static_cast<UU *>(result) = old;
}

}  // namespace mpix
