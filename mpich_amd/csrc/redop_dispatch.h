// redop_dispatch.h -- host-visible interface between the C-ABI
// (redop_capi.cpp, plain host C++) and the kernel instantiation units
// (inst_*.hip).  No device code here.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "redop_launch.h"
#include "redop_packed.h"

namespace mpix {

// Params, LaunchCfg, grid_for and max_blocks: redop_launch.h
constexpr unsigned kSignalMaxGrid = 64;     // 64 tiles of 64 x 1 packets: 64 KiB per operand

// One (op, type) pair: launchers for the contiguous and the vector-target form.
struct Entry {
    hipError_t (*contig)(const void *in, void *io, uint64_t count, const Params &,
                         const LaunchCfg &, hipStream_t);
    hipError_t (*vector)(const void *in, void *io, uint64_t count, uint64_t blocklen,
                         uint64_t stride, const Params &, const LaunchCfg &, hipStream_t);
    hipError_t (*multi)(const void *const *ins, int k, void *io, uint64_t count, const Params &,
                        const LaunchCfg &, hipStream_t);
    hipError_t (*iov)(const void *in, void *io, const int64_t *d_seg_off, const int64_t *d_prefix,
                      const int64_t *d_src_off, int64_t nseg, uint64_t total, const Params &,
                      const LaunchCfg &, hipStream_t);
    hipError_t (*tree)(const void *const *ins, int k, void *out, uint64_t count, const Params &,
                       const LaunchCfg &, hipStream_t);
    hipError_t (*batch)(const void *const *ins, void *const *ios, const uint64_t *counts, int k,
                        const Params &, const LaunchCfg &, hipStream_t);
};

constexpr int kMaxBatchSegs = 64;       // MPIX_BATCH_MAX

constexpr int kMaxMultiInputs = 16;

// Each instantiation unit resolves (raw internal type, op index) to an Entry
// or returns nullptr.  raw = handle & 0xffffff00 for builtins; struct pair
// handles 0x8c00000k are passed unchanged.  The six kernel families below
// (Entry, GetaccEntry, GetaccIovEntry, PlanEntry, TypedEntry, AtomicEntry) are
// built from the one (type, op) table of redop_tables.h, each in instantiation units of
// its own that compile side by side, so a pair has an entry in all of them or
// in none (AtomicEntry: with null launchers where the unit has no atomic).
const Entry *lookup_int(int raw, int opi);
const Entry *lookup_fp(int raw, int opi);
const Entry *lookup_pair(int raw, int opi);

// One residue group's run table as it lies in memory, on the host or on the
// device: [seg_off n][prefix n+1][src_off n] -- each run's element offset into
// the target, the packed elements of the group before it (prefix[n] = the
// group's total), and its first element's index in the packed operands.
struct RunGroup {
    const int64_t *seg_off, *prefix, *src_off;
    RunGroup(const int64_t *tab, int64_t n)
        : seg_off(tab), prefix(tab + n), src_off(tab + 2 * n + 1) {}
};

// The fused get-accumulate (MPIX_Get_accumulate_local*): result = target,
// target = target OP origin in one pass (inst_getacc_*.hip).
struct GetaccEntry {
    hipError_t (*contig)(const void *origin, void *result, void *target, uint64_t count,
                         const Params &, const LaunchCfg &, hipStream_t);
    hipError_t (*vector)(const void *origin, void *result, void *target, uint64_t count,
                         uint64_t blocklen, uint64_t stride, const Params &, const LaunchCfg &,
                         hipStream_t);
};

const GetaccEntry *lookup_getacc_int(int raw, int opi);
const GetaccEntry *lookup_getacc_fp(int raw, int opi);
const GetaccEntry *lookup_getacc_pair(int raw, int opi);

// The fetch form over an iov target (MPIX_Get_accumulate_local_iov[ec]_async):
// Entry::iov's run table with the packed result beside the packed origin, both
// indexed by d_src_off (inst_getacc_iov_*.hip).
struct GetaccIovEntry {
    hipError_t (*iov)(const void *origin, void *result, void *target, const int64_t *d_seg_off,
                      const int64_t *d_prefix, const int64_t *d_src_off, int64_t nseg,
                      uint64_t total, const Params &, const LaunchCfg &, hipStream_t);
};

const GetaccIovEntry *lookup_getacc_iov_int(int raw, int opi);
const GetaccIovEntry *lookup_getacc_iov_fp(int raw, int opi);
const GetaccIovEntry *lookup_getacc_iov_pair(int raw, int opi);

// What the copy launchers of MPI_NO_OP / MPI_REPLACE do with the target's
// elements: load them into the packed result (the fetch forms' MPI_NO_OP), also
// put the packed origin in their place (their MPI_REPLACE), or only that (the
// forms without a result).
enum CopyMode { kCopyFetch = 0, kCopySwap = 1, kCopyStore = 2 };

// kCopyFetch (gather the runs into the packed result) and kCopySwap (then
// scatter the packed origin's type map over the runs) on the same table, one
// launch: elements of `extent` bytes whose type map is the whole extent
// (value_bytes == 0) or a value of value_bytes at 0 and an int at loc_off (the
// padded pairs).  hipErrorInvalidValue for a layout without a kernel.
// inst_getacc_copy.hip.
hipError_t launch_getacc_iov_copy(CopyMode mode, uint32_t extent, uint32_t value_bytes,
                                  uint32_t loc_off, const void *origin, void *result, void *target,
                                  const int64_t *d_seg_off, const int64_t *d_prefix,
                                  const int64_t *d_src_off, int64_t nseg, uint64_t total,
                                  const LaunchCfg &, hipStream_t);

// The reduce and the fetch form over a committed plan (MPIX_Iov_plan,
// MPIX_*_local_plan*): one residue group's resident table d_tab (RunGroup's
// layout) and its per-tile index d_tile (the run holding packed index 256 t,
// closed by nseg - 1) (inst_plan_*.hip).
struct PlanEntry {
    hipError_t (*reduce)(const void *in, void *io, const int64_t *d_tab, const int32_t *d_tile,
                         int64_t nseg, uint64_t total, const Params &, const LaunchCfg &,
                         hipStream_t);
    hipError_t (*getacc)(const void *origin, void *result, void *target, const int64_t *d_tab,
                         const int32_t *d_tile, int64_t nseg, uint64_t total, const Params &,
                         const LaunchCfg &, hipStream_t);
};

const PlanEntry *lookup_plan_int(int raw, int opi);
const PlanEntry *lookup_plan_fp(int raw, int opi);
const PlanEntry *lookup_plan_pair(int raw, int opi);

// The type-map copies over the same tables: kCopyFetch gathers the runs into
// the packed result, kCopySwap also scatters the packed origin over them,
// kCopyStore scatters only (the reduce form's MPI_REPLACE, result unused).
// Layouts as launch_getacc_iov_copy.  inst_plan_copy.hip.
hipError_t launch_plan_copy(CopyMode mode, uint32_t extent, uint32_t value_bytes, uint32_t loc_off,
                            const void *origin, void *result, void *target, const int64_t *d_tab,
                            const int32_t *d_tile, int64_t nseg, uint64_t total,
                            const LaunchCfg &, hipStream_t);

// Accumulate and get-accumulate with a datatype on every side
// (MPIX_[Get_]accumulate_local_typed*): one residue group of the TARGET plan
// drives the launch as in PlanEntry (d_tab == nullptr: a target of one run,
// target element j = packed element j), and packed element p of the origin and
// of the result is found through that side's packed-order table (PackedTab,
// redop_packed.h; a null `prefix`: element p lies at base + p -- a packed
// operand, or one run whose offset the host has added to the base)
// (inst_typed_*.hip).
struct TypedRuns {
    const int64_t *d_tab;
    const int32_t *d_tile;
    int64_t nseg;
    uint64_t total;
    PackedTab origin, result;
};

struct TypedEntry {
    hipError_t (*acc)(const void *origin, void *target, const TypedRuns &, const Params &,
                      const LaunchCfg &, hipStream_t);
    hipError_t (*getacc)(const void *origin, void *result, void *target, const TypedRuns &,
                         const Params &, const LaunchCfg &, hipStream_t);
};

const TypedEntry *lookup_typed_int(int raw, int opi);
const TypedEntry *lookup_typed_fp(int raw, int opi);
const TypedEntry *lookup_typed_pair(int raw, int opi);

// The type-map copies of the same calls: kCopyFetch gathers the target into the
// result layout (MPI_Get), kCopySwap also puts the origin's elements in their
// place, kCopyStore only that (MPI_Put).  Layouts as launch_getacc_iov_copy.
// inst_typed_copy.hip.
hipError_t launch_typed_copy(CopyMode mode, uint32_t extent, uint32_t value_bytes, uint32_t loc_off,
                             const void *origin, void *result, void *target, const TypedRuns &,
                             const LaunchCfg &, hipStream_t);

// MPI_Compare_and_swap on one integer element of `size` bytes (1, 2, 4, 8,
// 16): *result = *target; if (*target == *compare) *target = *origin.
hipError_t launch_cas(uint32_t size, const void *origin, const void *compare, void *result,
                      void *target, hipStream_t);

// The element-atomic accumulate (MPIX_[Get_]accumulate_local_atomic*): every
// element's target = target OP origin is one device-scope read-modify-write on
// the 32- or 64-bit word that holds it; getacc also stores the element's value
// before that step to the packed result (inst_acc_atomic_*.hip).  The target
// is aligned to the unit.  Both launchers are null for a combiner whose unit
// is wider than 8 bytes: there is no wider atomic, the entries decline it.
struct AtomicEntry {
    hipError_t (*acc)(const void *origin, void *target, uint64_t count, const Params &,
                      const LaunchCfg &, hipStream_t);
    hipError_t (*getacc)(const void *origin, void *result, void *target, uint64_t count,
                         const Params &, const LaunchCfg &, hipStream_t);
};

const AtomicEntry *lookup_acc_atomic_int(int raw, int opi);
const AtomicEntry *lookup_acc_atomic_fp(int raw, int opi);
const AtomicEntry *lookup_acc_atomic_pair(int raw, int opi);

// MPI_NO_OP and MPI_REPLACE of the atomic entries on elements of `extent`
// bytes (1, 2, 4, 8) whose type map is the whole extent (value_bytes == 0) or
// a value and an int (the padded 8-byte pair): kCopyFetch an atomic load per
// element into the result, kCopySwap an atomic exchange of the type map,
// kCopyStore an atomic store of it (no result).  hipErrorInvalidValue for a
// layout without a kernel.  inst_acc_atomic_copy.hip.
hipError_t launch_atomic_copy(CopyMode mode, uint32_t extent, uint32_t value_bytes, uint32_t loc_off,
                              const void *origin, void *result, void *target, uint64_t count,
                              const LaunchCfg &, hipStream_t);

// MPI_Compare_and_swap as one device-scope compare-exchange on an aligned
// integer element of `size` bytes (1, 2, 4, 8); origin, compare and result
// need no alignment.  inst_acc_atomic_copy.hip.
hipError_t launch_cas_atomic(uint32_t size, const void *origin, const void *compare, void *result,
                             void *target, hipStream_t);

// MPIX_EQUAL on an MPI_BYTE buffer of n >= 8 bytes (opequal.c:20-35)
hipError_t launch_equal(const void *in, void *io, uint64_t n, hipStream_t s);

// A device buffer of at least `bytes` for the split combiners' fixup words,
// the caller's from fixup_acquire until fixup_release: it enqueues k_contig32
// and k_fixup32 on `s` in between, and no other caller's pair comes between
// them on that stream (one buffer per device and stream, per calling thread
// for hipStreamPerThread; redop_fixup.h has the lifetime rules).  words is
// nullptr when none can be had: nothing to release then.
struct FixupLease {
    uint64_t *words = nullptr;
    void *entry = nullptr;
};
FixupLease fixup_acquire(hipStream_t s, size_t bytes);
void fixup_release(const FixupLease &lease);

// up to kMaxMultiInputs independent device copies in one launch
hipError_t launch_copy_multi(const void *const *srcs, void *const *dsts, const uint64_t *bytes,
                             int n, hipStream_t s, unsigned wt_xcd = 0);

// compile-time unroll of the packet kernel (packets per lane per operand)
int unroll();

}  // namespace mpix
