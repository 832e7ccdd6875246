// redop_packed.h -- the packed-order table of a committed plan and its one
// lookup, shared by the host (MPIX_Iov_plan_locate, redop_capi.cpp) and the
// typed kernels (k_typed_*, redop_kernels.h): what the CPU tests prove about
// packed_run is what the GPU runs.
//
// A plan's device table (RunGroup) is grouped by residue and driven from the
// target side.  "Where is packed element p of this layout" needs one table
// over ALL merged runs in call order, as it lies in memory on the host and on
// the device:
//   prefix[nrun + 1]  packed elements before each run (prefix[nrun] = total)
//   off[nrun]         each run's byte offset from the buffer pointer (may be
//                     negative)
//   tile[ntile + 1]   32-bit: tile[t] = the run that holds packed index 256 t,
//                     closed by tile[ntile] = nrun - 1 (ntile = ceil(total / 256))
// A plan of at most one run keeps none: its one offset is enough.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace mpix {

struct PackedTab {
    const int64_t *prefix, *off;
    const int32_t *tile;
    // the table of `nrun` runs and `total` elements at `tab` (host or device)
    PackedTab(const char *tab, int64_t nrun)
        : prefix((const int64_t *) tab), off((const int64_t *) tab + nrun + 1),
          tile((const int32_t *) ((const int64_t *) tab + 2 * nrun + 1)) {}
    PackedTab() : prefix(nullptr), off(nullptr), tile(nullptr) {}
};

inline size_t packed_tab_bytes(int64_t nrun, uint64_t total)
{
    return (size_t) (2 * nrun + 1) * sizeof(int64_t) +
           (size_t) ((total + 255) / 256 + 1) * sizeof(int32_t);
}

// The run of packed index p < total: the two tile bounds, no search when they
// are equal, else a search of `prefix` between them only (the last s in
// [lo, hi] with prefix[s] <= p, as iov_search).
__host__ __device__ inline int64_t packed_run(const int64_t *prefix, const int32_t *tile,
                                              uint64_t p)
{
    int64_t lo = tile[p >> 8], hi = tile[(p >> 8) + 1];
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if ((uint64_t) prefix[mid] <= p)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// Byte offset, relative to the buffer pointer, of packed element p of a layout
// whose elements are `extent` bytes apart.
__host__ __device__ inline int64_t packed_byte(const int64_t *prefix, const int64_t *off,
                                               const int32_t *tile, uint64_t p, int64_t extent)
{
    const int64_t s = packed_run(prefix, tile, p);
    return off[s] + (int64_t) (p - (uint64_t) prefix[s]) * extent;
}

}  // namespace mpix
