// inst_getacc_copy.hip -- the fetching entries' kernels that belong to no
// combiner: the iov target's MPI_NO_OP / MPI_REPLACE copy kernel, one
// instantiation per unit body, and MPI_Compare_and_swap's one-element kernel.
#include "redop_kernels.h"

namespace mpix {

hipError_t launch_getacc_iov_copy(CopyMode mode, uint32_t extent, uint32_t value_bytes,
                                  uint32_t loc_off, const void *origin, void *result, void *target,
                                  const int64_t *d_seg_off, const int64_t *d_prefix,
                                  const int64_t *d_src_off, int64_t nseg, uint64_t total,
                                  const LaunchCfg &cfg, hipStream_t s)
{
    return with_copy_body(extent, value_bytes, loc_off, [&](auto body) {
        return launch_getacc_iov_copy_as<decltype(body)>(mode != kCopyFetch, origin, result, target,
                                                         d_seg_off, d_prefix, d_src_off, nseg,
                                                         total, cfg, s);
    });
}

hipError_t launch_cas(uint32_t size, const void *origin, const void *compare, void *result,
                      void *target, hipStream_t s)
{
#define MPIX_CAS_AS(U)                                                                        \
    hipLaunchKernelGGL((k_cas<U>), dim3(1), dim3(64), 0, s, origin, compare, result, target); \
    break
    switch (size) {
        case 1: MPIX_CAS_AS(uint8_t);
        case 2: MPIX_CAS_AS(uint16_t);
        case 4: MPIX_CAS_AS(uint32_t);
        case 8: MPIX_CAS_AS(uint64_t);
        case 16: MPIX_CAS_AS(unsigned __int128);
        default: return hipErrorInvalidValue;
    }
#undef MPIX_CAS_AS
    return hipGetLastError();
}

}  // namespace mpix
