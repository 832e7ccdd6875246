// inst_acc_atomic_copy.hip -- the atomic entries' kernels that belong to no
// combiner: MPI_NO_OP (atomic load) and MPI_REPLACE (atomic exchange / store)
// per unit body, and MPI_Compare_and_swap's one-element compare-exchange.
#include "redop_atomic.h"

namespace mpix {

namespace {
template <class T>
hipError_t atomic_copy_as(int mode, const void *origin, void *result, void *target, uint64_t count,
                          const LaunchCfg &cfg, hipStream_t s)
{
    const Params prm{};
    switch (mode) {
        case 0: return launch_atomic<AtomFetch<T>, true>(origin, result, target, count, prm, cfg, s);
        case 1: return launch_atomic<AtomSwap<T>, true>(origin, result, target, count, prm, cfg, s);
        case 2: return launch_atomic<AtomSwap<T>, false>(origin, result, target, count, prm, cfg, s);
        default: return hipErrorInvalidValue;
    }
}
}  // namespace

hipError_t launch_atomic_copy(CopyMode mode, uint32_t extent, uint32_t value_bytes, uint32_t loc_off,
                              const void *origin, void *result, void *target, uint64_t count,
                              const LaunchCfg &cfg, hipStream_t s)
{
    if (value_bytes) {
        if (extent == 8 && value_bytes == 2 && loc_off == 4)
            return atomic_copy_as<ShortInt>((int) mode, origin, result, target, count, cfg, s);
        return hipErrorInvalidValue;
    }
    switch (extent) {
        case 1: return atomic_copy_as<uint8_t>((int) mode, origin, result, target, count, cfg, s);
        case 2: return atomic_copy_as<uint16_t>((int) mode, origin, result, target, count, cfg, s);
        case 4: return atomic_copy_as<uint32_t>((int) mode, origin, result, target, count, cfg, s);
        case 8: return atomic_copy_as<uint64_t>((int) mode, origin, result, target, count, cfg, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_cas_atomic(uint32_t size, const void *origin, const void *compare, void *result,
                             void *target, hipStream_t s)
{
#define MPIX_CAS_AS(U)                                                                        \
    hipLaunchKernelGGL((k_cas_atomic<U>), dim3(1), dim3(64), 0, s, origin, compare, result,   \
                       target);                                                               \
    break
    switch (size) {
        case 1: MPIX_CAS_AS(uint8_t);
        case 2: MPIX_CAS_AS(uint16_t);
        case 4: MPIX_CAS_AS(uint32_t);
        case 8: MPIX_CAS_AS(uint64_t);
        default: return hipErrorInvalidValue;
    }
#undef MPIX_CAS_AS
    return hipGetLastError();
}

}  // namespace mpix
