// inst_typed_copy.hip -- the typed entries' type-map copy kernel (MPI_Get into a
// derived result, the swap, MPI_Put from a derived origin), one instantiation
// per unit body and mode, as inst_plan_copy.hip's.
#include "redop_kernels.h"

namespace mpix {

hipError_t launch_typed_copy(CopyMode mode, uint32_t extent, uint32_t value_bytes, uint32_t loc_off,
                             const void *origin, void *result, void *target, const TypedRuns &runs,
                             const LaunchCfg &cfg, hipStream_t s)
{
    return with_copy_body(extent, value_bytes, loc_off, [&](auto body) {
        return launch_typed_copy_as<decltype(body)>((int) mode, origin, result, target, runs, cfg,
                                                    s);
    });
}

}  // namespace mpix
