// inst_plan_copy.hip -- the committed plans' type-map copy kernel (gather, swap,
// scatter), one instantiation per unit body and mode, as inst_getacc_copy.hip's.
#include "redop_kernels.h"

namespace mpix {

hipError_t launch_plan_copy(CopyMode mode, uint32_t extent, uint32_t value_bytes, uint32_t loc_off,
                            const void *origin, void *result, void *target, const int64_t *d_tab,
                            const int32_t *d_tile, int64_t nseg, uint64_t total,
                            const LaunchCfg &cfg, hipStream_t s)
{
    return with_copy_body(extent, value_bytes, loc_off, [&](auto body) {
        return launch_plan_copy_as<decltype(body)>((int) mode, origin, result, target, d_tab, d_tile,
                                                   nseg, total, cfg, s);
    });
}

}  // namespace mpix
