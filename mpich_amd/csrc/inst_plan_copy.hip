// inst_plan_copy.hip -- the committed plans' type-map copy kernel (gather, swap,
// scatter), one instantiation per unit body and mode, as inst_getacc_copy.hip's.
#include "redop_kernels.h"

namespace mpix {

namespace {

// a 32-byte unit (the x87 / binary128 complex types) at the 16-byte alignment
// of their combiners' units
struct alignas(16) Raw32 {
    v4u lo, hi;
};

}  // namespace

hipError_t launch_plan_copy(int mode, uint32_t extent, uint32_t value_bytes, uint32_t loc_off,
                            const void *origin, void *result, void *target, const int64_t *d_tab,
                            const int32_t *d_tile, int64_t nseg, uint64_t total,
                            const LaunchCfg &cfg, hipStream_t s)
{
#define MPIX_COPY_AS(T)                                                                         \
    return launch_plan_copy_as<T>(mode, origin, result, target, d_tab, d_tile, nseg, total, cfg, s)
    if (value_bytes) {      // the padded pairs, member by member (FetchStore)
        if (extent == 16 && value_bytes == 8 && loc_off == 8)
            MPIX_COPY_AS(DoubleIntBody);        // MPI_LONG_INT has the same map
        if (extent == 8 && value_bytes == 2 && loc_off == 4)
            MPIX_COPY_AS(ShortInt);
        if (extent == 32 && value_bytes == 16 && loc_off == 16)
            MPIX_COPY_AS(LongDoubleInt);
        return hipErrorInvalidValue;
    }
    switch (extent) {
        case 1: MPIX_COPY_AS(uint8_t);
        case 2: MPIX_COPY_AS(RawOf<2>::type);
        case 4: MPIX_COPY_AS(RawOf<4>::type);
        case 8: MPIX_COPY_AS(RawOf<8>::type);
        case 16: MPIX_COPY_AS(RawOf<16>::type);
        case 32: MPIX_COPY_AS(Raw32);
        default: return hipErrorInvalidValue;
    }
#undef MPIX_COPY_AS
}

}  // namespace mpix
