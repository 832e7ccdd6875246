// inst_getacc_iov_fp.hip -- the fused get-accumulate's iov-target kernels
// of the floating-point and complex combiners: redop_tables.h's fp table over MakeGetaccIov.
#include "redop_tables.h"

namespace mpix {

const GetaccIovEntry *lookup_getacc_iov_fp(int raw, int opi)
{
    return table_fp<GetaccIovEntry, MakeGetaccIov>(raw, opi);
}

}  // namespace mpix
