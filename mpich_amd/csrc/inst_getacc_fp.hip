// inst_getacc_fp.hip -- the fused get-accumulate kernels
// of the floating-point and complex combiners: redop_tables.h's fp table over MakeGetacc.
#include "redop_tables.h"

namespace mpix {

const GetaccEntry *lookup_getacc_fp(int raw, int opi)
{
    return table_fp<GetaccEntry, MakeGetacc>(raw, opi);
}

}  // namespace mpix
