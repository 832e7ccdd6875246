// inst_getacc_iov_int.hip -- the fused get-accumulate's iov-target kernels
// of the integer and Fortran-logical combiners: redop_tables.h's int table over MakeGetaccIov.
#include "redop_tables.h"

namespace mpix {

const GetaccIovEntry *lookup_getacc_iov_int(int raw, int opi)
{
    return table_int<GetaccIovEntry, MakeGetaccIov>(raw, opi);
}

}  // namespace mpix
