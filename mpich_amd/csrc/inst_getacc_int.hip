// inst_getacc_int.hip -- the fused get-accumulate kernels
// of the integer and Fortran-logical combiners: redop_tables.h's int table over MakeGetacc.
#include "redop_tables.h"

namespace mpix {

const GetaccEntry *lookup_getacc_int(int raw, int opi)
{
    return table_int<GetaccEntry, MakeGetacc>(raw, opi);
}

}  // namespace mpix
