// inst_getacc_pair.hip -- the fused get-accumulate kernels
// of MAXLOC / MINLOC: redop_tables.h's pair table over MakeGetacc.
#include "redop_tables.h"

namespace mpix {

const GetaccEntry *lookup_getacc_pair(int raw, int opi)
{
    return table_pair<GetaccEntry, MakeGetacc>(raw, opi);
}

}  // namespace mpix
