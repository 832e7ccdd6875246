// inst_getacc_iov_pair.hip -- the fused get-accumulate's iov-target kernels
// of MAXLOC / MINLOC: redop_tables.h's pair table over MakeGetaccIov.
#include "redop_tables.h"

namespace mpix {

const GetaccIovEntry *lookup_getacc_iov_pair(int raw, int opi)
{
    return table_pair<GetaccIovEntry, MakeGetaccIov>(raw, opi);
}

}  // namespace mpix
