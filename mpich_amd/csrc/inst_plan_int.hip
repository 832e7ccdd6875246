// inst_plan_int.hip -- the committed-plan kernels (reduce and fetch form)
// of the integer and Fortran-logical combiners: redop_tables.h's int table over MakePlan.
#include "redop_tables.h"

namespace mpix {

const PlanEntry *lookup_plan_int(int raw, int opi)
{
    return table_int<PlanEntry, MakePlan>(raw, opi);
}

}  // namespace mpix
