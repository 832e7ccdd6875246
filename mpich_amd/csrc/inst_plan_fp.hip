// inst_plan_fp.hip -- the committed-plan kernels (reduce and fetch form)
// of the floating-point and complex combiners: redop_tables.h's fp table over MakePlan.
#include "redop_tables.h"

namespace mpix {

const PlanEntry *lookup_plan_fp(int raw, int opi)
{
    return table_fp<PlanEntry, MakePlan>(raw, opi);
}

}  // namespace mpix
