// inst_plan_pair.hip -- the committed-plan kernels (reduce and fetch form)
// of MAXLOC / MINLOC: redop_tables.h's pair table over MakePlan.
#include "redop_tables.h"

namespace mpix {

const PlanEntry *lookup_plan_pair(int raw, int opi)
{
    return table_pair<PlanEntry, MakePlan>(raw, opi);
}

}  // namespace mpix
