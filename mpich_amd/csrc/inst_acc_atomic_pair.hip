// inst_acc_atomic_pair.hip -- the element-atomic accumulate kernels
// of the MAXLOC / MINLOC combiners: redop_tables.h's pair table over MakeAtomic.
#include "redop_atomic.h"
#include "redop_tables.h"

namespace mpix {

const AtomicEntry *lookup_acc_atomic_pair(int raw, int opi)
{
    return table_pair<AtomicEntry, MakeAtomic>(raw, opi);
}

}  // namespace mpix
