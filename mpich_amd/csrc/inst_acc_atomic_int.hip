// inst_acc_atomic_int.hip -- the element-atomic accumulate kernels
// of the integer and Fortran-logical combiners: redop_tables.h's int table over MakeAtomic.
#include "redop_atomic.h"
#include "redop_tables.h"

namespace mpix {

const AtomicEntry *lookup_acc_atomic_int(int raw, int opi)
{
    return table_int<AtomicEntry, MakeAtomic>(raw, opi);
}

}  // namespace mpix
