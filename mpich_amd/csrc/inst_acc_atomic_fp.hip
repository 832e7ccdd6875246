// inst_acc_atomic_fp.hip -- the element-atomic accumulate kernels
// of the floating-point and complex combiners: redop_tables.h's fp table over MakeAtomic.
#include "redop_atomic.h"
#include "redop_tables.h"

namespace mpix {

const AtomicEntry *lookup_acc_atomic_fp(int raw, int opi)
{
    return table_fp<AtomicEntry, MakeAtomic>(raw, opi);
}

}  // namespace mpix
