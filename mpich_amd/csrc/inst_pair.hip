// inst_pair.hip -- MAXLOC / MINLOC over builtin pairs {T v; T loc}
// (MPIR_2INT8.. MPIR_2FLOAT64, op_fns.c:303-330) and the struct pair types
// MPI_{FLOAT,DOUBLE,LONG,SHORT,LONG_DOUBLE}_INT {T v; int loc} (op_fns.c:337-352,
// pairtypes.c:15-121), and MPIR_2FLOAT128.
// The reduction's kernels of redop_tables.h's pair table.
#include "redop_tables.h"

namespace mpix {

const Entry *lookup_pair(int raw, int opi)
{
    return table_pair<Entry, MakeEntry>(raw, opi);
}

}  // namespace mpix
