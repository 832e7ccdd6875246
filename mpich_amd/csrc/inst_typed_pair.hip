// inst_typed_pair.hip -- the typed accumulate / get-accumulate kernels (a datatype
// on every side) of MAXLOC / MINLOC: redop_tables.h's pair table over MakeTyped.
#include "redop_tables.h"

namespace mpix {

const TypedEntry *lookup_typed_pair(int raw, int opi)
{
    return table_pair<TypedEntry, MakeTyped>(raw, opi);
}

}  // namespace mpix
