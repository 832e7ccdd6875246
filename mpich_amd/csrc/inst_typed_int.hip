// inst_typed_int.hip -- the typed accumulate / get-accumulate kernels (a datatype
// on every side) of the integer and Fortran-logical combiners: redop_tables.h's int table over MakeTyped.
#include "redop_tables.h"

namespace mpix {

const TypedEntry *lookup_typed_int(int raw, int opi)
{
    return table_int<TypedEntry, MakeTyped>(raw, opi);
}

}  // namespace mpix
