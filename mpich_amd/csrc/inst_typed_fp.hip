// inst_typed_fp.hip -- the typed accumulate / get-accumulate kernels (a datatype
// on every side) of the floating-point and complex combiners: redop_tables.h's fp table over MakeTyped.
#include "redop_tables.h"

namespace mpix {

const TypedEntry *lookup_typed_fp(int raw, int opi)
{
    return table_fp<TypedEntry, MakeTyped>(raw, opi);
}

}  // namespace mpix
