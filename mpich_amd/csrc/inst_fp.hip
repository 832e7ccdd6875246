// inst_fp.hip -- floating-point and complex combiners
// (MPIR_OP_TYPE_GROUP(FLOATING_POINT) / (C_COMPLEX) / (COMPLEX) and the bf16
// SUM helper, src/include/mpir_op_util.h:211-236, op_fns.c:19-91,459-493).
// The reduction's kernels of redop_tables.h's fp table.
#include "redop_tables.h"

namespace mpix {

const Entry *lookup_fp(int raw, int opi)
{
    return table_fp<Entry, MakeEntry>(raw, opi);
}

int unroll() { return MPIX_REDOP_UNROLL; }

}  // namespace mpix

#define MPIX_STR2(x) #x
#define MPIX_STR(x) MPIX_STR2(x)
extern "C" const char *mpix_build_info(void)
{
    return "libmpix_redop gfx950 HIP " MPIX_STR(HIP_VERSION_MAJOR) "." MPIX_STR(HIP_VERSION_MINOR)
        " unroll=" MPIX_STR(MPIX_REDOP_UNROLL) " nt_load=" MPIX_STR(MPIX_REDOP_NT_LOAD)
        " nt_store=" MPIX_STR(MPIX_REDOP_NT_STORE) " grouped_loads=" MPIX_STR(MPIX_REDOP_GROUPED_LOADS);
}
