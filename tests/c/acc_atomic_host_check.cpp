// acc_atomic_host_check.cpp -- the host side of the element-atomic entries
// (MPIX_[Get_]accumulate_local_atomic*, MPIX_Compare_and_swap_local_atomic*,
// MPIX_Accumulate_atomic_is_supported) under AddressSanitizer +
// UndefinedBehaviorSanitizer: built by mpich_amd/csrc/sanitize.mk against the
// sanitizer build of redop_capi.cpp, run on the CPU, nothing preloaded.  Wild
// pointers stand for buffers: every call here is refused, or has nothing to
// do, before a buffer is looked at.
#include <stdint.h>
#include <stdio.h>

#include "mpix_redop.h"

namespace {

int g_errors = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            ++g_errors;                                                    \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);     \
        }                                                                  \
    } while (0)

// handles and error classes of mpix_redop.h / mpi.h as this library numbers them
const MPIX_Datatype kFloat = 0x4c00040a, kDouble = 0x4c00080b, kInt8 = 0x4c000137,
                    kInt16 = 0x4c000238, kInt32 = 0x4c000439, kInt64 = 0x4c00083a,
                    kDoubleInt = (MPIX_Datatype) 0x8c000001, kFloatInt = (MPIX_Datatype) 0x8c000000,
                    kShortInt = (MPIX_Datatype) 0x8c000003,
                    kLongDoubleInt = (MPIX_Datatype) 0x8c000004, kByte = 0x4c00010d,
                    kUnknown = 0x4c0000ff;
const MPIX_Op kMax = 0x58000001, kSum = 0x58000003, kBand = 0x58000006, kMaxloc = 0x5800000c,
              kReplace = 0x5800000d, kNoOp = 0x5800000e, kEqual = 0x5800000f, kNullOp = 0x18000000;
enum { OK = 0, BUFFER = 1, COUNT = 2, TYPE = 3, OP = 9, ARG = 12 };

void *P(uintptr_t a) { return (void *) a; }
void *const A = P(0x100000), *const B = P(0x200000), *const C = P(0x300000),
            *const D = P(0x400000), *const WILD = P(~(uintptr_t) 0);

// all four forms of the accumulate give one class (fetch: the fetch forms only)
int acc(const void *o, void *t, MPIX_Aint n, MPIX_Datatype dt, MPIX_Op op)
{
    const int rc = MPIX_Accumulate_local_atomic_async(o, t, n, dt, op, nullptr);
    CHECK(MPIX_Redop_last_error() == rc);
    CHECK(MPIX_Accumulate_local_atomic(o, t, n, dt, op) == rc);
    return rc;
}

int getacc(const void *o, void *r, void *t, MPIX_Aint n, MPIX_Datatype dt, MPIX_Op op)
{
    const int rc = MPIX_Get_accumulate_local_atomic_async(o, r, t, n, dt, op, nullptr);
    CHECK(MPIX_Redop_last_error() == rc);
    CHECK(MPIX_Get_accumulate_local_atomic(o, r, t, n, dt, op) == rc);
    return rc;
}

int cas(const void *o, const void *c, void *r, void *t, MPIX_Datatype dt)
{
    const int rc = MPIX_Compare_and_swap_local_atomic_async(o, c, r, t, dt, nullptr);
    CHECK(MPIX_Redop_last_error() == rc);
    CHECK(MPIX_Compare_and_swap_local_atomic(o, c, r, t, dt) == rc);
    return rc;
}

void predicate()
{
    CHECK(MPIX_Accumulate_atomic_is_supported(kSum, kFloat) == 1);
    CHECK(MPIX_Accumulate_atomic_is_supported(kSum, kInt8) == 1);
    CHECK(MPIX_Accumulate_atomic_is_supported(kMaxloc, kFloatInt) == 1);
    CHECK(MPIX_Accumulate_atomic_is_supported(kMaxloc, kShortInt) == 1);
    CHECK(MPIX_Accumulate_atomic_is_supported(kMaxloc, kDoubleInt) == 0);
    CHECK(MPIX_Accumulate_atomic_is_supported(kMaxloc, kLongDoubleInt) == 0);
    CHECK(MPIX_Accumulate_atomic_is_supported(kMaxloc, kFloat) == 0);
    CHECK(MPIX_Accumulate_atomic_is_supported(kBand, kFloat) == 0);
    CHECK(MPIX_Accumulate_atomic_is_supported(kReplace, kShortInt) == 1);
    CHECK(MPIX_Accumulate_atomic_is_supported(kNoOp, kDoubleInt) == 0);
    CHECK(MPIX_Accumulate_atomic_is_supported(kEqual, kByte) == 0);
    CHECK(MPIX_Accumulate_atomic_is_supported(kSum, kUnknown) == 0);
    CHECK(MPIX_Accumulate_atomic_is_supported(kNullOp, kInt64) == 1);
    CHECK(MPIX_Accumulate_atomic_is_supported(kNullOp, kFloat) == 0);
    CHECK(MPIX_Accumulate_atomic_is_supported(kNullOp, 0x4c811000) == 0);    // MPIR_INT128
    CHECK(MPIX_Accumulate_atomic_is_supported(0, 0) == 0);
    CHECK(MPIX_Accumulate_atomic_is_supported((MPIX_Op) 0xffffffff, (MPIX_Datatype) 0xffffffff) == 0);
    // every bit pattern of the low op and type bytes stays inside the tables
    for (unsigned op = 0; op < 16; ++op)
        for (unsigned t = 0; t < 256; ++t) {
            const int r = MPIX_Accumulate_atomic_is_supported((MPIX_Op) (0x58000000u | op),
                                                              (MPIX_Datatype) (0x4c000000u | t));
            CHECK(r == 0 || r == 1);
            for (unsigned sz = 0; sz < 0x40; sz += 1)
                (void) MPIX_Accumulate_atomic_is_supported(
                    (MPIX_Op) (0x58000000u | op), (MPIX_Datatype) (0x4c800000u | (t << 16) | (sz << 8)));
        }
}

void order_of_checks()
{
    // count < 0 before everything
    CHECK(acc(nullptr, nullptr, -1, kUnknown, kEqual) == COUNT);
    CHECK(getacc(nullptr, nullptr, nullptr, -1, kUnknown, kEqual) == COUNT);
    // MPIX_EQUAL before the type, count 0 included
    CHECK(acc(A, B, 0, kUnknown, kEqual) == OP);
    CHECK(getacc(A, B, C, 8, kByte, kEqual) == OP);
    // a non-builtin op, an unknown type, an illegal pair
    CHECK(acc(A, B, 4, kFloat, kNullOp) == OP);
    CHECK(acc(A, B, 4, kUnknown, kSum) == TYPE);
    CHECK(getacc(A, B, C, 4, kFloat, kBand) == OP);
    CHECK(getacc(A, B, C, 4, kFloat, kMaxloc) == OP);
    // count 0 looks at no pointer
    CHECK(acc(WILD, nullptr, 0, kFloat, kSum) == OK);
    CHECK(getacc(nullptr, WILD, nullptr, 0, kDoubleInt, kMaxloc) == OK);
    // the cap before the pointers
    CHECK(acc(nullptr, nullptr, ((MPIX_Aint) 1 << 54) + 1, kFloat, kSum) == COUNT);
    CHECK(getacc(nullptr, nullptr, nullptr, ((MPIX_Aint) 1 << 53) + 1, kDouble, kSum) == COUNT);
    // NULL / MPI_IN_PLACE before the declined pair
    CHECK(acc(nullptr, B, 4, kDoubleInt, kMaxloc) == BUFFER);
    CHECK(acc(A, WILD, 4, kDoubleInt, kMaxloc) == BUFFER);
    CHECK(getacc(A, nullptr, C, 4, kDoubleInt, kMaxloc) == BUFFER);
    CHECK(getacc(nullptr, B, C, 4, kFloat, kReplace) == BUFFER);
    // overlap before the declined pair
    CHECK(acc(A, (char *) A + 60, 4, kDoubleInt, kMaxloc) == BUFFER);
    CHECK(getacc(A, B, (char *) B + 15, 4, kFloat, kSum) == BUFFER);
    CHECK(getacc(A, (char *) A + 15, C, 4, kFloat, kSum) == BUFFER);
    CHECK(getacc(B, B, (char *) B + 15, 4, kFloat, kNoOp) == BUFFER);
    // a declined pair: MPI_ERR_TYPE
    CHECK(acc(A, B, 4, kDoubleInt, kMaxloc) == TYPE);
    CHECK(getacc(A, B, C, 4, kLongDoubleInt, kMaxloc) == TYPE);
    CHECK(getacc(A, B, C, 4, 0x4c811000, kSum) == TYPE);
    CHECK(getacc(nullptr, B, C, 4, kDoubleInt, kNoOp) == TYPE);
    CHECK(acc(A, B, 4, kDoubleInt, kReplace) == TYPE);
    CHECK(acc(A, B, 4, 0x4c850200, kMax) == TYPE);      // bf16 MAX: no kernel
    // before the alignment
    CHECK(acc(A, (char *) B + 4, 4, kDoubleInt, kMaxloc) == TYPE);
    // a misaligned target
    CHECK(acc(A, (char *) B + 2, 4, kFloat, kSum) == BUFFER);
    CHECK(getacc(A, B, (char *) C + 4, 4, kDouble, kSum) == BUFFER);
    CHECK(getacc(A, B, (char *) C + 4, 4, kFloatInt, kMaxloc) == BUFFER);
    CHECK(acc(A, (char *) B + 1, 4, kInt16, kSum) == BUFFER);
    // an aligned one reaches the placement check; there is no device here
    CHECK(acc((char *) A + 1, (char *) B + 3, 4, kInt8, kSum) == BUFFER);
    CHECK(getacc(nullptr, B, C, 4, kFloat, kNoOp) == BUFFER);
    CHECK(acc(A, (char *) B + 4, 4, kInt32, kSum) == BUFFER);
}

void compare_and_swap()
{
    CHECK(cas(nullptr, nullptr, nullptr, nullptr, kFloat) == TYPE);
    CHECK(cas(nullptr, nullptr, nullptr, nullptr, kUnknown) == TYPE);
    CHECK(cas(nullptr, B, C, D, kInt32) == BUFFER);
    CHECK(cas(A, B, C, WILD, kInt32) == BUFFER);
    CHECK(cas(A, B, A, D, kInt32) == BUFFER);                   // result over origin
    CHECK(cas(A, B, C, (char *) C + 3, kInt32) == BUFFER);
    // NULLs and overlaps before the declined 16-byte type
    CHECK(cas(nullptr, B, C, D, 0x4c811000) == BUFFER);
    CHECK(cas(A, B, C, (char *) C + 15, 0x4c811000) == BUFFER);
    CHECK(cas(A, B, C, D, 0x4c811000) == TYPE);
    CHECK(cas(A, B, C, (char *) D + 8, 0x4c821000) == TYPE);
    // alignment of the target alone
    CHECK(cas((char *) A + 1, (char *) B + 3, (char *) C + 5, (char *) D + 2, kInt32) == BUFFER);
    CHECK(cas(A, B, C, (char *) D + 4, kInt64) == BUFFER);
    CHECK(cas(A, B, C, (char *) D + 1, kInt16) == BUFFER);
    CHECK(cas(A, A, C, (char *) D + 3, kInt8) == BUFFER);       // placement: no device here
}

}  // namespace

int main()
{
    predicate();
    order_of_checks();
    compare_and_swap();
    printf("acc_atomic_host_check: %d errors\n", g_errors);
    return g_errors ? 1 : 0;
}
