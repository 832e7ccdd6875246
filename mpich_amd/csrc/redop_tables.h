// redop_tables.h -- the (raw internal type, op index) -> combiner maps, once.
//
// Every kernel family (the reduction's Entry, the fused get-accumulate's
// GetaccEntry, its iov form's GetaccIovEntry, the committed plans' PlanEntry,
// the typed entries' TypedEntry, the element-atomic accumulate's AtomicEntry of
// redop_atomic.h)
// builds its three tables from these maps, in its own instantiation units
// (inst_[<family>_]{int,fp,pair}.hip): E is the family's entry type and
// Make<C>::get() its entry for combiner C (redop_kernels.h).  So a pair has an
// entry in one family exactly when it has one in every other; a new type or op
// is one line here.
//
// Op indices (handle & 0xf): 1 MAX, 2 MIN, 3 SUM, 4 PROD, 5 LAND, 6 BAND,
// 7 LOR, 8 BOR, 9 LXOR, 10 BXOR, 11 MINLOC, 12 MAXLOC.
#pragma once

#include "redop_kernels.h"

namespace mpix {

// entry i of the combiners Cs, in that order; nullptr outside them
template <class E, template <class> class Make, class... Cs>
const E *entry_at(int i)
{
    static const E tab[] = { Make<Cs>::get()... };
    return (i >= 0 && i < (int) sizeof...(Cs)) ? &tab[i] : nullptr;
}

// ---- integers and Fortran logicals
// (MPIR_OP_TYPE_GROUP(INTEGER) / (FORTRAN_LOGICAL), src/include/mpir_op_util.h:195-244)

// SUM/PROD/bitwise/logical are sign-agnostic bit patterns: share the unsigned
// instantiation; only MAX/MIN depend on signedness (M: S or U).
template <class E, template <class> class Make, typename M, typename U>
const E *int_ops(int opi)
{
    return entry_at<E, Make, IMax<M>, IMin<M>, ISum<U>, IProd<U>, ILand<U>, IBand<U>, ILor<U>,
                    IBor<U>, ILxor<U>, IBxor<U>>(opi - 1);
}

template <class E, template <class> class Make, typename S>
const E *flog_ops(int opi)
{
    if (opi != 5 && opi != 7 && opi != 9)
        return nullptr;
    return entry_at<E, Make, FLand<S>, FLor<S>, FLxor<S>>((opi - 5) / 2);
}

template <class E, template <class> class Make>
const E *table_int(int raw, int opi)
{
    switch ((unsigned) raw) {
        case 0x4c810100u: return int_ops<E, Make, int8_t, uint8_t>(opi);
        case 0x4c810200u: return int_ops<E, Make, int16_t, uint16_t>(opi);
        case 0x4c810400u: return int_ops<E, Make, int32_t, uint32_t>(opi);
        case 0x4c810800u: return int_ops<E, Make, int64_t, uint64_t>(opi);
        case 0x4c811000u: return int_ops<E, Make, __int128, unsigned __int128>(opi);
        case 0x4c820100u: return int_ops<E, Make, uint8_t, uint8_t>(opi);
        case 0x4c820200u: return int_ops<E, Make, uint16_t, uint16_t>(opi);
        case 0x4c820400u: return int_ops<E, Make, uint32_t, uint32_t>(opi);
        case 0x4c820800u: return int_ops<E, Make, uint64_t, uint64_t>(opi);
        case 0x4c821000u: return int_ops<E, Make, unsigned __int128, unsigned __int128>(opi);
        case 0x4c870100u: return flog_ops<E, Make, int8_t>(opi);
        case 0x4c870200u: return flog_ops<E, Make, int16_t>(opi);
        case 0x4c870400u: return flog_ops<E, Make, int32_t>(opi);
        case 0x4c870800u: return flog_ops<E, Make, int64_t>(opi);
        case 0x4c871000u: return flog_ops<E, Make, __int128>(opi);
        default: return nullptr;
    }
}

// ---- floating point and complex
// (MPIR_OP_TYPE_GROUP(FLOATING_POINT) / (C_COMPLEX) / (COMPLEX) and the bf16
// SUM helper, src/include/mpir_op_util.h:211-236, op_fns.c:19-91,459-493)

template <class E, template <class> class Make, class Max, class Min, class Sum, class Prod>
const E *four_ops(int opi)
{
    return entry_at<E, Make, Max, Min, Sum, Prod>(opi - 1);
}

template <class E, template <class> class Make, typename T>
const E *real_ops(int opi)
{
    return four_ops<E, Make, FMax<T>, FMin<T>, FSum<T>, FProd<T>>(opi);
}

template <class E, template <class> class Make, class Sum, class Prod>
const E *cplx_ops(int opi)
{
    return entry_at<E, Make, Sum, Prod>(opi - 3);
}

template <class E, template <class> class Make>
const E *table_fp(int raw, int opi)
{
    switch ((unsigned) raw) {
        case 0x4c830200u: return real_ops<E, Make, _Float16>(opi);
        case 0x4c830400u: return real_ops<E, Make, float>(opi);
        case 0x4c830800u: return real_ops<E, Make, double>(opi);
        case 0x4c840400u: return cplx_ops<E, Make, CSum<_Float16>, CProdHalf>(opi);
        case 0x4c840800u: return cplx_ops<E, Make, CSum<float>, CProdAnnexG<float>>(opi);
        case 0x4c841000u: return cplx_ops<E, Make, CSum<double>, CProdAnnexG<double>>(opi);
        // only MPIR_SUM handles MPIR_BFLOAT16
        case 0x4c850200u: return entry_at<E, Make, Bf16Sum>(opi - 3);
        // MPI_LONG_DOUBLE (x87 in 16 bytes) and MPI_REAL16 (binary128): MAX / MIN
        // compare and select in integer arithmetic (redop_ops.h), SUM / PROD in
        // software extended / quad arithmetic (redop_soft.h)
        case 0x4c851000u: return four_ops<E, Make, X87Max, X87Min, X87Sum, X87Prod>(opi);
        case 0x4c831000u: return four_ops<E, Make, QuadMax, QuadMin, QuadSum, QuadProd>(opi);
        // their complex forms: binary128 struct complex, x87 C complex
        case 0x4c842000u: return cplx_ops<E, Make, QuadCSum, QuadCProd>(opi);
        case 0x4c862000u: return cplx_ops<E, Make, X87CSum, X87CProd>(opi);
        default: return nullptr;
    }
}

// ---- MAXLOC / MINLOC over builtin pairs {T v; T loc}
// (MPIR_2INT8.. MPIR_2FLOAT64, op_fns.c:303-330), the struct pair types
// MPI_{FLOAT,DOUBLE,LONG,SHORT,LONG_DOUBLE}_INT {T v; int loc} (op_fns.c:337-352,
// pairtypes.c:15-121), and MPIR_2FLOAT128

template <class E, template <class> class Make, class Min, class Max>
const E *loc_pair(int opi)
{
    return entry_at<E, Make, Min, Max>(opi - 11);
}

template <class E, template <class> class Make, typename P>
const E *loc_ops(int opi)
{
    return loc_pair<E, Make, Loc<P, false>, Loc<P, true>>(opi);
}

template <class E, template <class> class Make>
const E *table_pair(int raw, int opi)
{
    switch ((unsigned) raw) {
        case 0x4cc10200u: return loc_ops<E, Make, BPair<int8_t, int8_t>>(opi);
        case 0x4cc10400u: return loc_ops<E, Make, BPair<int16_t, int16_t>>(opi);
        case 0x4cc10800u: return loc_ops<E, Make, BPair<int32_t, int32_t>>(opi);
        case 0x4cc11000u: return loc_ops<E, Make, BPair<int64_t, int64_t>>(opi);
        case 0x4cc20200u: return loc_ops<E, Make, BPair<uint8_t, uint8_t>>(opi);
        case 0x4cc20400u: return loc_ops<E, Make, BPair<uint16_t, uint16_t>>(opi);
        case 0x4cc20800u: return loc_ops<E, Make, BPair<uint32_t, uint32_t>>(opi);
        case 0x4cc21000u: return loc_ops<E, Make, BPair<uint64_t, uint64_t>>(opi);
        case 0x4cc30400u: return loc_ops<E, Make, BPair<_Float16, _Float16>>(opi);
        case 0x4cc30800u: return loc_ops<E, Make, BPair<float, float>>(opi);
        case 0x4cc31000u: return loc_ops<E, Make, BPair<double, double>>(opi);
        case 0x8c000000u: return loc_ops<E, Make, FloatInt>(opi);
        case 0x8c000001u: return loc_ops<E, Make, DoubleIntBody>(opi);
        case 0x8c000002u: return loc_ops<E, Make, LongIntBody>(opi);
        case 0x8c000003u: return loc_ops<E, Make, ShortInt>(opi);
        // the long double / binary128 pairs: their own comparisons (redop_ops.h)
        case 0x8c000004u: return loc_pair<E, Make, LocX87<false>, LocX87<true>>(opi);   // MPI_LONG_DOUBLE_INT
        case 0x4cc32000u: return loc_pair<E, Make, LocQuad<false>, LocQuad<true>>(opi); // MPIR_2FLOAT128
        default: return nullptr;
    }
}

}  // namespace mpix
