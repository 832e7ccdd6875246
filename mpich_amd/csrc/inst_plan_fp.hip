// inst_plan_fp.hip -- the committed-plan kernels (reduce and fetch form) of the
// floating-point and complex combiners: inst_fp.hip's (type, op) table over plan_entry.
#include "redop_kernels.h"

namespace mpix {

namespace {

template <class Max, class Min, class Sum, class Prod>
const PlanEntry *four_ops(int opi)
{
    static const PlanEntry tab[4] = { plan_entry<Max>(), plan_entry<Min>(), plan_entry<Sum>(),
                                      plan_entry<Prod>() };
    return (opi >= 1 && opi <= 4) ? &tab[opi - 1] : nullptr;
}

template <typename T>
const PlanEntry *real_ops(int opi)
{
    return four_ops<FMax<T>, FMin<T>, FSum<T>, FProd<T>>(opi);
}

template <class Sum, class Prod>
const PlanEntry *cplx_ops(int opi)
{
    static const PlanEntry tab[2] = { plan_entry<Sum>(), plan_entry<Prod>() };
    return (opi == 3 || opi == 4) ? &tab[opi - 3] : nullptr;
}

const PlanEntry *bf16_ops(int opi)
{
    static const PlanEntry e = plan_entry<Bf16Sum>();
    return opi == 3 ? &e : nullptr;     // only MPIR_SUM handles MPIR_BFLOAT16
}

}  // namespace

const PlanEntry *lookup_plan_fp(int raw, int opi)
{
    switch ((unsigned) raw) {
        case 0x4c830200u: return real_ops<_Float16>(opi);
        case 0x4c830400u: return real_ops<float>(opi);
        case 0x4c830800u: return real_ops<double>(opi);
        case 0x4c840400u: return cplx_ops<CSum<_Float16>, CProdHalf>(opi);
        case 0x4c840800u: return cplx_ops<CSum<float>, CProdAnnexG<float>>(opi);
        case 0x4c841000u: return cplx_ops<CSum<double>, CProdAnnexG<double>>(opi);
        case 0x4c850200u: return bf16_ops(opi);
        case 0x4c851000u: return four_ops<X87Max, X87Min, X87Sum, X87Prod>(opi);
        case 0x4c831000u: return four_ops<QuadMax, QuadMin, QuadSum, QuadProd>(opi);
        case 0x4c842000u: return cplx_ops<QuadCSum, QuadCProd>(opi);
        case 0x4c862000u: return cplx_ops<X87CSum, X87CProd>(opi);
        default: return nullptr;
    }
}

}  // namespace mpix
