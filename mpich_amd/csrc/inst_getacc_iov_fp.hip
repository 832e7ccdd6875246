// inst_getacc_iov_fp.hip -- the iov-target get-accumulate kernels of the floating-point
// and complex combiners: inst_fp.hip's (type, op) table over getacc_iov_entry.
#include "redop_kernels.h"

namespace mpix {

namespace {

template <class Max, class Min, class Sum, class Prod>
const GetaccIovEntry *four_ops(int opi)
{
    static const GetaccIovEntry tab[4] = { getacc_iov_entry<Max>(), getacc_iov_entry<Min>(),
                                        getacc_iov_entry<Sum>(), getacc_iov_entry<Prod>() };
    return (opi >= 1 && opi <= 4) ? &tab[opi - 1] : nullptr;
}

template <typename T>
const GetaccIovEntry *real_ops(int opi)
{
    return four_ops<FMax<T>, FMin<T>, FSum<T>, FProd<T>>(opi);
}

template <class Sum, class Prod>
const GetaccIovEntry *cplx_ops(int opi)
{
    static const GetaccIovEntry tab[2] = { getacc_iov_entry<Sum>(), getacc_iov_entry<Prod>() };
    return (opi == 3 || opi == 4) ? &tab[opi - 3] : nullptr;
}

const GetaccIovEntry *bf16_ops(int opi)
{
    static const GetaccIovEntry e = getacc_iov_entry<Bf16Sum>();
    return opi == 3 ? &e : nullptr;     // only MPIR_SUM handles MPIR_BFLOAT16
}

}  // namespace

const GetaccIovEntry *lookup_getacc_iov_fp(int raw, int opi)
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
