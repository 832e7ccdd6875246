// inst_plan_pair.hip -- the committed-plan kernels (reduce and fetch form) of MAXLOC /
// MINLOC: inst_pair.hip's (type, op) table over plan_entry.
#include "redop_kernels.h"

namespace mpix {

namespace {

template <class Min, class Max>
const PlanEntry *loc_pair(int opi)
{
    static const PlanEntry tab[2] = { plan_entry<Min>(), plan_entry<Max>() };
    return (opi == 11 || opi == 12) ? &tab[opi - 11] : nullptr;     // MINLOC, MAXLOC
}

template <typename P>
const PlanEntry *loc_ops(int opi)
{
    return loc_pair<Loc<P, false>, Loc<P, true>>(opi);
}

}  // namespace

const PlanEntry *lookup_plan_pair(int raw, int opi)
{
    switch ((unsigned) raw) {
        case 0x4cc10200u: return loc_ops<BPair<int8_t, int8_t>>(opi);
        case 0x4cc10400u: return loc_ops<BPair<int16_t, int16_t>>(opi);
        case 0x4cc10800u: return loc_ops<BPair<int32_t, int32_t>>(opi);
        case 0x4cc11000u: return loc_ops<BPair<int64_t, int64_t>>(opi);
        case 0x4cc20200u: return loc_ops<BPair<uint8_t, uint8_t>>(opi);
        case 0x4cc20400u: return loc_ops<BPair<uint16_t, uint16_t>>(opi);
        case 0x4cc20800u: return loc_ops<BPair<uint32_t, uint32_t>>(opi);
        case 0x4cc21000u: return loc_ops<BPair<uint64_t, uint64_t>>(opi);
        case 0x4cc30400u: return loc_ops<BPair<_Float16, _Float16>>(opi);
        case 0x4cc30800u: return loc_ops<BPair<float, float>>(opi);
        case 0x4cc31000u: return loc_ops<BPair<double, double>>(opi);
        case 0x8c000000u: return loc_ops<FloatInt>(opi);
        case 0x8c000001u: return loc_ops<DoubleIntBody>(opi);
        case 0x8c000002u: return loc_ops<LongIntBody>(opi);
        case 0x8c000003u: return loc_ops<ShortInt>(opi);
        case 0x8c000004u: return loc_pair<LocX87<false>, LocX87<true>>(opi);   // MPI_LONG_DOUBLE_INT
        case 0x4cc32000u: return loc_pair<LocQuad<false>, LocQuad<true>>(opi); // MPIR_2FLOAT128
        default: return nullptr;
    }
}

}  // namespace mpix
