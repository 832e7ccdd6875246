// inst_plan_int.hip -- the committed-plan kernels (reduce and fetch form) of the integer
// and Fortran-logical combiners: inst_int.hip's (type, op) table over plan_entry.
#include "redop_kernels.h"

namespace mpix {

namespace {

template <typename S, typename U>
const PlanEntry *int_ops(int opi)
{
    // as inst_int.hip: only MAX / MIN depend on signedness
    static const PlanEntry tab[11] = {
        PlanEntry{nullptr, nullptr},
        plan_entry<IMax<S>>(), plan_entry<IMin<S>>(), plan_entry<ISum<U>>(),
        plan_entry<IProd<U>>(), plan_entry<ILand<U>>(), plan_entry<IBand<U>>(),
        plan_entry<ILor<U>>(), plan_entry<IBor<U>>(), plan_entry<ILxor<U>>(),
        plan_entry<IBxor<U>>(),
    };
    return (opi >= 1 && opi <= 10) ? &tab[opi] : nullptr;
}

template <typename U>
const PlanEntry *uint_minmax(int opi)
{
    static const PlanEntry tab[2] = { plan_entry<IMax<U>>(), plan_entry<IMin<U>>() };
    return (opi == 1 || opi == 2) ? &tab[opi - 1] : nullptr;
}

template <typename S>
const PlanEntry *flog_ops(int opi)
{
    static const PlanEntry tab[3] = { plan_entry<FLand<S>>(), plan_entry<FLor<S>>(),
                                      plan_entry<FLxor<S>>() };
    switch (opi) {
        case 5: return &tab[0];
        case 7: return &tab[1];
        case 9: return &tab[2];
        default: return nullptr;
    }
}

}  // namespace

const PlanEntry *lookup_plan_int(int raw, int opi)
{
    switch ((unsigned) raw) {
        case 0x4c810100u: return int_ops<int8_t, uint8_t>(opi);
        case 0x4c810200u: return int_ops<int16_t, uint16_t>(opi);
        case 0x4c810400u: return int_ops<int32_t, uint32_t>(opi);
        case 0x4c810800u: return int_ops<int64_t, uint64_t>(opi);
        case 0x4c811000u: return int_ops<__int128, unsigned __int128>(opi);
        case 0x4c820100u: return (opi <= 2) ? uint_minmax<uint8_t>(opi) : int_ops<int8_t, uint8_t>(opi);
        case 0x4c820200u: return (opi <= 2) ? uint_minmax<uint16_t>(opi) : int_ops<int16_t, uint16_t>(opi);
        case 0x4c820400u: return (opi <= 2) ? uint_minmax<uint32_t>(opi) : int_ops<int32_t, uint32_t>(opi);
        case 0x4c820800u: return (opi <= 2) ? uint_minmax<uint64_t>(opi) : int_ops<int64_t, uint64_t>(opi);
        case 0x4c821000u:
            return (opi <= 2) ? uint_minmax<unsigned __int128>(opi)
                              : int_ops<__int128, unsigned __int128>(opi);
        case 0x4c870100u: return flog_ops<int8_t>(opi);
        case 0x4c870200u: return flog_ops<int16_t>(opi);
        case 0x4c870400u: return flog_ops<int32_t>(opi);
        case 0x4c870800u: return flog_ops<int64_t>(opi);
        case 0x4c871000u: return flog_ops<__int128>(opi);
        default: return nullptr;
    }
}

}  // namespace mpix
