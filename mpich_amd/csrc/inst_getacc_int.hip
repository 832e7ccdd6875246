// inst_getacc_int.hip -- the fused get-accumulate kernels of the integer and
// Fortran-logical combiners: inst_int.hip's (type, op) table over getacc_entry.
#include "redop_kernels.h"

namespace mpix {

namespace {

template <typename S, typename U>
const GetaccEntry *int_ops(int opi)
{
    // as inst_int.hip: only MAX / MIN depend on signedness
    static const GetaccEntry tab[11] = {
        GetaccEntry{nullptr, nullptr},
        getacc_entry<IMax<S>>(), getacc_entry<IMin<S>>(), getacc_entry<ISum<U>>(),
        getacc_entry<IProd<U>>(), getacc_entry<ILand<U>>(), getacc_entry<IBand<U>>(),
        getacc_entry<ILor<U>>(), getacc_entry<IBor<U>>(), getacc_entry<ILxor<U>>(),
        getacc_entry<IBxor<U>>(),
    };
    return (opi >= 1 && opi <= 10) ? &tab[opi] : nullptr;
}

template <typename U>
const GetaccEntry *uint_minmax(int opi)
{
    static const GetaccEntry tab[2] = { getacc_entry<IMax<U>>(), getacc_entry<IMin<U>>() };
    return (opi == 1 || opi == 2) ? &tab[opi - 1] : nullptr;
}

template <typename S>
const GetaccEntry *flog_ops(int opi)
{
    static const GetaccEntry tab[3] = { getacc_entry<FLand<S>>(), getacc_entry<FLor<S>>(),
                                        getacc_entry<FLxor<S>>() };
    switch (opi) {
        case 5: return &tab[0];
        case 7: return &tab[1];
        case 9: return &tab[2];
        default: return nullptr;
    }
}

}  // namespace

const GetaccEntry *lookup_getacc_int(int raw, int opi)
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
