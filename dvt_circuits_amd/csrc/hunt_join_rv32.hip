// The join hunt (hunt_join.cuh) over the RV32IM core machine's chips up to sha_compress, in a unit of its own; program,
// byte and mem_image may serve as supply tables.
#include "hunt_join.cuh"
#include "gen/air_rv32.inc"
#include "gen/rv32_cols.h"

namespace dvt {
namespace {
template <int I, class A>
bool pick(int chip, ChipDesc *d) {
    if constexpr (I < RV32_FIRST_WIDE_CHIP) {
        if (chip == I) {
            *d = with_join_fn<A>(*d);
            if constexpr (I == RV32_CHIP_PROGRAM || I == RV32_CHIP_BYTE || I == RV32_CHIP_MEM_IMAGE) *d = with_supply_fn<A>(*d);
            return true;
        }
    }
    return false;
}
}  // namespace
void rv32_join_fns(int chip, ChipDesc *d) {
#define DVT_X(i, A) if (pick<i, A>(chip, d)) return;
    DVT_AIR_RV32_CHIPS(DVT_X)
#undef DVT_X
}
}  // namespace dvt
