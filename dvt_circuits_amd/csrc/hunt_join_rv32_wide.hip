// The join hunt (hunt_join.cuh) over the field / curve precompile chips of the RV32IM core machine (fp_op onwards).
#include "hunt_join.cuh"
#include "gen/air_rv32.inc"

namespace dvt {
namespace {
template <int I, class A>
bool pick(int chip, ChipDesc *d) {
    if constexpr (I >= RV32_FIRST_WIDE_CHIP) {
        if (chip == I) { *d = with_join_fn<A>(*d); return true; }
    }
    return false;
}
}  // namespace
void rv32_wide_join_fns(int chip, ChipDesc *d) {
#define DVT_X(i, A) if (pick<i, A>(chip, d)) return;
    DVT_AIR_RV32_CHIPS(DVT_X)
#undef DVT_X
}
}  // namespace dvt
