// The trace-row checks (check.cuh) of the RV32IM core machine's chips up to sha_compress, instantiated apart from the STARK
// kernels of machine_rv32.hip so that the units compile side by side.  Device code only: the host verifier's F_p^4
// instantiation of the generated AIR is not needed here.
#include "machine.h"
#include "gen/air_rv32.inc"

namespace dvt {
namespace {
template <int I, class A>
bool pick(int chip, ChipDesc *d) {
    if constexpr (I < RV32_FIRST_WIDE_CHIP) {
        if (chip == I) { *d = with_check_fns<A>(*d); return true; }
    }
    return false;
}
}  // namespace
void rv32_check_fns(int chip, ChipDesc *d) {
#define DVT_X(i, A) if (pick<i, A>(chip, d)) return;
    DVT_AIR_RV32_CHIPS(DVT_X)
#undef DVT_X
}
}  // namespace dvt
