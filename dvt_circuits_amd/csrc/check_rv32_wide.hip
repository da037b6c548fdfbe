// The trace-row checks (check.cuh) of the field / curve precompile chips of the RV32IM core machine (fp_op, fp2_op, bls_g1,
// secp_k1, u256_mul): see check_rv32.hip.
#include "machine.h"
#include "gen/air_rv32.inc"

namespace dvt {
namespace {
template <int I, class A>
bool pick(int chip, ChipDesc *d) {
    if constexpr (I >= RV32_FIRST_WIDE_CHIP) {
        if (chip == I) { *d = with_check_fns<A>(*d); return true; }
    }
    return false;
}
}  // namespace
void rv32_wide_check_fns(int chip, ChipDesc *d) {
#define DVT_X(i, A) if (pick<i, A>(chip, d)) return;
    DVT_AIR_RV32_CHIPS(DVT_X)
#undef DVT_X
}
}  // namespace dvt
