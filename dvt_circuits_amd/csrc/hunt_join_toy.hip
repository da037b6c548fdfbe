// The join hunt (hunt_join.cuh) over the toy machine's chips; range8 may serve as a supply table.
#include "hunt_join.cuh"
#include "gen/air_toy.inc"

namespace dvt {
void toy_join_fns(int chip, ChipDesc *d) {
#define DVT_X(i, A) if (chip == i) { *d = with_join_fn<A>(*d); }
    DVT_AIR_TOY_CHIPS(DVT_X)
#undef DVT_X
    if (chip == 0) *d = with_supply_fn<air_toy::Range8>(*d);
}
}  // namespace dvt
