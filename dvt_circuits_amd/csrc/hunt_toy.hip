// The forgery hunt (hunt.cuh) over the toy machine's chips.
#include "hunt.cuh"
#include "gen/air_toy.inc"

namespace dvt {
void toy_hunt_fns(int chip, ChipDesc *d) {
#define DVT_X(i, A) if (chip == i) { *d = with_hunt_fn<A>(*d); return; }
    DVT_AIR_TOY_CHIPS(DVT_X)
#undef DVT_X
}
}  // namespace dvt
