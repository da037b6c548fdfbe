// Instantiates the generic STARK kernels for the toy machine (engine unit tests).
#include "machine.h"
#include "gen/air_toy.inc"

namespace dvt {
void toy_ledger_fns(int chip, ChipDesc *d);   // ledger_toy.hip
void toy_hunt_fns(int chip, ChipDesc *d);     // hunt_toy.hip
void toy_join_fns(int chip, ChipDesc *d);     // hunt_join_toy.hip
namespace {
template <int I, class A>
ChipDesc chip_desc_here() {
    ChipDesc d = with_check_fns<A>(make_chip_desc<A>());
    toy_ledger_fns(I, &d);
    toy_hunt_fns(I, &d);
    toy_join_fns(I, &d);
    return d;
}
}  // namespace
#define DVT_X(i, A) chip_desc_here<i, A>(),
static const ChipDesc toy_chips[] = {DVT_AIR_TOY_CHIPS(DVT_X)};
#undef DVT_X
static const MachineDesc toy_machine = {"toy", air_toy::N_CHIPS, toy_chips};
const MachineDesc *machine_toy() { return &toy_machine; }
}  // namespace dvt
