// What a committed shard keeps in HBM between phase 1 and phase 2, and the rule that decides it ("keep_phase1", DESIGN.md
// section 8).  Host only: plain integers in, a tier out, no device state; shard_commit (capi_rv32.hip) asks it under the
// device's turn, dvt_debug_keep_plan exposes it.  The proof bytes do not depend on the tier.
#pragma once
#include <cstdint>

namespace dvt {

// the values of DVT_KEEP_* (include/dvt_prover.h)
constexpr int KEEP_NONE = 0;   // nothing: phase 2 runs K0, the main LDEs and the main commitment again
constexpr int KEEP_TREE = 1;   // the main Merkle tree and its root: phase 2 runs K0 and the main LDEs again, hashes nothing
constexpr int KEEP_FULL = 2;   // K0 output, main LDEs and tree

struct KeepPlanIn {
    int mode = 1;              // "keep_phase1": 0 never, 1 full while it fits (then nothing), 2 full, then trees, then nothing
    uint64_t free_b = 0;       // bytes free on the device, the committing pool's cached bytes included
    uint64_t total_b = 0;      // bytes of the device
    uint64_t reserve = 0;      // what stays free whatever is kept (24 GB + the room of the lanes not yet created)
    uint64_t full_b = 0;       // F: what this shard keeps in full
    uint64_t tree_b = 0;       // T: its tree
    uint64_t later_b = 0;      // L: what every later shard takes at least (its tree and what its upload allocates)
    uint64_t remaining = 0;    // R: shards known to be still to commit on this device in this prepare, after this one
    bool count_known = true;   // the fast pass has finished: R is exact, not a lower bound
    int64_t full_cap = -1;     // "keep_full_max": shards kept in full per device and job at most; negative = no cap
    uint64_t full_kept = 0;    // shards already kept in full on the device in this job
};

// floor(3 x / 4) without overflow
inline uint64_t three_quarters(uint64_t x) { return x / 4 * 3 + x % 4 * 3 / 4; }

inline int keep_plan(const KeepPlanIn &in) {
    if (in.mode <= 0) return KEEP_NONE;
    const bool room = in.free_b > in.reserve;
    if (in.mode == 1) return room ? KEEP_FULL : KEEP_NONE;
    // mode 2.  FULL leaves every later shard room for its uploads and its tree (R L), and while R is only a lower bound
    // it is taken from the first quarter of the device alone.  (Sums that leave 64 bits count as "does not fit".)
    const uint64_t extra = in.full_b > in.tree_b ? in.full_b - in.tree_b : 0;
    uint64_t need = in.reserve, later = 0;
    bool fits = !__builtin_mul_overflow(in.remaining, in.later_b, &later) && !__builtin_add_overflow(need, extra, &need) &&
                !__builtin_add_overflow(need, later, &need) && in.free_b > need;
    if (fits && !in.count_known) fits = in.free_b > three_quarters(in.total_b);
    if (fits && in.full_cap >= 0) fits = in.full_kept < (uint64_t)in.full_cap;
    return fits ? KEEP_FULL : room ? KEEP_TREE : KEEP_NONE;
}

}  // namespace dvt
