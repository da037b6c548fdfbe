// The one key function of the bus ledger (ledger.cuh), shared by the kernels and the host: the host keys the tuples it adds
// itself (the verifier's side of the COMMIT tuples) with the function the rows are keyed with.
#pragma once
#include <cstdint>

#include "bb.cuh"

namespace dvt {

// a bijection of the 64-bit words (the finaliser of splitmix64)
DVT_HD uint64_t ledger_mix(uint64_t x) {
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}
// key(seed, bus, arity, canonical values).  Every step is a bijection of the running word after a XOR with one input, so the
// key depends on the seed, the bus, the arity and every value.
// (in steps, for a caller that has the values one at a time: ledger_key_begin, then ledger_key_value for each canonical value)
DVT_HD uint64_t ledger_key_begin(uint64_t seed, uint32_t bus, uint32_t arity) {
    return ledger_mix(ledger_mix(seed ^ 0x6a09e667f3bcc908ull) ^ (((uint64_t)bus << 32) | arity));
}
DVT_HD uint64_t ledger_key_value(uint64_t h, uint32_t canonical) { return ledger_mix(h ^ canonical); }
DVT_HD uint64_t ledger_key(uint64_t seed, uint32_t bus, uint32_t arity, const uint32_t *values) {
    uint64_t h = ledger_key_begin(seed, bus, arity);
    for (uint32_t k = 0; k < arity; k++) h = ledger_key_value(h, values[k]);
    return h;
}
// the two weights of a key, in [1, p)
DVT_HD uint32_t ledger_weight(uint64_t key, int which) {
    const uint64_t x = ledger_mix(key ^ (which ? 0xbb67ae8584caa73bull : 0x3c6ef372fe94f82bull)) >> 33;   // 31 bits
    return 1u + (uint32_t)((x * (uint64_t)(P - 1)) >> 31);
}
DVT_HD uint32_t ledger_bucket(uint64_t key, uint32_t log_buckets) { return (uint32_t)(key >> (64 - log_buckets)); }
DVT_HD uint32_t ledger_start_slot(uint64_t key, uint32_t cap_slots) { return (uint32_t)(ledger_mix(key ^ 0xa54ff53a5f1d36f1ull) >> 32) % cap_slots; }

// where a tuple occurred, packed so that the numeric minimum is the lowest (tag, chip, row, interaction)
constexpr uint32_t LEDGER_HOST_CHIP = 63;   // the chip field of a tuple the host added (reported as 0xffffffff)
DVT_HD uint64_t ledger_occurrence(uint32_t tag, uint32_t chip, uint32_t row, uint32_t interaction) {
    return ((uint64_t)(tag & 0xffffu) << 38) | ((uint64_t)(chip & 63u) << 32) | ((uint64_t)(row & 0x3fffffu) << 10) | (interaction & 0x3ffu);
}

}  // namespace dvt
