// The join hunt: two-cell forgeries across tables and distant rows, and single cells that a lookup table absorbs.  The hunt
// of hunt.cuh stops at the edge of one table and at a distance of one row, and calls a change caught as soon as the
// multiset of its touched rows differs from the honest one.  Here that difference is KEPT: a change that passes every
// constraint of its own table leaves a record with the fingerprint of its difference, and a second pass looks for records
// whose differences cancel.  Same generated AIR source, same view of the trace (JoinRowCtx is HuntRowCtx plus one lookup),
// same fingerprint and key function (ledger_key.h) under ONE key for all tables of a call, same launch shape as
// hunt_kernel in HUNT_CELLS mode.
//
//   SUPPLY   the key of every interaction of every row of a supply table, whatever its multiplicity holds, goes into a hash
//            set: 64-bit keys, 0 = empty (a key of 0 is kept as 1), open addressing, at most JOIN_PROBES probes of one
//            atomicCAS each.  A key that finds no slot raises a flag and the host fails the call: never a silent miss.
//   HONEST   the fingerprints of the honest rows, [6][n]: words 0..2 over all tuples, 3..5 over the tuples whose key is not
//            in the supply set.
//   EMIT     a workgroup holds 256 consecutive base rows of one candidate (col, delta).  Constraint pass as in hunt.cuh;
//            for the survivors D_all and D = forged - honest fingerprints of the touched rows {row - 1, row}, over all and
//            over the unsupplied tuples.  D_all = 0: free, nothing kept.  D_all != 0, D = 0: ABSORBED, a record in the
//            second array.  D != 0: OPEN, a record (D, tag, chip, col, row, delta index) in the first.  One atomicAdd per
//            wave and array: lane k takes the base plus the popcount of the ballot below it and stores only while that
//            index is below the capacity; the totals keep counting.
//   INSERT   one thread per open record.  Canonical form: when the first non-zero word of D is above (p - 1) / 2 the record
//            is on side 1 and keyed by -D, else on side 0 and keyed by D (p is odd and D != 0: no record is its own
//            negative).  The 64-bit mix of the three canonical words claims a slot (at most JOIN_PROBES atomicCAS probes)
//            and the record adds 1 to the slot's counter of its side.  A record that finds no slot sets a flag and is left
//            out.
//   PROBE    one thread per open record again: it finds its slot and, when both counters are non-zero, copies the record
//            to the output (wave-aggregated index, bounded by a capacity, with a total).
// The host groups the matched records by the exact three words (two D that share a 64-bit slot key part there), applies the
// exclusion rule (same table instance at circular row distance <= 1: the touched rows overlap, the differences do not
// add) and sorts.
//
// Every loop has a trip count bounded by the launch (a probe sequence ends early on a hit or a free slot) and no thread waits for another.  Indices: rows are masked by n - 1,
// slots by the table's mask, record and output stores are guarded by their capacity, candidates by gridDim.y.
// Thousands of records with one D (a hot group) all add to ONE slot's counter and serialise there: this is a diagnostic
// and is built plain, as ledger.cuh is.
//
// WHAT IT MISSES is what hunt.cuh's fingerprint misses (differences whose three sums vanish although the multisets differ,
// about 2^-60 over the key; two tuples sharing a 64-bit key, 2^-63 per pair), here also for the membership in the supply
// set, and by construction: forgeries of three or more cells; a pair in which one half is caught by a constraint and
// repaired by the other; permutation and quotient columns.  No soundness claim follows from an empty answer.
#pragma once
#include "hunt.cuh"

namespace dvt {

constexpr uint32_t JOIN_HONEST = 0, JOIN_EMIT = 1;
constexpr uint32_t JOIN_PROBES = 64;
constexpr uint32_t JOIN_FLAG_SUPPLY_FULL = 0, JOIN_FLAG_NO_SLOT = 1;   // words of JoinArgs::flags / JoinTable::flags
constexpr uint32_t JOIN_HALF_P = (P - 1) / 2;

struct JoinRecord {
    uint32_t d[3];       // the fingerprint of D, each word below p
    uint32_t where;      // tag | chip << 16
    uint32_t col, row;
    uint32_t delta;      // index into the call's list
    uint32_t pad;
};
static_assert(sizeof(JoinRecord) == 32, "the host copies these records out");

struct JoinSlot {
    unsigned long long key;   // 0: free
    uint32_t n[2];            // records of side 0 / 1
};
static_assert(sizeof(JoinSlot) == 16, "cleared with a memset");

struct JoinArgs {
    HuntArgs h;   // main, prep, pub, xi_pows, xi_d, log_n, key, row_first, rows, n_deltas, delta_m, cols, n_cols, cand_first
    uint32_t mode;                        // JOIN_HONEST or JOIN_EMIT
    unsigned long long *supply;           // [supply_mask + 1] keys, or nullptr: no supply table
    uint32_t supply_mask;
    uint32_t *honest;                     // [6][n]
    uint32_t where;                       // tag | chip << 16 of the records
    JoinRecord *open, *absorbed;
    uint32_t cap_open, cap_absorbed;
    unsigned long long *counters;         // [0] open emitted, [1] absorbed emitted
    uint32_t *flags;                      // [JOIN_FLAG_SUPPLY_FULL]
};

struct JoinTable {
    const JoinRecord *recs;
    uint32_t n_recs;
    JoinSlot *slots;
    uint32_t slot_mask;
    JoinRecord *out;
    uint32_t cap_out;
    unsigned long long *counters;         // [2] matched
    uint32_t *flags;                      // [JOIN_FLAG_NO_SLOT]
};

// side of a difference and its canonical words (DVT_HD: the host groups by them)
DVT_HD uint32_t join_canonical(const uint32_t d[3], uint32_t out[3]) {
    uint32_t side = 0;
    for (int k = 0; k < 3; k++)
        if (d[k]) { side = d[k] > JOIN_HALF_P; break; }
    for (int k = 0; k < 3; k++) out[k] = side && d[k] ? P - d[k] : d[k];
    return side;
}
DVT_HD uint64_t join_slot_key(const uint32_t c[3]) {
    const uint64_t h = ledger_mix(ledger_mix(ledger_mix(0x9b05688c2b3e6c1full ^ c[0]) ^ c[1]) ^ c[2]);
    return h ? h : 1;
}
DVT_HD uint32_t join_start(uint64_t key) { return (uint32_t)(ledger_mix(key ^ 0xa54ff53a5f1d36f1ull) >> 32); }

#if defined(__HIPCC__)
// ---- the supply set
static __device__ __noinline__ bool join_supply_insert(unsigned long long *set, uint32_t mask, uint64_t key) {
    uint32_t s = join_start(key);
    for (uint32_t i = 0; i < JOIN_PROBES; i++, s++) {
        const unsigned long long old = atomicCAS(set + (s & mask), 0ull, (unsigned long long)key);
        if (old == 0 || old == key) return true;
    }
    return false;
}
// (a key that is in the set lies within JOIN_PROBES slots of its start: the insertion went no further)
static __device__ __noinline__ bool join_supplied(const unsigned long long *set, uint32_t mask, uint64_t key) {
    uint32_t s = join_start(key);
    for (uint32_t i = 0; i < JOIN_PROBES; i++, s++) {
        const unsigned long long k = set[s & mask];
        if (k == key) return true;
        if (k == 0) return false;
    }
    return false;
}
static __device__ __noinline__ uint64_t join_key_of(uint64_t key, uint32_t bus, const Fp *vals, uint32_t nv) {
    uint64_t h = ledger_key_begin(key, bus, nv);
    for (uint32_t k = 0; k < nv; k++) h = ledger_key_value(h, vals[k].canonical());
    return h ? h : 1;
}
struct JoinPrint { uint32_t w[3]; uint32_t supplied; };
// what one interaction adds to the fingerprint of its row (as hunt_print_of), and whether a supply table holds its tuple
static __device__ __noinline__ JoinPrint join_print_of(const JoinArgs &j, uint32_t bus, bool send, Fp mult, const Fp *vals, uint32_t nv) {
    const uint64_t h = join_key_of(j.h.key, bus, vals, nv);
    const uint32_t m = (send ? mult : -mult).canonical();
    return {{m, (uint32_t)((uint64_t)m * ledger_weight(h, 0) % P), (uint32_t)((uint64_t)m * ledger_weight(h, 1) % P)},
            j.supply && join_supplied(j.supply, j.supply_mask, h) ? 1u : 0u};
}

// every interaction of the row, whatever its multiplicity: the tuples a supply table can hold
template <class Air>
struct SupplyRowCtx {
    using T = Fp;
    const JoinArgs &a;
    size_t n, row;
    bool on, full;
    __device__ SupplyRowCtx(const JoinArgs &args) : a(args), n((size_t)1 << args.h.log_n), row(0), on(false), full(false) {}
    __device__ static T K(uint32_t m) { return Fp::raw(m); }
    __device__ static T KI(uint32_t canonical) { return Fp::from_canonical(canonical); }
    __device__ T main(int c, int r) const { return Fp::raw(a.h.main[(size_t)c * n + ((row + r) & (n - 1))]); }
    __device__ T prep(int c, int r) const { return Fp::raw(a.h.prep[(size_t)c * n + ((row + r) & (n - 1))]); }
    __device__ T pub(int k) const { return Fp::raw(a.h.pub[k]); }
    __device__ void constraint(int, int, const T &) {}
    __device__ Fp4 poly(const T *, int) const { return Fp4::zero(); }
    __device__ Fp4 alpha_minus(uint32_t) const { return Fp4::zero(); }
    __device__ void fold_poly(int, const Fp4 &) {}
    __device__ __forceinline__ void interaction(int, int bus, int, int, const T &, const T *vals, int nv) {
        if (!on || bus < 0) return;
        full |= !join_supply_insert(a.supply, a.supply_mask, join_key_of(a.h.key, (uint32_t)bus, vals, (uint32_t)nv));
    }
};
template <class Air>
__global__ void __launch_bounds__(256) join_supply_kernel(JoinArgs a) {
    const size_t n = (size_t)1 << a.h.log_n, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    SupplyRowCtx<Air> ctx(a);
    ctx.row = i & (n - 1);
    ctx.on = i < n;
    if constexpr (Air::N_INTERACTIONS > 0) hunt_interactions_from<Air, 0>(ctx);
    if (ctx.full) a.flags[JOIN_FLAG_SUPPLY_FULL] = 1;
}

// ---- HONEST and EMIT
// HuntRowCtx with a second fingerprint over the tuples that no supply table holds
template <class Air>
struct JoinRowCtx : HuntRowCtx<Air> {
    using T = Fp;
    using Base = HuntRowCtx<Air>;
    const JoinArgs &j;
    uint32_t print_u[3];
    __device__ JoinRowCtx(const JoinArgs &args) : Base(args.h), j(args), print_u{0, 0, 0} {}
    __device__ __forceinline__ void interaction(int, int bus, int sign, int /*scope*/, const T &mult, const T *vals, int nv) {
        if (!this->on || mult.is_zero() || bus < 0) return;
        const JoinPrint f = join_print_of(j, (uint32_t)bus, sign > 0, mult, vals, (uint32_t)nv);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            uint32_t s = this->print[k] + f.w[k];   // both below p < 2^31
            this->print[k] = s >= P ? s - P : s;
            s = print_u[k] + (f.supplied ? 0u : f.w[k]);
            print_u[k] = s >= P ? s - P : s;
        }
    }
};

// the records of the wave's lanes with `want` set: one atomicAdd for the wave, stores below the capacity only
static __device__ __forceinline__ void join_emit(bool want, unsigned long long *total, JoinRecord *out, uint32_t cap, const JoinRecord &r) {
    const unsigned long long m = __ballot(want);
    if (!m) return;   // (wave-uniform)
    const uint32_t lane = threadIdx.x & 63, leader = (uint32_t)__ffsll((long long)m) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(total, (unsigned long long)__popcll(m));
    const uint32_t lo = __shfl((uint32_t)base, (int)leader), hi = __shfl((uint32_t)(base >> 32), (int)leader);
    const unsigned long long at = (((unsigned long long)hi << 32) | lo) + (unsigned long long)__popcll(m & ((1ull << lane) - 1));
    if (want && at < cap) out[at] = r;
}

// grid (row blocks, candidates of the launch; JOIN_HONEST: (row blocks of the table, 1))
template <class Air>
__global__ void __launch_bounds__(256) join_kernel(JoinArgs a) {
    const size_t n = (size_t)1 << a.h.log_n, mask = n - 1;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;   // window index of the base row
    JoinRowCtx<Air> ctx(a);
    if (a.mode == JOIN_HONEST) {
        if constexpr (Air::N_INTERACTIONS > 0) {
            ctx.row = i & mask;
            ctx.on = i < n;
            hunt_interactions_from<Air, 0>(ctx);
        }
        if (i < n)
            for (int k = 0; k < 3; k++) {
                a.honest[(size_t)k * n + i] = ctx.print[k];
                a.honest[(size_t)(3 + k) * n + i] = ctx.print_u[k];
            }
        return;
    }
    // ---- the candidate of this workgroup (scalar)
    const uint32_t cand = a.h.cand_first + blockIdx.y;
    const uint32_t e0 = cand / a.h.n_cols, k0 = cand % a.h.n_cols;
    const size_t base = ((size_t)a.h.row_first + i) & mask;   // (lanes past the window run along on a row of the table)
    const bool live = i < a.h.rows;                           // ... and enter no ballot
    ctx.col0 = a.h.cols[k0];
    ctx.crow0 = base;
    ctx.d0 = Fp::raw(a.h.delta_m[e0]);
    // ---- the touched rows base - 1, base, each once: with one row the second repeats the first
    if constexpr (Air::N_CONSTRAINTS > 0) {
#pragma unroll 1
        for (uint32_t t = 0; t < 2; t++) {
            ctx.row = (base + mask + t) & mask;
            ctx.on = live && t < n;
            hunt_constraints_from<Air, 0>(ctx);
        }
    }
    uint32_t d_all[3] = {0, 0, 0}, d_u[3] = {0, 0, 0};
    const bool survivor = live && !ctx.caught;
    if constexpr (Air::N_INTERACTIONS > 0) {
        if (__ballot(survivor)) {
            uint32_t honest[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll 1
            for (uint32_t t = 0; t < 2; t++) {
                ctx.row = (base + mask + t) & mask;
                ctx.on = survivor && t < n;
                hunt_interactions_from<Air, 0>(ctx);
                if (ctx.on)
                    for (int k = 0; k < 6; k++) {
                        const uint32_t s = honest[k] + a.honest[(size_t)k * n + ctx.row];
                        honest[k] = s >= P ? s - P : s;
                    }
            }
            for (int k = 0; k < 3; k++) {
                d_all[k] = ctx.print[k] >= honest[k] ? ctx.print[k] - honest[k] : ctx.print[k] + P - honest[k];
                d_u[k] = ctx.print_u[k] >= honest[3 + k] ? ctx.print_u[k] - honest[3 + k] : ctx.print_u[k] + P - honest[3 + k];
            }
        }
    }
    const bool changed = survivor && (d_all[0] | d_all[1] | d_all[2]) != 0;
    const bool open = changed && (d_u[0] | d_u[1] | d_u[2]) != 0;
    JoinRecord r;
    r.d[0] = d_u[0]; r.d[1] = d_u[1]; r.d[2] = d_u[2];
    r.where = a.where;
    r.col = ctx.col0;
    r.row = (uint32_t)base;
    r.delta = e0;
    r.pad = 0;
    join_emit(open, a.counters + 0, a.open, a.cap_open, r);
    join_emit(changed && !open, a.counters + 1, a.absorbed, a.cap_absorbed, r);
}

template <class Air>
hipError_t launch_join_t(hipStream_t st, const JoinArgs &a, unsigned row_blocks, unsigned n_candidates) {
    if (row_blocks == 0 || n_candidates == 0 || n_candidates > HUNT_MAX_CANDIDATES) return hipErrorInvalidValue;
    join_kernel<Air><<<dim3(row_blocks, n_candidates), 256, 0, st>>>(a);
    return hipGetLastError();
}
template <class Air>
hipError_t launch_supply_t(hipStream_t st, const JoinArgs &a) {
    join_supply_kernel<Air><<<(unsigned)((((size_t)1 << a.h.log_n) + 255) / 256), 256, 0, st>>>(a);
    return hipGetLastError();
}
template <class Air>
ChipDesc with_join_fn(ChipDesc d) {
    d.launch_join = &launch_join_t<Air>;
    return d;
}
template <class Air>
ChipDesc with_supply_fn(ChipDesc d) {
    d.launch_supply = &launch_supply_t<Air>;
    return d;
}
#endif  // __HIPCC__

}  // namespace dvt
