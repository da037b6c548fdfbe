// The forgery hunt: which one- and two-cell changes of a chip's trace rows does NOTHING reject?  Over the same generated AIR
// source (gen/air_*.inc) as K4, K5, the trace-row checks and the bus ledger (HuntRowCtx: the sixth context of the generated
// code).  HuntRowCtx is a VIEW of the trace: main(c, rot) returns value + delta where (c, (row + rot) mod n) is a changed
// cell, and the trace itself is only read.
//
// A candidate is one change (col, delta) or a pair of changes; a workgroup holds 256 consecutive base rows of ONE candidate
// (grid: x = row blocks of the window, y = candidates of the launch), so the changed columns and deltas are wave-uniform:
// the compare against the literal column index of the generated code is scalar, and the loads stay coalesced as in
// check_rows_kernel.  One EVALUATION is one row evaluated for one candidate; a thread evaluates the touched rows of its
// forgery, {row - 1, row} over the changed cells (the generated AIR reads rotations 0 and 1 only), each once.
//   constraint pass  every unit of the chip on every touched row (units, `when` predicates and the closed-form identities
//                    at xi exactly as in check.cuh) sets a per-thread flag: no atomic.  A constraint group is skipped when
//                    the ballot says every live lane of the wave is caught already.
//   multiset pass    for the survivors only: the fingerprints of the touched rows under the view against those of the
//                    honest table (HUNT_HONEST: one launch per call writes them, [3][n]).
//   HUNT_CELLS       the single-cell map, bits [delta][col][window row] (set: the change ESCAPES, the cell is free for that
//                    delta on that row), written as one ballot word per wave by one lane: no atomic.  It stays on the device.
//   HUNT_PAIRS       a pair of two free cells is dropped without being evaluated; the others are counted (one atomic add per
//                    wave); a pair that escapes is REPORTED: one atomic add for its index, the record stored while the index is
//                    below the capacity.
// Every loop has a trip count fixed by the launch, no thread waits for another, and all indices are masked or bounded by
// the grid: rows by n - 1, columns by the literals of the generated code, candidates by gridDim.y.
//
// THE FINGERPRINT of a row is (sum m, sum m w1(key), sum m w2(key)) mod p over its interactions with a non-zero multiplicity
// m (signed, canonical), key = the ledger's key of (bus, arity, values) under the call's 64-bit key (ledger_key.h), w1, w2
// in [1, p).  Equal signed multisets over the touched rows give equal sums: an escape of the exact multiset is never called
// caught.  WHAT IT MISSES: multisets that differ in tuples with nets m_i are called equal only when sum m_i = sum m_i w1_i =
// sum m_i w2_i = 0 mod p; one differing tuple never is (m w1 != 0), several are with probability about p^-2 ~ 2^-60 over
// the key, and two tuples share a 64-bit key with 2^-63 per pair: the order of the ledger's own miss probability (ledger.cuh
// "WHAT IT MISSES").  Multiplicities are compared mod p: nets that differ by a multiple of p are equal here.  As with the
// checker's xi this is the miss probability of a diagnostic: the key does not depend on the rows.
#pragma once
#include "ledger_key.h"
#include "machine.h"

namespace dvt {

constexpr uint32_t HUNT_HONEST = 0, HUNT_CELLS = 1, HUNT_PAIRS = 2;
constexpr uint32_t HUNT_MAX_DELTAS = 8;          // = DVT_HUNT_MAX_DELTAS (include/dvt_prover.h)
constexpr uint32_t HUNT_NO_COL = 0xffffffffu;    // a change that is not there (no literal column equals it)
constexpr unsigned HUNT_MAX_CANDIDATES = 65535;  // of one launch: gridDim.y

struct HuntEscape {   // = dvt_escape
    uint32_t row, n_cells;
    uint32_t col[2], row_off[2], delta[2];
    uint32_t alone;
};
static_assert(sizeof(HuntEscape) == 36, "the host copies these records out");

struct HuntArgs {
    const uint32_t *main, *prep, *pub;   // as CheckArgs
    const Fp4 *xi_pows;
    const double *xi_d;
    uint32_t log_n;
    uint32_t mode;                    // HUNT_HONEST, HUNT_CELLS or HUNT_PAIRS
    uint64_t key;                     // of the fingerprints
    uint32_t *honest;                 // [3][n] fingerprints of the honest rows: written by HUNT_HONEST, read by the others
    uint32_t row_first, rows;         // base rows (row_first + i) mod n, i < rows
    uint32_t n_deltas;
    uint32_t delta_m[HUNT_MAX_DELTAS], delta_c[HUNT_MAX_DELTAS];   // Montgomery / canonical
    const uint32_t *cols;             // [n_cols] the columns the changed cells are taken from
    uint32_t n_cols;
    uint32_t cand_first;              // candidate of blockIdx.y = 0: CELLS delta * n_cols + k, PAIRS (pair * n_deltas + d0) * n_deltas + d1
    unsigned long long *map;          // [n_deltas * n_cols][map_words] the single-cell map over the window indices i < map_rows
    uint32_t map_words, map_rows;
    const uint32_t *pairs;            // PAIRS: k0 | k1 << 16, positions in cols
    uint32_t adjacent;                // PAIRS: the second cell lies in the next row
    HuntEscape *out;                  // [cap]
    uint32_t cap;
    unsigned long long *counters;     // [0] reported pairs, [1] pairs evaluated
};

#if defined(__HIPCC__)
struct HuntPrint { uint32_t w[3]; };
// what one interaction adds to the fingerprint of its row (key as ledger_row_occurrence keys it)
static __device__ __noinline__ HuntPrint hunt_print_of(uint64_t key, uint32_t bus, bool send, Fp mult, const Fp *vals, uint32_t nv) {
    uint64_t h = ledger_key_begin(key, bus, nv);   // = ledger_key of the canonical values, without a copy of them
    for (uint32_t k = 0; k < nv; k++) h = ledger_key_value(h, vals[k].canonical());
    const uint32_t m = (send ? mult : -mult).canonical();
    return {{m, (uint32_t)((uint64_t)m * ledger_weight(h, 0) % P), (uint32_t)((uint64_t)m * ledger_weight(h, 1) % P)}};
}

template <class Air>
struct HuntRowCtx {
    using T = Fp;
    const HuntArgs &a;
    size_t n, row;
    uint32_t col0, col1;     // wave-uniform; HUNT_NO_COL: no such change
    size_t crow0, crow1;     // the rows of the changed cells
    Fp d0, d1;
    bool on;                 // this lane evaluates this row
    bool caught;
    uint32_t print[3];       // fingerprint of the rows evaluated so far, each word below p
    __device__ HuntRowCtx(const HuntArgs &args) : a(args), n((size_t)1 << args.log_n), row(0), col0(HUNT_NO_COL), col1(HUNT_NO_COL), crow0(0), crow1(0),
                                                   d0(Fp::zero()), d1(Fp::zero()), on(false), caught(false), print{0, 0, 0} {}
    __device__ static T K(uint32_t m) { return Fp::raw(m); }
    __device__ static T KI(uint32_t canonical) { return Fp::from_canonical(canonical); }
    __device__ __forceinline__ T main(int c, int r) const {
        const size_t at = (row + r) & (n - 1);
        Fp v = Fp::raw(a.main[(size_t)c * n + at]);
        if ((uint32_t)c == col0 && at == crow0) v = v + d0;
        if ((uint32_t)c == col1 && at == crow1) v = v + d1;
        return v;
    }
    __device__ T prep(int c, int r) const { return Fp::raw(a.prep[(size_t)c * n + ((row + r) & (n - 1))]); }
    __device__ T pub(int k) const { return Fp::raw(a.pub[k]); }
    __device__ __forceinline__ void constraint(int, int when, const T &v) {
        const bool active = when == WHEN_ALL || (when == WHEN_FIRST && row == 0) || (when == WHEN_LAST && row == n - 1) ||
                            (when == WHEN_TRANS && row != n - 1);
        caught |= on && active && !v.is_zero();
    }
    __device__ __forceinline__ Fp4 poly(const T *v, int nv) const {
        DotAcc4 s;
        for (int k = 0; k < nv; k++) {
            s.add(a.xi_d + 4 * k, v[k]);
            if ((k & 31) == 31) s.reduce();
        }
        return s.value();
    }
    __device__ __forceinline__ Fp4 alpha_minus(uint32_t k) const { return a.xi_pows[1] - Fp::from_canonical(k); }
    __device__ __forceinline__ void fold_poly(int, const Fp4 &tot) { caught |= on && tot != Fp4::zero(); }
    __device__ __forceinline__ void interaction(int, int bus, int sign, int /*scope*/, const T &mult, const T *vals, int nv) {
        if (!on || mult.is_zero() || bus < 0) return;
        const HuntPrint f = hunt_print_of(a.key, (uint32_t)bus, sign > 0, mult, vals, (uint32_t)nv);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint32_t s = print[k] + f.w[k];   // both below p < 2^31
            print[k] = s >= P ? s - P : s;
        }
    }
};

// the constraint groups from PART on; a group runs only while a lane of the wave that evaluates this row is not caught
template <class Air, int PART, class Ctx>
__device__ __forceinline__ void hunt_constraints_from(Ctx &ctx) {
    if (__ballot(ctx.on && !ctx.caught)) Air::template constraints_part<PART>(ctx);
    if constexpr (PART + 1 < Air::N_PARTS) hunt_constraints_from<Air, PART + 1>(ctx);
}
template <class Air, int LP, class Ctx>
__device__ __forceinline__ void hunt_interactions_from(Ctx &ctx) {
    Air::template interactions_part<LP>(ctx);
    if constexpr (LP + 1 < Air::N_LPARTS) hunt_interactions_from<Air, LP + 1>(ctx);
}

// grid (row blocks, candidates of the launch; HUNT_HONEST: (row blocks of the table, 1))
template <class Air>
__global__ void __launch_bounds__(256) hunt_kernel(HuntArgs a) {
    const size_t n = (size_t)1 << a.log_n, mask = n - 1;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;   // window index of the base row
    const uint32_t lane = threadIdx.x & 63;
    HuntRowCtx<Air> ctx(a);
    if (a.mode == HUNT_HONEST) {
        if constexpr (Air::N_INTERACTIONS > 0) {
            ctx.row = i & mask;
            ctx.on = i < n;
            hunt_interactions_from<Air, 0>(ctx);
        }
        if (i < n)
            for (int k = 0; k < 3; k++) a.honest[(size_t)k * n + i] = ctx.print[k];
        return;
    }
    // ---- the candidate of this workgroup (scalar)
    const uint32_t cand = a.cand_first + blockIdx.y;
    const size_t base = ((size_t)a.row_first + i) & mask;   // (lanes past the window run along on a row of the table)
    bool live = i < a.rows;                                 // ... and enter no ballot
    uint32_t k0, k1 = 0, e0, e1 = 0;
    bool free0 = false, free1 = false;
    if (a.mode == HUNT_CELLS) {
        e0 = cand / a.n_cols;
        k0 = cand % a.n_cols;
    } else {
        const uint32_t dd = cand % (a.n_deltas * a.n_deltas), pr = a.pairs[cand / (a.n_deltas * a.n_deltas)];
        e0 = dd / a.n_deltas;
        e1 = dd % a.n_deltas;
        k0 = pr & 0xffffu;
        k1 = pr >> 16;
        ctx.col1 = a.cols[k1];
        ctx.crow1 = (base + a.adjacent) & mask;
        ctx.d1 = Fp::raw(a.delta_m[e1]);
    }
    ctx.col0 = a.cols[k0];
    ctx.crow0 = base;
    ctx.d0 = Fp::raw(a.delta_m[e0]);
    if (a.mode == HUNT_PAIRS) {
        if (live) {   // the single-cell map: is each change free on its own?
            const uint32_t i1 = a.adjacent ? (i + 1 < a.map_rows ? i + 1 : 0) : i;
            free0 = (a.map[((size_t)e0 * a.n_cols + k0) * a.map_words + (i >> 6)] >> (i & 63)) & 1;
            free1 = (a.map[((size_t)e1 * a.n_cols + k1) * a.map_words + (i1 >> 6)] >> (i1 & 63)) & 1;
        }
        live = live && !(free0 && free1) && !(ctx.col0 == ctx.col1 && ctx.crow0 == ctx.crow1);
        const unsigned long long tried = __ballot(live);
        if (tried && lane == (uint32_t)(__ffsll((long long)tried) - 1)) atomicAdd(a.counters + 1, (unsigned long long)__popcll(tried));
    }
    // ---- the touched rows base - 1, base (, base + 1), each once: below n rows the later ones repeat the earlier
    const uint32_t n_touched = a.mode == HUNT_PAIRS && a.adjacent ? 3 : 2;
    if constexpr (Air::N_CONSTRAINTS > 0) {
#pragma unroll 1
        for (uint32_t t = 0; t < n_touched; t++) {
            ctx.row = (base + mask + t) & mask;
            ctx.on = live && t < n;
            hunt_constraints_from<Air, 0>(ctx);
        }
    }
    if constexpr (Air::N_INTERACTIONS > 0) {
        const bool survivor = live && !ctx.caught;
        if (__ballot(survivor)) {
            uint32_t honest[3] = {0, 0, 0};
#pragma unroll 1
            for (uint32_t t = 0; t < n_touched; t++) {
                ctx.row = (base + mask + t) & mask;
                ctx.on = survivor && t < n;
                hunt_interactions_from<Air, 0>(ctx);
                if (ctx.on)
                    for (int k = 0; k < 3; k++) {
                        const uint32_t s = honest[k] + a.honest[(size_t)k * n + ctx.row];
                        honest[k] = s >= P ? s - P : s;
                    }
            }
            ctx.caught |= survivor && (ctx.print[0] != honest[0] || ctx.print[1] != honest[1] || ctx.print[2] != honest[2]);
        }
    }
    const bool escapes = live && !ctx.caught;
    if (a.mode == HUNT_CELLS) {
        const unsigned long long word = __ballot(escapes);
        if (lane == 0) a.map[(size_t)cand * a.map_words + (i >> 6)] = word;
        return;
    }
    if (escapes) {
        const unsigned long long at = atomicAdd(a.counters, 1ull);
        if (at < a.cap) {
            HuntEscape &o = a.out[at];
            o.row = (uint32_t)base;
            o.n_cells = 2;
            o.col[0] = ctx.col0; o.col[1] = ctx.col1;
            o.row_off[0] = 0; o.row_off[1] = a.adjacent;
            o.delta[0] = a.delta_c[e0]; o.delta[1] = a.delta_c[e1];
            o.alone = (free0 ? 0u : 1u) | (free1 ? 0u : 2u);
        }
    }
}
// row_blocks x n_candidates workgroups (n_candidates <= HUNT_MAX_CANDIDATES; HUNT_HONEST: 1)
template <class Air>
hipError_t launch_hunt_t(hipStream_t st, const HuntArgs &a, unsigned row_blocks, unsigned n_candidates) {
    if (row_blocks == 0 || n_candidates == 0 || n_candidates > HUNT_MAX_CANDIDATES) return hipErrorInvalidValue;
    hunt_kernel<Air><<<dim3(row_blocks, n_candidates), 256, 0, st>>>(a);
    return hipGetLastError();
}
template <class Air>
ChipDesc with_hunt_fn(ChipDesc d) {
    d.launch_hunt = &launch_hunt_t<Air>;
    return d;
}
#endif  // __HIPCC__

}  // namespace dvt
