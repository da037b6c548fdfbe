// The bus ledger: WHICH tuples of the LogUp buses do not cancel, over the same generated AIR source (gen/air_*.inc) as K4,
// K5 and the trace-row checks (LedgerRowCtx: the fifth context of the generated code, next to BusRowCtx of check.cuh).
// Two passes over the interactions of every chip table, and no thread ever waits for another:
//   TALLY    every occurrence (a row's interaction with a non-zero multiplicity) adds its canonical signed multiplicity m,
//            m w1 mod p and m w2 mod p to the three 64-bit words of the bucket its key selects (key: ledger_key.h; w1, w2 in
//            [1, p) from the key).  The occurrences of a balanced tuple add up to 0 mod p in all three words, so an honest
//            job leaves every bucket zero.
//   close    one dirty bit per bucket with a non-zero word, and their count.
//   COLLECT  (only when a bucket is dirty) every occurrence of a dirty bucket goes into a bounded open-addressing table of
//            fixed records: at most LEDGER_PROBES probes, one atomicCAS on the record's key word per probe, then atomics on
//            the record's sum, counters and lowest occurrence.  The thread that claims a record writes bus, arity and
//            values with plain stores; nobody reads them on the device.  A full neighbourhood sets the overflow flag and
//            drops the occurrence: the records that exist still saw every occurrence of their tuple.
// The host drops the records whose sum is 0 (balanced tuples that share a dirty bucket).
//
// WHAT IT MISSES.  An unmatched tuple goes unseen only when its bucket holds other unmatched tuples and all three words
// cancel: for tuples with nets m_i that needs sum m_i = sum m_i w1_i = sum m_i w2_i = 0 mod p with independent weights,
// probability about p^-2 ~ 2^-60 per bucket that holds several.  Two different tuples with one 64-bit key (2^-63 per pair)
// would share a record.  Both are the miss probability of a diagnostic for rows that are wrong by accident, not a
// soundness claim: the seed does not depend on the rows.
//
// NO OVERFLOW.  Every addend is below p < 2^31.  A launch has at most 2^22 rows of at most 2^10 interactions, i.e. fewer
// than 2^32 terms per word even if all fall into one; on top of a word reduced below p that stays under 2^63 + 2^31.  Every
// launch is followed by ledger_reduce_kernel, which takes the words mod p again.
#pragma once
#include <algorithm>

#include "ledger_key.h"
#include "machine.h"   // ChipDesc::launch_ledger; bus_row_blocks of check.cuh

namespace dvt {

constexpr uint32_t LEDGER_TALLY = 0, LEDGER_COLLECT = 1;
constexpr uint32_t LEDGER_MAX_ARITY = 40;   // = DVT_LEDGER_MAX_ARITY (include/dvt_prover.h)
constexpr uint32_t LEDGER_PROBES = 64;
constexpr uint32_t LEDGER_MAX_INTERACTIONS = 1024;   // the interaction field of an occurrence has 10 bits
constexpr unsigned long long LEDGER_NO_OCCURRENCE = ~0ull;

struct LedgerSlot {
    unsigned long long key;      // 0: free; else the tuple's key | 1
    unsigned long long sum;      // of the signed multiplicities; below p between launches
    unsigned long long first;    // lowest ledger_occurrence (LEDGER_NO_OCCURRENCE in a free record)
    unsigned long long n_send, n_recv;
    uint32_t bus, arity;
    uint32_t values[LEDGER_MAX_ARITY];   // canonical
};
static_assert(sizeof(LedgerSlot) == 208, "the host downloads these records");

struct LedgerArgs {
    const uint32_t *main, *prep, *pub;   // as BusArgs
    uint32_t log_n;
    uint32_t mode;                  // LEDGER_TALLY or LEDGER_COLLECT
    uint64_t seed;
    uint32_t log_buckets;           // 10..24
    unsigned long long *tally;      // [2^log_buckets][3]
    const uint32_t *dirty;          // [2^log_buckets / 32] bitmap (COLLECT)
    LedgerSlot *slots;              // [cap_slots] (COLLECT)
    uint32_t cap_slots;
    uint32_t *flags;                // [0] dirty buckets (close), [1] overflow
    uint32_t tag, chip;             // of the occurrences of this launch
};
// a tuple the host adds itself, keyed by the host with ledger_key
struct LedgerTuple {
    uint64_t key, occurrence;
    uint32_t bus, arity, m, send;   // m: canonical signed multiplicity; send: sign > 0
    uint32_t values[LEDGER_MAX_ARITY];
};

#if defined(__HIPCC__)
// One occurrence of a keyed tuple.  `write_values(dst)` stores the canonical values; it runs only in the thread that claims
// a record.  Every index is bounded here: bucket < 2^log_buckets by the shift, the probe index by the modulo.
template <class WriteValues>
__device__ __forceinline__ void ledger_apply(const LedgerArgs &a, uint64_t key, uint32_t bus, uint32_t arity, uint32_t m, bool send,
                                             uint64_t occurrence, const WriteValues &write_values) {
    const uint32_t bucket = ledger_bucket(key, a.log_buckets);
    if (a.mode == LEDGER_TALLY) {
        unsigned long long *t = a.tally + (size_t)bucket * 3;
        atomicAdd(t, (unsigned long long)m);
        atomicAdd(t + 1, (unsigned long long)((uint64_t)m * ledger_weight(key, 0) % P));
        atomicAdd(t + 2, (unsigned long long)((uint64_t)m * ledger_weight(key, 1) % P));
        return;
    }
    if (!((a.dirty[bucket >> 5] >> (bucket & 31)) & 1u)) return;
    const unsigned long long want = key | 1ull;
    uint32_t at = ledger_start_slot(key, a.cap_slots);
    const uint32_t probes = a.cap_slots < LEDGER_PROBES ? a.cap_slots : LEDGER_PROBES;
    for (uint32_t i = 0; i < probes; i++) {
        LedgerSlot *s = a.slots + at;
        const unsigned long long old = atomicCAS(&s->key, 0ull, want);
        if (old == 0ull) {   // claimed: nobody else writes these words, and only the host reads them
            s->bus = bus;
            s->arity = arity;
            write_values(s->values);
        }
        if (old == 0ull || old == want) {
            atomicAdd(&s->sum, (unsigned long long)m);
            atomicAdd(send ? &s->n_send : &s->n_recv, 1ull);
            atomicMin(&s->first, (unsigned long long)occurrence);
            return;
        }
        at = at + 1 == a.cap_slots ? 0 : at + 1;
    }
    atomicOr(a.flags + 1, 1u);
}

// the occurrence of a row: key from the Montgomery values as they stand in the generated code's array
static __device__ __noinline__ void ledger_row_occurrence(const LedgerArgs &a, uint32_t row, uint32_t j, uint32_t bus, bool send, Fp mult,
                                                          const Fp *vals, uint32_t nv) {
    if (nv > LEDGER_MAX_ARITY || j >= LEDGER_MAX_INTERACTIONS) { atomicOr(a.flags + 1, 1u); return; }
    uint64_t h = ledger_key_begin(a.seed, bus, nv);   // ledger_key without the canonical copy of the values
    for (uint32_t k = 0; k < nv; k++) h = ledger_key_value(h, vals[k].canonical());
    const uint32_t m = (send ? mult : -mult).canonical();
    ledger_apply(a, h, bus, nv, m, send, ledger_occurrence(a.tag, a.chip, row, j), [&](uint32_t *dst) {
        for (uint32_t k = 0; k < nv; k++) dst[k] = vals[k].canonical();
    });
}

template <class Air>
struct LedgerRowCtx {
    using T = Fp;
    const LedgerArgs &a;
    size_t n, row;
    bool live;   // row < n
    __device__ LedgerRowCtx(const LedgerArgs &args, size_t r)
        : a(args), n((size_t)1 << args.log_n), row(r & (((size_t)1 << args.log_n) - 1)), live(r < ((size_t)1 << args.log_n)) {}
    __device__ static T K(uint32_t m) { return Fp::raw(m); }
    __device__ static T KI(uint32_t canonical) { return Fp::from_canonical(canonical); }
    __device__ T main(int c, int r) const { return Fp::raw(a.main[(size_t)c * n + ((row + r) & (n - 1))]); }
    __device__ T prep(int c, int r) const { return Fp::raw(a.prep[(size_t)c * n + ((row + r) & (n - 1))]); }
    __device__ T pub(int k) const { return Fp::raw(a.pub[k]); }
    __device__ __forceinline__ void interaction(int j, int bus, int sign, int /*scope*/, const T &mult, const T *vals, int nv) {
        if (!live || mult.is_zero() || bus < 0) return;
        ledger_row_occurrence(a, (uint32_t)row, (uint32_t)j, (uint32_t)bus, sign > 0, mult, vals, (uint32_t)nv);
    }
};

// grid (row blocks <= BUS_ROW_BLOCKS_MAX, Air::N_LPARTS), as bus_rows_kernel: the LogUp group blockIdx.y on the rows
// blockIdx.x * 256 + t, + gridDim.x * 256, ...  The trip count is fixed by the launch.
template <class Air>
__global__ void __launch_bounds__(256) ledger_rows_kernel(LedgerArgs a) {
    const size_t n = (size_t)1 << a.log_n;
    for (size_t base = (size_t)blockIdx.x * 256; base < n; base += (size_t)gridDim.x * 256) {
        LedgerRowCtx<Air> ctx(a, base + threadIdx.x);
        interactions_of_part<Air, 0>(ctx, (int)blockIdx.y);
    }
}
template <class Air>
hipError_t launch_ledger_t(hipStream_t st, const LedgerArgs &a) {
    static_assert(Air::MAX_ARITY <= (int)LEDGER_MAX_ARITY && Air::N_INTERACTIONS <= (int)LEDGER_MAX_INTERACTIONS, "a tuple or an occurrence would not fit its record");
    if (Air::N_INTERACTIONS == 0) return hipSuccess;
    ledger_rows_kernel<Air><<<dim3(bus_row_blocks(a.log_n), Air::N_LPARTS), 256, 0, st>>>(a);
    return hipGetLastError();
}
template <class Air>
ChipDesc with_ledger_fn(ChipDesc d) {
    d.launch_ledger = &launch_ledger_t<Air>;
    return d;
}
#endif  // __HIPCC__

}  // namespace dvt
