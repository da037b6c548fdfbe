// The watchpoint search (watch.h) over the cycle records a prepared job holds in HBM: count, scan, emit.
//
// One thread per record, the launch shape of memory_records_kernel (256 threads, a fixed span of DVT_WATCH_SPAN = 4096
// consecutive records per workgroup, 16 rounds of 256).  Execution order inside a span is round by round and, inside a round,
// wave by wave: a span is 64 UNITS of 64 consecutive records, unit u = 4 round + wave.  The queries and the precompile shapes
// travel as kernel arguments, so every query field is wave-uniform; rd, class and offset of an instruction come from two
// static words per instruction.  A thread reads the first and the third 16-byte word of its record (idx a b c; m_prev m_ts
// sh_ab sh_cm) and decides with watch::decode / watch::test, the functions the host path runs.
//   count   every lane tests its record against every query (a lane past the end of the shard and a lane with a record the
//           executor never writes take part with a false predicate; nobody returns early); a ballot per query and wave, one
//           LDS add per wave with a hit, one u32 per (span, query) written by the workgroup.  Bad records are counted.
//   scan    one workgroup per shard: wave w takes the queries w, w + 4, ...; 64 spans per step, an inclusive scan by
//           __shfl_up and a carried base; writes the exclusive offset of every (span, query) and the shard's totals.
//   emit    given, per query, the rank of the shard's first hit, the total and K: a workgroup whose span has no rank in
//           [0, K) or [total - K, total) of any query leaves at once (all of it).  Otherwise it tests its records again,
//           keeps the 16 hit bits of every record in LDS and the hit counts of every (unit, query), turns those into
//           exclusive offsets, and a hit's rank is  shard base + span offset + unit offset + the ballot prefix of its lane
//           (mbcnt).  A hit whose rank is kept reads its record again and writes its dvt_watch_hit to slot rank (first list) or
//           K + rank - (total - K) (last list): the order is exact and no slot is written twice with different content.
// Every loop is bounded by the launch, by the 72 words of a call or by the table sizes; every output index is checked
// against its array before the store.
#include "kernels.h"
#include "records.cuh"
#include "watch.h"

namespace dvt {

namespace {

constexpr uint32_t ROUNDS = watch::SPAN / 256, UNITS = watch::SPAN / 64;
static_assert(watch::MAX_Q <= 16, "a record's hit bits are kept in 16 bits");

// bit q: the record is a hit of query q
__device__ __forceinline__ uint32_t hit_bits(const WatchArgs &a, const watch::Decoded &d, const rv32::CycleRec &rec, uint32_t row) {
    uint32_t bits = 0;
    for (uint32_t q = 0; q < a.n_queries && q < watch::MAX_Q; q++) {
        watch::CallMatch cm;
        if (watch::test(a.q[q], d, rec, a.shard, row, a.sh, &cm)) bits |= 1u << q;
    }
    return bits;
}

__global__ void __launch_bounds__(256) watch_count_kernel(const rv32::CycleRec *recs, size_t n_recs, const WatchArgs a, uint32_t *span_counts,
                                                          unsigned long long *bad_records) {
    __shared__ uint32_t cnt[watch::MAX_Q], wg_bad;
    if (threadIdx.x < watch::MAX_Q) cnt[threadIdx.x] = 0;
    if (threadIdx.x == 0) wg_bad = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * watch::SPAN;
    const bool lane0 = (threadIdx.x & 63) == 0;
    for (uint32_t k = 0; k < ROUNDS; k++) {   // (every thread runs every round: the ballots need all lanes)
        const size_t r = base + (size_t)k * 256 + threadIdx.x;
        const rv32::CycleRec rec = read_record(recs, r, n_recs);
        const watch::Decoded d = watch::decode(rec, a.n_instr, a.text_base, a.statics, a.offs, a.sh);
        if (r < n_recs && d.bad) atomicAdd(&wg_bad, 1u);
        const uint32_t bits = hit_bits(a, d, rec, (uint32_t)r);
        if (__ballot(bits != 0) == 0) continue;   // (wave-uniform)
        for (uint32_t q = 0; q < a.n_queries && q < watch::MAX_Q; q++) {
            const unsigned long long b = __ballot((bits >> q) & 1);
            if (b && lane0) atomicAdd(&cnt[q], (uint32_t)__popcll(b));
        }
    }
    __syncthreads();
    if (threadIdx.x < a.n_queries && threadIdx.x < watch::MAX_Q) span_counts[(size_t)blockIdx.x * a.n_queries + threadIdx.x] = cnt[threadIdx.x];
    if (threadIdx.x == 0 && wg_bad) atomicAdd(bad_records, (unsigned long long)wg_bad);
}

__global__ void __launch_bounds__(256) watch_scan_kernel(const uint32_t *span_counts, uint32_t *span_offs, uint32_t n_spans, uint32_t n_queries, uint32_t *totals) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (uint32_t q = wave; q < n_queries; q += 4) {
        uint32_t carry = 0;
        for (uint32_t s0 = 0; s0 < n_spans; s0 += 64) {
            const uint32_t s = s0 + lane;
            const uint32_t v = s < n_spans ? span_counts[(size_t)s * n_queries + q] : 0;
            uint32_t inc = v;
            for (uint32_t dlt = 1; dlt < 64; dlt <<= 1) {
                const uint32_t t = (uint32_t)__shfl_up((int)inc, dlt);
                if (lane >= dlt) inc += t;
            }
            if (s < n_spans) span_offs[(size_t)s * n_queries + q] = carry + inc - v;
            carry += (uint32_t)__shfl((int)inc, 63);
        }
        if (lane == 0) totals[q] = carry;
    }
}

__global__ void __launch_bounds__(256) watch_emit_kernel(const rv32::CycleRec *recs, size_t n_recs, const WatchArgs a, const WatchEmitArgs e,
                                                         const uint32_t *span_counts, const uint32_t *span_offs, dvt_watch_hit *out) {
    __shared__ uint32_t unit[UNITS][watch::MAX_Q];
    __shared__ uint16_t bits_of[watch::SPAN];
    __shared__ uint32_t wanted;
    const uint32_t nq = a.n_queries < watch::MAX_Q ? a.n_queries : watch::MAX_Q, K = e.cap_each;
    if (threadIdx.x == 0) wanted = 0;
    __syncthreads();
    if (threadIdx.x < nq) {   // does a rank of this span belong to a kept range of the query?
        const uint32_t q = threadIdx.x, c = span_counts[(size_t)blockIdx.x * nq + q];
        const unsigned long long lo = e.base[q] + span_offs[(size_t)blockIdx.x * nq + q], hi = lo + c;
        const watch::Keep keep = watch::keep_of(e.total[q], K);
        if (c && (lo < keep.first_end || hi > keep.last_begin)) atomicOr(&wanted, 1u << q);
    }
    __syncthreads();
    const uint32_t want = wanted;
    if (!want) return;   // (the whole workgroup)
    const size_t base = (size_t)blockIdx.x * watch::SPAN;
    const uint32_t wave = threadIdx.x >> 6;
    const bool lane0 = (threadIdx.x & 63) == 0;
    for (uint32_t k = 0; k < ROUNDS; k++) {
        const size_t r = base + (size_t)k * 256 + threadIdx.x;
        const rv32::CycleRec rec = read_record(recs, r, n_recs);
        const watch::Decoded d = watch::decode(rec, a.n_instr, a.text_base, a.statics, a.offs, a.sh);
        const uint32_t bits = hit_bits(a, d, rec, (uint32_t)r);
        bits_of[k * 256 + threadIdx.x] = (uint16_t)bits;
        for (uint32_t q = 0; q < nq; q++) {
            const unsigned long long b = __ballot((bits >> q) & 1);
            if (lane0) unit[4 * k + wave][q] = (uint32_t)__popcll(b);
        }
    }
    __syncthreads();
    if (threadIdx.x < nq) {
        uint32_t run = 0;
        for (uint32_t u = 0; u < UNITS; u++) {
            const uint32_t c = unit[u][threadIdx.x];
            unit[u][threadIdx.x] = run;
            run += c;
        }
    }
    __syncthreads();
    for (uint32_t k = 0; k < ROUNDS; k++) {
        const size_t r = base + (size_t)k * 256 + threadIdx.x;
        const uint32_t bits = bits_of[k * 256 + threadIdx.x] & want;
        if (__ballot(bits != 0) == 0) continue;   // (wave-uniform)
        for (uint32_t q = 0; q < nq; q++) {
            const bool hit = (bits >> q) & 1;
            const unsigned long long b = __ballot(hit);   // (all lanes of the wave: nothing above diverges)
            const unsigned long long rank = e.base[q] + span_offs[(size_t)blockIdx.x * nq + q] + unit[4 * k + wave][q] + lanes_below(b);
            const watch::Keep keep = watch::keep_of(e.total[q], K);
            const bool in_first = rank < keep.first_end, in_last = rank >= keep.last_begin && rank - keep.last_begin < K;
            if (hit && (in_first || in_last) && r < n_recs) {
                const rv32::CycleRec rec = read_record(recs, r, n_recs);
                const watch::Decoded d = watch::decode(rec, a.n_instr, a.text_base, a.statics, a.offs, a.sh);
                watch::CallMatch cm{};
                if (watch::test(a.q[q], d, rec, a.shard, (uint32_t)r, a.sh, &cm)) {   // (it did a moment ago)
                    const dvt_watch_hit h = watch::make_hit(q, a.q[q], d, rec, a.shard, (uint32_t)r, cm);
                    if (in_first) out[(size_t)2 * q * K + rank] = h;
                    if (in_last) out[(size_t)(2 * q + 1) * K + (rank - keep.last_begin)] = h;
                }
            }
        }
    }
}

bool args_ok(const WatchArgs &a) { return a.n_instr && a.n_queries >= 1 && a.n_queries <= watch::MAX_Q && a.sh.n <= memrep::MAX_PRE; }

}  // namespace

hipError_t launch_watch_count(hipStream_t st, const rv32::CycleRec *d_recs, size_t n_recs, const WatchArgs &a, uint32_t *d_span_counts,
                              unsigned long long *d_bad_records) {
    if (!n_recs) return hipSuccess;
    if (!args_ok(a)) return hipErrorInvalidValue;
    watch_count_kernel<<<(unsigned)((n_recs + watch::SPAN - 1) / watch::SPAN), 256, 0, st>>>(d_recs, n_recs, a, d_span_counts, d_bad_records);
    return hipGetLastError();
}

hipError_t launch_watch_scan(hipStream_t st, const uint32_t *d_span_counts, uint32_t *d_span_offs, uint32_t n_spans, uint32_t n_queries, uint32_t *d_totals) {
    if (n_queries < 1 || n_queries > watch::MAX_Q) return hipErrorInvalidValue;
    watch_scan_kernel<<<1, 256, 0, st>>>(d_span_counts, d_span_offs, n_spans, n_queries, d_totals);
    return hipGetLastError();
}

hipError_t launch_watch_emit(hipStream_t st, const rv32::CycleRec *d_recs, size_t n_recs, const WatchArgs &a, const WatchEmitArgs &e,
                             const uint32_t *d_span_counts, const uint32_t *d_span_offs, void *d_out) {
    if (!n_recs) return hipSuccess;
    if (!args_ok(a) || e.cap_each < 1 || e.cap_each > watch::MAX_KEEP) return hipErrorInvalidValue;
    watch_emit_kernel<<<(unsigned)((n_recs + watch::SPAN - 1) / watch::SPAN), 256, 0, st>>>(d_recs, n_recs, a, e, d_span_counts, d_span_offs, static_cast<dvt_watch_hit *>(d_out));
    return hipGetLastError();
}

}  // namespace dvt
