// The device passes of the divergence report (diverge.h) over the cycle records two prepared jobs hold in HBM: classify, merge,
// emit.  (The records of pairs stop - 1 and stop and the rejoin windows are copied out with origin.hip's gather.)
//
// The launch shape of snapshot.hip / origin.hip: 256 threads and a fixed span of DVT_DIVERGE_SPAN = 4096 consecutive pairs per
// workgroup, 16 rounds of 256.  A launch covers one SEGMENT: a run of pairs in which each side stays inside one shard, so both
// record pointers are plain arrays.  The spans of a call are numbered in pair order across its segments.
//   classify  a thread reads the first 16-byte word (idx a b c) and m_prev of both records of its pair and decodes BOTH with
//             watch::decode: whether a record is bad depends on its own idx and its own address, and a store's word after the
//             store on its own b, c and m_prev, so one decode cannot stand for the pair (with equal idx, which is whenever the
//             rest matters, the second decode reads the same two static words again, from cache).  It keeps the class word of diverge::classify for each of its 16 pairs in registers: the 16 rounds are fully
//             unrolled, so nothing is indexed at run time and nothing goes to scratch.  A CONTROL or BAD pair offers its local
//             number to an LDS min: the span's stop.  After the barrier every lane adds up its pairs before the span's stop:
//             the data count, first / last data pair, mask OR, load / store counts in registers and then one LDS atomic each;
//             the 32 register entries by LDS atomics, rounds descending and behind a plain read of the slot, so that the
//             last-write maximum of a register a loop writes costs few atomics.  One DivergeSpan and one DivergeSpanRegs go
//             to global memory, and a span with a stop offers its pair number to the call's stop flag (one 64-bit atomicMin).
//   merge     one workgroup over the span records up to the first span with a stop: the summary counts, regs[32] (8 spans in
//             flight per register, combined through LDS) and, by a wave scan of the data counts, the rank base of every span.
//   emit      as the watchpoints' emit: a workgroup whose span owns none of the first or last K ranks leaves at once (all of
//             it, before any barrier); the others classify again, count the data pairs of every unit of 64 consecutive pairs,
//             and a data pair's rank is  span base + unit offset + the ballot prefix of its lane.
// No lane returns before a barrier unless its whole workgroup does; every loop is bounded by the launch or by the table sizes;
// every index is checked before the store.
#include "diverge.h"
#include "kernels.h"
#include "records.cuh"

namespace dvt {

namespace {

constexpr uint32_t ROUNDS = diverge::SPAN / 256, UNITS = diverge::SPAN / 64, NONE32 = 0xffffffffu;
static_assert(ROUNDS == 16, "a thread's data bits are kept in 16 bits");

// the record at r (the caller checked r)
__device__ __forceinline__ rv32::CycleRec read_record(const rv32::CycleRec *recs, size_t r) { return dvt::read_record(recs, r, r + 1); }

// the class word of the pair at `local` of the segment; 0 (SAME, no rd) for a lane past the end
__device__ __forceinline__ uint32_t class_of(const DivergeArgs &a, uint32_t local) {
    if (local >= a.n_pairs) return 0;
    const rv32::CycleRec ra = read_record(a.rec_a, local), rb = read_record(a.rec_b, local);
    const watch::Decoded da = watch::decode(ra, a.n_instr, a.text_base, a.statics, a.offs, a.sh);
    const watch::Decoded db = watch::decode(rb, a.n_instr, a.text_base, a.statics, a.offs, a.sh);
    return diverge::classify(ra, rb, da, db);
}

__global__ void __launch_bounds__(256) diverge_classify_kernel(const DivergeArgs a, DivergeSpan *spans, DivergeSpanRegs *span_regs, uint32_t cap_spans,
                                                               unsigned long long *stop_flag) {
    __shared__ uint32_t s_stop, s_stopped, s_n_data, s_first, s_last1, s_mask, s_n_load, s_n_store;
    __shared__ uint32_t r_n[32], r_first[32], r_last1[32], r_write1[32];
    const uint32_t base = blockIdx.x * diverge::SPAN;
    const uint32_t n_here = a.n_pairs > base ? (a.n_pairs - base < diverge::SPAN ? a.n_pairs - base : diverge::SPAN) : 0;
    if (threadIdx.x < 32) { r_n[threadIdx.x] = 0; r_first[threadIdx.x] = NONE32; r_last1[threadIdx.x] = 0; r_write1[threadIdx.x] = 0; }
    if (threadIdx.x == 0) { s_stop = n_here; s_stopped = 0; s_n_data = 0; s_first = NONE32; s_last1 = 0; s_mask = 0; s_n_load = 0; s_n_store = 0; }
    __syncthreads();
    uint32_t cls[ROUNDS];
#pragma unroll
    for (uint32_t k = 0; k < ROUNDS; k++) {
        const uint32_t local = k * 256 + threadIdx.x;
        cls[k] = class_of(a, base + local);
        if (cls[k] & diverge::C_STOP) atomicMin(&s_stop, local);
    }
    __syncthreads();
    const uint32_t stop = s_stop;   // (<= n_here)
    uint32_t n_data = 0, first = NONE32, last1 = 0, mask = 0, n_load = 0, n_store = 0;
#pragma unroll
    for (int k = ROUNDS - 1; k >= 0; k--) {   // (descending: the first offers to a maximum are the largest)
        const uint32_t local = (uint32_t)k * 256 + threadIdx.x, w = cls[k];
        if (local == stop && (w & diverge::C_STOP)) s_stopped = w & diverge::C_BAD ? 2 : 1;
        if (local >= stop) continue;   // (no barrier inside the loop)
        const uint32_t rd = (w & diverge::C_RD_MASK) >> diverge::C_RD_SHIFT;   // < 32
        if (rd) {
            if (*(volatile uint32_t *)&r_write1[rd] < local + 1) atomicMax(&r_write1[rd], local + 1);
            if (w & DVT_DIV_RD) {
                atomicAdd(&r_n[rd], 1u);
                atomicMin(&r_first[rd], local);
                if (*(volatile uint32_t *)&r_last1[rd] < local + 1) atomicMax(&r_last1[rd], local + 1);
            }
        }
        if (w & diverge::C_MASK) {
            n_data++;
            first = local;   // (descending: the last assignment is the smallest)
            if (!last1) last1 = local + 1;
            mask |= w & diverge::C_MASK;
            n_load += (w & diverge::C_LOAD_DIFF) != 0;
            n_store += (w & diverge::C_STORE_DIFF) != 0;
        }
    }
    if (n_data) {
        atomicAdd(&s_n_data, n_data);
        atomicMin(&s_first, first);
        atomicMax(&s_last1, last1);
        atomicOr(&s_mask, mask);
        if (n_load) atomicAdd(&s_n_load, n_load);
        if (n_store) atomicAdd(&s_n_store, n_store);
    }
    __syncthreads();
    const uint32_t span = a.span0 + blockIdx.x;
    if (span >= cap_spans) return;   // (the whole workgroup, and no barrier follows)
    if (threadIdx.x < 32) {
        DivergeSpanRegs &o = span_regs[span];
        o.n_diff[threadIdx.x] = r_n[threadIdx.x]; o.first_diff[threadIdx.x] = r_first[threadIdx.x];
        o.last_diff1[threadIdx.x] = r_last1[threadIdx.x]; o.last_write1[threadIdx.x] = r_write1[threadIdx.x];
    }
    if (threadIdx.x == 0) {
        DivergeSpan o;
        o.k_base = a.k0 + base;
        o.stop = stop; o.stopped = s_stopped;
        o.n_data = s_n_data; o.first_data = s_first; o.last_data = s_last1 ? s_last1 - 1 : NONE32;
        o.mask = s_mask; o.n_load = s_n_load; o.n_store = s_n_store;
        spans[span] = o;
        if (s_stopped) atomicMin(stop_flag, a.k0 + base + stop);
    }
}

__global__ void __launch_bounds__(256) diverge_merge_kernel(const DivergeSpan *spans, const DivergeSpanRegs *span_regs, uint32_t n_spans,
                                                            unsigned long long *rank_base, DivergeMerged *out) {
    constexpr unsigned long long NONE = diverge::NONE;
    __shared__ uint32_t first_stop;
    __shared__ unsigned long long g_n[8][32], g_first[8][32], g_last1[8][32], g_write1[8][32];
    if (threadIdx.x == 0) first_stop = n_spans;
    __syncthreads();
    uint32_t mine = n_spans;
    for (uint32_t s = threadIdx.x; s < n_spans; s += 256)
        if (spans[s].stopped && s < mine) mine = s;
    if (mine < n_spans) atomicMin(&first_stop, mine);
    __syncthreads();
    const uint32_t n_used = first_stop < n_spans ? first_stop + 1 : n_spans;
    // ---- the registers: group g takes the spans g, g + 8, ...
    {
        const uint32_t r = threadIdx.x & 31, g = threadIdx.x >> 5;
        unsigned long long n = 0, first = NONE, last1 = 0, write1 = 0;
        for (uint32_t s = g; s < n_used; s += 8) {
            const unsigned long long kb = spans[s].k_base;
            const DivergeSpanRegs &sr = span_regs[s];
            const uint32_t f = sr.first_diff[r], l1 = sr.last_diff1[r], w1 = sr.last_write1[r];
            n += sr.n_diff[r];
            if (f != NONE32 && kb + f < first) first = kb + f;
            if (l1 && kb + l1 > last1) last1 = kb + l1;
            if (w1 && kb + w1 > write1) write1 = kb + w1;
        }
        g_n[g][r] = n; g_first[g][r] = first; g_last1[g][r] = last1; g_write1[g][r] = write1;
    }
    __syncthreads();
    if (threadIdx.x < 32) {
        const uint32_t r = threadIdx.x;
        unsigned long long n = 0, first = NONE, last1 = 0, write1 = 0;
        for (uint32_t g = 0; g < 8; g++) {
            n += g_n[g][r];
            first = g_first[g][r] < first ? g_first[g][r] : first;
            last1 = g_last1[g][r] > last1 ? g_last1[g][r] : last1;
            write1 = g_write1[g][r] > write1 ? g_write1[g][r] : write1;
        }
        out->reg_n_diff[r] = n; out->reg_first_diff[r] = first;
        out->reg_last_diff[r] = last1 ? last1 - 1 : NONE; out->reg_last_write[r] = write1 ? write1 - 1 : NONE;
    }
    // ---- the counts and the rank bases: wave 0, 64 spans per step, an inclusive scan by __shfl_up and a carried base
    if (threadIdx.x >= 64) return;   // (no barrier follows)
    const uint32_t lane = threadIdx.x;
    unsigned long long carry = 0, first = NONE, last1 = 0, n_load = 0, n_store = 0;
    uint32_t mask = 0;
    for (uint32_t s0 = 0; s0 < n_used; s0 += 64) {   // (wave-uniform bounds: every lane takes part in the shuffles)
        const uint32_t s = s0 + lane;
        uint32_t v = 0;
        if (s < n_used) {
            const DivergeSpan sp = spans[s];
            v = sp.n_data;
            if (v) {
                if (sp.k_base + sp.first_data < first) first = sp.k_base + sp.first_data;
                if (sp.k_base + sp.last_data + 1 > last1) last1 = sp.k_base + sp.last_data + 1;
            }
            mask |= sp.mask; n_load += sp.n_load; n_store += sp.n_store;
        }
        uint32_t inc = v;
        for (uint32_t dlt = 1; dlt < 64; dlt <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)inc, dlt);
            if (lane >= dlt) inc += t;
        }
        if (s < n_used) rank_base[s] = carry + inc - v;
        carry += (uint32_t)__shfl((int)inc, 63);
    }
    for (uint32_t dlt = 32; dlt; dlt >>= 1) {
        const unsigned long long f = __shfl_xor(first, dlt), l = __shfl_xor(last1, dlt);
        first = f < first ? f : first;
        last1 = l > last1 ? l : last1;
        n_load += __shfl_xor(n_load, dlt);
        n_store += __shfl_xor(n_store, dlt);
        mask |= (uint32_t)__shfl_xor((int)mask, dlt);
    }
    if (lane == 0) {
        out->stop = n_used ? spans[n_used - 1].k_base + spans[n_used - 1].stop : 0;
        out->stopped = first_stop < n_spans ? spans[first_stop].stopped : 0;
        out->n_data = carry; out->first_data = first; out->last_data = last1 ? last1 - 1 : NONE;
        out->n_load = n_load; out->n_store = n_store; out->mask = mask; out->n_used = n_used; out->pad = 0;
    }
}

__global__ void __launch_bounds__(256) diverge_emit_kernel(const DivergeArgs a, const DivergeSpan *spans, const unsigned long long *rank_base,
                                                           const DivergeMerged *merged, uint32_t cap_spans, uint32_t K, dvt_diverge_pair *first,
                                                           dvt_diverge_pair *last) {
    __shared__ uint32_t unit[UNITS];
    const uint32_t span = a.span0 + blockIdx.x;
    if (span >= cap_spans || span >= merged->n_used) return;   // (the whole workgroup, before any barrier; so are the next two)
    const uint32_t n = spans[span].n_data, stop = spans[span].stop;
    const unsigned long long lo = rank_base[span], hi = lo + n;
    const watch::Keep keep = watch::keep_of(merged->n_data, K);
    if (!n || !(lo < keep.first_end || hi > keep.last_begin)) return;
    const uint32_t base = blockIdx.x * diverge::SPAN, wave = threadIdx.x >> 6;
    const bool lane0 = (threadIdx.x & 63) == 0;
    uint32_t bits = 0;
#pragma unroll
    for (uint32_t k = 0; k < ROUNDS; k++) {   // (every thread runs every round: the ballots need all lanes)
        const uint32_t local = k * 256 + threadIdx.x;
        const bool data = local < stop && (class_of(a, base + local) & diverge::C_MASK);
        bits |= (uint32_t)data << k;
        const unsigned long long b = __ballot(data);
        if (lane0) unit[4 * k + wave] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (uint32_t u = 0; u < UNITS; u++) {
            const uint32_t c = unit[u];
            unit[u] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < ROUNDS; k++) {
        const uint32_t local = k * 256 + threadIdx.x;
        const bool hit = (bits >> k) & 1;
        const unsigned long long b = __ballot(hit);   // (all lanes of the wave: nothing above diverges)
        const unsigned long long rank = lo + unit[4 * k + wave] + lanes_below(b);
        const bool in_first = rank < keep.first_end && rank < K, in_last = rank >= keep.last_begin && rank - keep.last_begin < K;
        if (!hit || !(in_first || in_last) || base + local >= a.n_pairs) continue;   // (the next round's ballot is where the wave meets again)
        const rv32::CycleRec ra = read_record(a.rec_a, base + local), rb = read_record(a.rec_b, base + local);
        const watch::Decoded da = watch::decode(ra, a.n_instr, a.text_base, a.statics, a.offs, a.sh);
        const watch::Decoded db = watch::decode(rb, a.n_instr, a.text_base, a.statics, a.offs, a.sh);
        const uint32_t w = diverge::classify(ra, rb, da, db);
        const dvt_diverge_pair e = diverge::make_pair(a.k0 + base + local, w & diverge::C_MASK, ra, rb, da, db, a.shard_a, a.row_a + base + local, a.shard_b,
                                                      a.row_b + base + local);
        if (in_first) first[rank] = e;
        if (in_last) last[rank - keep.last_begin] = e;
    }
}

bool args_ok(const DivergeArgs &a) {
    return a.n_instr && a.statics && a.offs && a.rec_a && a.rec_b && a.sh.n <= memrep::MAX_PRE && a.n_pairs &&
           (unsigned long long)a.span0 + (a.n_pairs + diverge::SPAN - 1) / diverge::SPAN <= 0xffffffffull;
}

}  // namespace

hipError_t launch_diverge_classify(hipStream_t st, const DivergeArgs &a, DivergeSpan *d_spans, DivergeSpanRegs *d_span_regs, uint32_t cap_spans,
                                   unsigned long long *d_stop_flag) {
    if (!a.n_pairs) return hipSuccess;
    if (!args_ok(a) || !d_spans || !d_span_regs || !d_stop_flag || a.span0 + (a.n_pairs + diverge::SPAN - 1) / diverge::SPAN > cap_spans) return hipErrorInvalidValue;
    diverge_classify_kernel<<<(a.n_pairs + diverge::SPAN - 1) / diverge::SPAN, 256, 0, st>>>(a, d_spans, d_span_regs, cap_spans, d_stop_flag);
    return hipGetLastError();
}

hipError_t launch_diverge_merge(hipStream_t st, const DivergeSpan *d_spans, const DivergeSpanRegs *d_span_regs, uint32_t n_spans, unsigned long long *d_rank_base,
                                DivergeMerged *d_out) {
    if (!d_spans || !d_span_regs || !d_rank_base || !d_out) return hipErrorInvalidValue;
    diverge_merge_kernel<<<1, 256, 0, st>>>(d_spans, d_span_regs, n_spans, d_rank_base, d_out);
    return hipGetLastError();
}

hipError_t launch_diverge_emit(hipStream_t st, const DivergeArgs &a, const DivergeSpan *d_spans, const unsigned long long *d_rank_base, const DivergeMerged *d_merged,
                               uint32_t cap_spans, uint32_t K, void *d_first, void *d_last) {
    if (!a.n_pairs) return hipSuccess;
    if (!args_ok(a) || !d_spans || !d_rank_base || !d_merged || !d_first || !d_last || K < 1 || K > diverge::MAX_KEEP) return hipErrorInvalidValue;
    diverge_emit_kernel<<<(a.n_pairs + diverge::SPAN - 1) / diverge::SPAN, 256, 0, st>>>(a, d_spans, d_rank_base, d_merged, cap_spans, K, static_cast<dvt_diverge_pair *>(d_first),
                                                                                              static_cast<dvt_diverge_pair *>(d_last));
    return hipGetLastError();
}

}  // namespace dvt
