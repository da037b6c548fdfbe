// The device passes of the origin search (origin.h) over the cycle records a prepared job holds in HBM: reduce and gather.
//
// The launch shape of snapshot.hip: 256 threads, a fixed span of DVT_ORIGIN_SPAN = 4096 consecutive records of one shard per
// workgroup, 16 rounds of 256; a thread reads the first and the third 16-byte word of its record and decodes it with
// watch::decode, the function the host path runs.
//   reduce   answers up to DVT_ORIGIN_PASS_QUESTIONS = 256 questions "the last record before Q that writes the target" in one
//            pass.  The host sorts them (origin::sorts_before) and sends the 33 offsets of the register questions.  The
//            questions (target u32, Q u64; stage_pass, records.cuh) and one u32 slot per question are in LDS, 4 KB.  A workgroup whose first
//            position is at or after the largest Q leaves after the staging barrier (all of it: there is no barrier behind);
//            the host launches no span past that position at all.  For every target the record writes (flow::for_written,
//            dataflow.h): a register k walks the questions of register k from the largest Q down and stops at the first that
//            lies at or before the record; a word finds its questions by binary search (first_word, records.cuh) and walks
//            the equal run; a call has at most 72 written words.
//            A record before Q offers atomicMax(slot, its number in the span + 1).  After the barrier one 64-bit global
//            atomicMax per touched slot: a loop that writes one register costs one global atomic per span, not per record.
//            Bad records before the largest Q are counted.  No lane returns before a barrier.
//   gather   one lane per OriginFetch copies the 12 words of its record out; an item outside its shard gives all ones, which
//            decodes as bad.
// Every loop is bounded by the launch, by the 72 words of a call, by the 256 questions or by the depth of the binary search;
// every index is checked before the store.
#include "kernels.h"
#include "origin.h"
#include "records.cuh"

namespace dvt {

namespace {

constexpr uint32_t ROUNDS = origin::SPAN / 256, PASS_Q = origin::PASS_Q;
static_assert(PASS_Q == 256, "one question per thread of the staging round");

__global__ void __launch_bounds__(256) origin_reduce_kernel(const rv32::CycleRec *recs, size_t n_take, const OriginArgs a, unsigned long long *win,
                                                            unsigned long long *bad_records) {
    __shared__ unsigned long long q_pos[PASS_Q];
    __shared__ uint32_t q_target[PASS_Q], slot[PASS_Q], reg_off[33], wg_bad;
    slot[threadIdx.x] = 0;   // (blockDim.x == PASS_Q)
    if (threadIdx.x == 0) wg_bad = 0;
    const uint32_t n_q = stage_pass(a, q_pos, q_target, reg_off);
    const size_t base = (size_t)blockIdx.x * origin::SPAN;
    if (watch::position(a.shard, (uint32_t)base) >= a.max_q) return;   // (the whole workgroup, and no barrier follows for it)
    const uint32_t words_lo = reg_off[32];
    for (uint32_t k = 0; k < ROUNDS; k++) {
        const uint32_t local = k * 256 + threadIdx.x;
        const size_t r = base + local;
        const rv32::CycleRec rec = read_record(recs, r, n_take);
        const watch::Decoded d = watch::decode(rec, a.n_instr, a.text_base, a.statics, a.offs, a.sh);
        if (r >= n_take) continue;   // (no barrier inside the loop)
        const unsigned long long pos = watch::position(a.shard, (uint32_t)r);
        if (pos >= a.max_q) continue;
        if (d.bad) { atomicAdd(&wg_bad, 1u); continue; }
        flow::for_written(d, a.sh, words_lo < n_q, [&](uint32_t what, uint32_t t) {
            if (what == DVT_ORIGIN_REG) {   // (t < 32; sorted by Q: the questions the record lies before are a suffix)
                const uint32_t first = reg_off[t];
                for (uint32_t q = reg_off[t + 1]; q > first; q--) {
                    if (pos >= q_pos[q - 1]) break;
                    atomicMax(&slot[q - 1], local + 1);
                }
            } else {   // every question of word t the record answers: the run of equal targets
                for (uint32_t q = first_word(q_target, words_lo, n_q, t); q < n_q && q_target[q] == t; q++)
                    if (pos < q_pos[q]) atomicMax(&slot[q], local + 1);
            }
        });
    }
    __syncthreads();
    if (threadIdx.x < n_q && slot[threadIdx.x]) atomicMax(&win[threadIdx.x], watch::position(a.shard, (uint32_t)(base + slot[threadIdx.x] - 1)));
    if (threadIdx.x == 0 && wg_bad) atomicAdd(bad_records, (unsigned long long)wg_bad);
}

__global__ void __launch_bounds__(256) origin_gather_kernel(const OriginFetch *items, uint32_t n_items, rv32::CycleRec *out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_items) return;   // (no barrier in this kernel)
    const OriginFetch it = items[i];
    uint4 w0 = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu), w1 = w0, w2 = w0;
    if (it.recs && it.row < it.n_recs) {
        const uint4 *p = reinterpret_cast<const uint4 *>(&it.recs[it.row]);
        w0 = p[0]; w1 = p[1]; w2 = p[2];
    }
    uint4 *o = reinterpret_cast<uint4 *>(&out[i]);
    o[0] = w0; o[1] = w1; o[2] = w2;
}

}  // namespace

hipError_t launch_origin_reduce(hipStream_t st, const rv32::CycleRec *d_recs, size_t n_take, const OriginArgs &a, unsigned long long *d_win,
                                unsigned long long *d_bad_records) {
    if (!n_take) return hipSuccess;
    if (!pass_ok(a) || !d_recs || !d_win || !d_bad_records || n_take > 0xffffffffull) return hipErrorInvalidValue;
    origin_reduce_kernel<<<(unsigned)((n_take + origin::SPAN - 1) / origin::SPAN), 256, 0, st>>>(d_recs, n_take, a, d_win, d_bad_records);
    return hipGetLastError();
}

hipError_t launch_origin_gather(hipStream_t st, const OriginFetch *d_items, uint32_t n_items, rv32::CycleRec *d_out) {
    if (!n_items) return hipSuccess;
    if (!d_items || !d_out) return hipErrorInvalidValue;
    origin_gather_kernel<<<(n_items + 255) / 256, 256, 0, st>>>(d_items, n_items, d_out);
    return hipGetLastError();
}

}  // namespace dvt
