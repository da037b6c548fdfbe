// The device passes of the origin search (origin.h) over the cycle records a prepared job holds in HBM: reduce and gather.
//
// The launch shape of snapshot.hip: 256 threads, a fixed span of DVT_ORIGIN_SPAN = 4096 consecutive records of one shard per
// workgroup, 16 rounds of 256; a thread reads the first and the third 16-byte word of its record and decodes it with
// watch::decode, the function the host path runs.
//   reduce   answers up to DVT_ORIGIN_PASS_QUESTIONS = 256 questions "the last record before Q that writes the target" in one
//            pass.  The host sorts them (origin::sorts_before) and sends the 33 offsets of the register questions.  The
//            questions (target u32, Q u64) and one u32 slot per question are staged in LDS, 4 KB.  A workgroup whose first
//            position is at or after the largest Q leaves after the staging barrier (all of it: there is no barrier behind);
//            the host launches no span past that position at all.  A record with rd = k walks the questions of register k
//            from the largest Q down and stops at the first that lies at or before it; a store finds the questions of its
//            word by binary search and walks the equal run; a call does the same for each of its at most 72 written words.
//            A record before Q offers atomicMax(slot, its number in the span + 1).  After the barrier one 64-bit global
//            atomicMax per touched slot: a loop that writes one register costs one global atomic per span, not per record.
//            Bad records before the largest Q are counted.  No lane returns before a barrier.
//   gather   one lane per OriginFetch copies the 12 words of its record out; an item outside its shard gives all ones, which
//            decodes as bad.
// Every loop is bounded by the launch, by the 72 words of a call, by the 256 questions or by the depth of the binary search;
// every index is checked before the store.
#include "kernels.h"
#include "origin.h"

namespace dvt {

namespace {

constexpr uint32_t ROUNDS = origin::SPAN / 256, PASS_Q = origin::PASS_Q;
static_assert(PASS_Q == 256, "one question per thread of the staging round");

// the record at r, or one that decodes as bad for a lane past the end (the words decode() reads)
__device__ __forceinline__ rv32::CycleRec read_record(const rv32::CycleRec *recs, size_t r, size_t n_recs) {
    rv32::CycleRec rec{};
    rec.idx = 0xffffffffu;
    if (r < n_recs) {
        const uint4 *p = reinterpret_cast<const uint4 *>(&recs[r]);
        const uint4 w0 = p[0], w2 = p[2];
        rec.idx = w0.x; rec.a = w0.y; rec.b = w0.z; rec.c = w0.w;
        rec.m_prev = w2.x; rec.m_ts = w2.y; rec.sh_ab = w2.z; rec.sh_cm = w2.w;
    }
    return rec;
}

__global__ void __launch_bounds__(256) origin_reduce_kernel(const rv32::CycleRec *recs, size_t n_take, const OriginArgs a, unsigned long long *win,
                                                            unsigned long long *bad_records) {
    __shared__ unsigned long long q_pos[PASS_Q];
    __shared__ uint32_t q_target[PASS_Q], slot[PASS_Q], reg_off[33], wg_bad;
    const uint32_t n_q = a.n_q < PASS_Q ? a.n_q : PASS_Q;
    if (threadIdx.x < n_q) { q_pos[threadIdx.x] = a.q_pos[threadIdx.x]; q_target[threadIdx.x] = a.q_target[threadIdx.x]; }
    slot[threadIdx.x] = 0;   // (blockDim.x == PASS_Q)
    if (threadIdx.x < 33) reg_off[threadIdx.x] = a.reg_off[threadIdx.x] < n_q ? a.reg_off[threadIdx.x] : n_q;
    if (threadIdx.x == 0) wg_bad = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * origin::SPAN;
    if (watch::position(a.shard, (uint32_t)base) >= a.max_q) return;   // (the whole workgroup, and no barrier follows for it)
    const uint32_t words_lo = reg_off[32];
    // every question of word `addr` the record at `pos` answers: the run of equal targets among the word questions
    auto offer_word = [&](uint32_t addr, unsigned long long pos, uint32_t local) {
        uint32_t lo = words_lo, hi = n_q;
        while (lo < hi) {   // (at most 9 steps: the first question with target >= addr)
            const uint32_t mid = (lo + hi) / 2;
            if (q_target[mid] < addr) lo = mid + 1;
            else hi = mid;
        }
        for (uint32_t q = lo; q < n_q && q_target[q] == addr; q++)
            if (pos < q_pos[q]) atomicMax(&slot[q], local + 1);
    };
    for (uint32_t k = 0; k < ROUNDS; k++) {
        const uint32_t local = k * 256 + threadIdx.x;
        const size_t r = base + local;
        const rv32::CycleRec rec = read_record(recs, r, n_take);
        const watch::Decoded d = watch::decode(rec, a.n_instr, a.text_base, a.statics, a.offs, a.sh);
        if (r >= n_take) continue;   // (no barrier inside the loop)
        const unsigned long long pos = watch::position(a.shard, (uint32_t)r);
        if (pos >= a.max_q) continue;
        if (d.bad) { atomicAdd(&wg_bad, 1u); continue; }
        const uint32_t rd = d.st & watch::ST_RD_MASK;   // < 32
        if (rd) {
            const uint32_t first = reg_off[rd], end = reg_off[rd + 1] < n_q ? reg_off[rd + 1] : n_q;
            for (uint32_t q = end; q > first; q--) {   // (sorted by Q: the questions the record lies before are a suffix)
                if (pos >= q_pos[q - 1]) break;
                atomicMax(&slot[q - 1], local + 1);
            }
        }
        if (words_lo >= n_q) continue;
        if (d.dir == DVT_WATCH_STORE) offer_word(d.addr, pos, local);
        else if (!d.dir && d.shape >= 0 && d.shape < (int)memrep::MAX_PRE) {
            const memrep::PreShape &s = a.sh.s[d.shape];
            for (uint32_t arr = 0; arr < 2; arr++) {
                const uint32_t ab = arr ? d.a1 : d.a0, n = arr ? s.n1 : s.n0, w = arr ? s.w1 : s.w0;
                for (uint32_t i = 0; i < n && i < memrep::MAX_CALL_WORDS; i++)
                    if (i + w >= n) offer_word(ab + 4 * i, pos, local);
            }
        }
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

bool args_ok(const OriginArgs &a) {
    if (!a.n_instr || !a.statics || !a.offs || a.sh.n > memrep::MAX_PRE || !a.n_q || a.n_q > PASS_Q || !a.q_target || !a.q_pos) return false;
    if (a.reg_off[0] != 0) return false;
    for (uint32_t k = 0; k < 32; k++)
        if (a.reg_off[k] > a.reg_off[k + 1]) return false;
    return a.reg_off[32] <= a.n_q;
}

}  // namespace

hipError_t launch_origin_reduce(hipStream_t st, const rv32::CycleRec *d_recs, size_t n_take, const OriginArgs &a, unsigned long long *d_win,
                                unsigned long long *d_bad_records) {
    if (!n_take) return hipSuccess;
    if (!args_ok(a) || !d_recs || !d_win || !d_bad_records || n_take > 0xffffffffull) return hipErrorInvalidValue;
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
