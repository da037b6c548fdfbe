// The device passes of the uses search (uses.h) over the cycle records a prepared job holds in HBM: next, count, scan and emit
// (the consumers' records come out by origin.hip's gather).
//
// The launch shape of origin.hip: 256 threads, a fixed span of DVT_USES_SPAN = 4096 consecutive records of one shard per
// workgroup, 16 rounds of 256; a thread reads the first and the third 16-byte word of its record and decodes it with
// watch::decode, the function the host path runs.  A pass takes up to DVT_USES_PASS_DEFS = 256 definitions, sorted by the host
// (origin::sorts_before) with the 33 offsets of the register definitions; targets, F (stage_pass, records.cuh) and N are staged in
// LDS.  What a record writes and reads comes from flow::for_written and flow::for_read (dataflow.h).
//   next    one u32 LDS slot per definition holds the SMALLEST number in the span of a record at or after F that writes the
//           target.  A written register k walks the definitions of register k from the smallest F up and stops at the first that
//           begins after the record; a written word finds its definitions by binary search and walks the equal run; a call
//           has at most 72 written words.  After the barrier one 64-bit global
//           atomicMin per touched slot.  The host launches no span before the smallest F; bad records at or after it are counted.
//   count   with the windows [F, N] known: per span and definition the number of uses, counted in LDS.  A record finds the
//           definitions of the registers it reads by the register offsets and of the words it reads by binary search, walks the
//           run of equal targets and tests the window.  The workgroup writes its 256 counts as one row of the member's count
//           table: no global atomic at all.  Only the spans that intersect [min F, max N] are launched.
//   scan    one workgroup per shard, launched in execution order on one stream, one lane per definition: walks the shard's
//           launched spans in order (16 rows in flight), carrying the member's running count per definition from shard to shard in global memory,
//           and appends (span, def, rank before the span) for every span that holds a rank below fan: at most 256 x fan items
//           per member and pass, one global atomic each.
//   emit    one workgroup per item over a fixed grid; workgroups past the list's length return at once.  Each ranks its
//           definition's uses inside the span in execution order, round by round, by ballot prefixes (a record holds 0, 1 or 2
//           uses of one definition: two ballots), and writes position and role of the ranks below fan.
// Every loop is bounded by the launch, by the 72 words of a call, by the 256 definitions or by the depth of the binary search;
// every index is checked before the store; no lane leaves before a barrier its workgroup still meets.
#include "kernels.h"
#include "records.cuh"
#include "uses.h"

namespace dvt {

namespace {

constexpr uint32_t ROUNDS = uses::SPAN / 256, PASS_D = uses::PASS_DEFS;
static_assert(PASS_D == 256, "one definition per thread of the staging round");

__global__ void __launch_bounds__(256) uses_next_kernel(const rv32::CycleRec *recs, size_t n_recs, uint32_t first_span, const UsesArgs a,
                                                        unsigned long long *win, unsigned long long *bad_records) {
    __shared__ unsigned long long d_from[PASS_D];
    __shared__ uint32_t d_target[PASS_D], slot[PASS_D], reg_off[33], wg_bad;
    slot[threadIdx.x] = 0xffffffffu;   // (blockDim.x == PASS_D)
    if (threadIdx.x == 0) wg_bad = 0;
    const uint32_t n_d = stage_pass(a, d_from, d_target, reg_off);
    const size_t base = ((size_t)first_span + blockIdx.x) * uses::SPAN;
    const uint32_t words_lo = reg_off[32];
    for (uint32_t k = 0; k < ROUNDS; k++) {
        const uint32_t local = k * 256 + threadIdx.x;
        const size_t r = base + local;
        const rv32::CycleRec rec = read_record(recs, r, n_recs);
        const watch::Decoded d = watch::decode(rec, a.n_instr, a.text_base, a.statics, a.offs, a.sh);
        if (r >= n_recs) continue;   // (no barrier inside the loop)
        const unsigned long long pos = watch::position(a.shard, (uint32_t)r);
        if (pos < a.min_from) continue;
        if (d.bad) { atomicAdd(&wg_bad, 1u); continue; }
        flow::for_written(d, a.sh, words_lo < n_d, [&](uint32_t what, uint32_t t) {
            if (what == DVT_USES_REG) {   // (t < 32; sorted by F: the definitions that began at or before the record are a prefix)
                const uint32_t end = reg_off[t + 1];
                for (uint32_t q = reg_off[t]; q < end; q++) {
                    if (d_from[q] > pos) break;
                    atomicMin(&slot[q], local);
                }
            } else {   // every definition of word t that began at or before the record: the run of equal targets
                for (uint32_t q = first_word(d_target, words_lo, n_d, t); q < n_d && d_target[q] == t; q++)
                    if (d_from[q] <= pos) atomicMin(&slot[q], local);
            }
        });
    }
    __syncthreads();
    if (threadIdx.x < n_d && slot[threadIdx.x] != 0xffffffffu) atomicMin(&win[threadIdx.x], watch::position(a.shard, (uint32_t)(base + slot[threadIdx.x])));
    if (threadIdx.x == 0 && wg_bad) atomicAdd(bad_records, (unsigned long long)wg_bad);
}

__global__ void __launch_bounds__(256) uses_count_kernel(const rv32::CycleRec *recs, size_t n_recs, uint32_t first_span, const UsesArgs a, uint32_t *table,
                                                         size_t table_row, size_t table_rows) {
    __shared__ unsigned long long d_from[PASS_D], d_next[PASS_D];
    __shared__ uint32_t d_target[PASS_D], cnt[PASS_D], reg_off[33];
    if (threadIdx.x < a.n) d_next[threadIdx.x] = a.d_next[threadIdx.x];   // (blockDim.x == PASS_D)
    cnt[threadIdx.x] = 0;
    const uint32_t n_d = stage_pass(a, d_from, d_target, reg_off);
    const size_t base = ((size_t)first_span + blockIdx.x) * uses::SPAN;
    const uint32_t words_lo = reg_off[32];
    for (uint32_t k = 0; k < ROUNDS; k++) {
        const size_t r = base + k * 256 + threadIdx.x;
        const rv32::CycleRec rec = read_record(recs, r, n_recs);
        const watch::Decoded d = watch::decode(rec, a.n_instr, a.text_base, a.statics, a.offs, a.sh);
        if (r >= n_recs || d.bad) continue;   // (no barrier inside the loop; d.bad: rec.idx >= n_instr among others)
        const unsigned long long pos = watch::position(a.shard, (uint32_t)r);
        if (pos < a.min_from || pos > a.max_next) continue;
        flow::for_read(d, a.ostat[rec.idx], a.sh, a.flags, words_lo < n_d, [&](uint32_t, uint32_t what, uint32_t t) {
            if (what == DVT_USES_REG) {   // (t < 32) the definitions of register t whose window holds pos
                const uint32_t end = reg_off[t + 1];
                for (uint32_t q = reg_off[t]; q < end; q++) {
                    if (d_from[q] > pos) break;
                    if (pos <= d_next[q]) atomicAdd(&cnt[q], 1u);
                }
            } else {
                for (uint32_t q = first_word(d_target, words_lo, n_d, t); q < n_d && d_target[q] == t; q++)
                    if (d_from[q] <= pos && pos <= d_next[q]) atomicAdd(&cnt[q], 1u);
            }
        });
    }
    __syncthreads();
    const size_t row = table_row + blockIdx.x;
    if (row < table_rows) table[row * PASS_D + threadIdx.x] = cnt[threadIdx.x];
}

__global__ void __launch_bounds__(256) uses_scan_kernel(const uint32_t *table, size_t table_row, uint32_t n_spans, size_t table_rows, const rv32::CycleRec *recs,
                                                        uint32_t n_recs, uint32_t shard, uint32_t first_span, uint32_t n_d, uint32_t fan,
                                                        unsigned long long *carry, UsesItem *items, uint32_t *n_items, uint32_t cap_items) {
    const uint32_t i = threadIdx.x;
    if (i >= n_d || i >= PASS_D) return;   // (no barrier in this kernel)
    unsigned long long run = carry[i];
    constexpr uint32_t BATCH = 16;   // rows in flight: the walk is one dependent chain, its loads need not be
    for (uint32_t s0 = 0; s0 < n_spans; s0 += BATCH) {
        uint32_t c[BATCH];
#pragma unroll
        for (uint32_t k = 0; k < BATCH; k++) c[k] = s0 + k < n_spans && table_row + s0 + k < table_rows ? table[(table_row + s0 + k) * PASS_D + i] : 0;
#pragma unroll
        for (uint32_t k = 0; k < BATCH; k++) {
            if (c[k] && run < fan) {
                const uint32_t at = atomicAdd(n_items, 1u);
                if (at < cap_items) items[at] = UsesItem{recs, n_recs, shard, first_span + s0 + k, i, (uint32_t)run, 0};
            }
            run += c[k];
        }
    }
    carry[i] = run;
}

__global__ void __launch_bounds__(256) uses_emit_kernel(const UsesItem *items, const uint32_t *n_items, uint32_t cap_items, const UsesArgs a,
                                                        unsigned long long *out_pos, uint32_t *out_role) {
    __shared__ uint32_t wave_total[4];
    const uint32_t n = *n_items < cap_items ? *n_items : cap_items;
    if (blockIdx.x >= n) return;   // (the whole workgroup, before any barrier)
    const UsesItem it = items[blockIdx.x];
    if (it.def >= a.n || it.def >= PASS_D || !it.recs) return;   // (uniform)
    const uint32_t what = it.def < a.reg_off[32] ? DVT_USES_REG : DVT_USES_WORD, target = a.target[it.def];
    const unsigned long long from = a.pos[it.def], next = a.d_next[it.def];
    const uint32_t wave = threadIdx.x >> 6;
    const size_t base = (size_t)it.span * uses::SPAN;
    uint32_t running = it.rank;
    for (uint32_t k = 0; k < ROUNDS && running < a.fan; k++) {   // (running is uniform: every thread runs the same rounds)
        const size_t r = base + k * 256 + threadIdx.x;
        const rv32::CycleRec rec = read_record(it.recs, r, it.n_recs);
        const watch::Decoded d = watch::decode(rec, a.n_instr, a.text_base, a.statics, a.offs, a.sh);
        const unsigned long long pos = watch::position(it.shard, (uint32_t)r);
        uses::Reads rd{0, 0, 0};
        if (r < it.n_recs && !d.bad && pos >= from && pos <= next) rd = uses::reads(d, a.ostat[rec.idx], a.sh, what, target, a.flags);
        const unsigned long long b1 = __ballot(rd.n >= 1), b2 = __ballot(rd.n >= 2);
        if ((threadIdx.x & 63) == 0) wave_total[wave] = (uint32_t)(__popcll(b1) + __popcll(b2));
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < 4; w++) {
            if (w < wave) before += wave_total[w];
            total += wave_total[w];
        }
        const uint32_t rank = running + before + lanes_below(b1) + lanes_below(b2);
        if (rd.n >= 1 && rank < a.fan) {
            out_pos[(size_t)it.def * a.fan + rank] = pos;
            out_role[(size_t)it.def * a.fan + rank] = rd.role0;
        }
        if (rd.n >= 2 && rank + 1 < a.fan) {
            out_pos[(size_t)it.def * a.fan + rank + 1] = pos;
            out_role[(size_t)it.def * a.fan + rank + 1] = rd.role1;
        }
        running += total;
        __syncthreads();   // (wave_total is written again in the next round)
    }
}

bool args_ok(const UsesArgs &a, bool windows) {
    return pass_ok(a) && a.ostat && (!windows || (a.d_next && a.fan && a.fan <= uses::MAX_FAN));
}

// the spans [first_span, first_span + n_spans) lie in a shard of n_recs records
bool spans_ok(size_t n_recs, uint32_t first_span, uint32_t n_spans) {
    return n_recs <= 0xffffffffull && (size_t)first_span + n_spans <= (n_recs + uses::SPAN - 1) / uses::SPAN;
}

}  // namespace

hipError_t launch_uses_next(hipStream_t st, const rv32::CycleRec *d_recs, size_t n_recs, uint32_t first_span, uint32_t n_spans, const UsesArgs &a,
                            unsigned long long *d_win, unsigned long long *d_bad_records) {
    if (!n_spans) return hipSuccess;
    if (!args_ok(a, false) || !d_recs || !d_win || !d_bad_records || !spans_ok(n_recs, first_span, n_spans)) return hipErrorInvalidValue;
    uses_next_kernel<<<n_spans, 256, 0, st>>>(d_recs, n_recs, first_span, a, d_win, d_bad_records);
    return hipGetLastError();
}

hipError_t launch_uses_count(hipStream_t st, const rv32::CycleRec *d_recs, size_t n_recs, uint32_t first_span, uint32_t n_spans, const UsesArgs &a,
                             uint32_t *d_table, size_t table_row, size_t table_rows) {
    if (!n_spans) return hipSuccess;
    if (!args_ok(a, true) || !d_recs || !d_table || !spans_ok(n_recs, first_span, n_spans) || table_row + n_spans > table_rows) return hipErrorInvalidValue;
    uses_count_kernel<<<n_spans, 256, 0, st>>>(d_recs, n_recs, first_span, a, d_table, table_row, table_rows);
    return hipGetLastError();
}

hipError_t launch_uses_scan(hipStream_t st, const uint32_t *d_table, size_t table_row, uint32_t n_spans, size_t table_rows, const rv32::CycleRec *d_recs,
                            size_t n_recs, uint32_t shard, uint32_t first_span, uint32_t n_d, uint32_t fan, unsigned long long *d_carry, UsesItem *d_items,
                            uint32_t *d_n_items, uint32_t cap_items) {
    if (!n_spans) return hipSuccess;
    if (!d_table || !d_recs || !d_carry || !d_items || !d_n_items || !n_d || n_d > PASS_D || !fan || fan > uses::MAX_FAN ||
        !spans_ok(n_recs, first_span, n_spans) || table_row + n_spans > table_rows)
        return hipErrorInvalidValue;
    uses_scan_kernel<<<1, 256, 0, st>>>(d_table, table_row, n_spans, table_rows, d_recs, (uint32_t)n_recs, shard, first_span, n_d, fan, d_carry, d_items,
                                        d_n_items, cap_items);
    return hipGetLastError();
}

hipError_t launch_uses_emit(hipStream_t st, const UsesItem *d_items, const uint32_t *d_n_items, uint32_t cap_items, const UsesArgs &a,
                            unsigned long long *d_out_pos, uint32_t *d_out_role) {
    if (!cap_items) return hipSuccess;
    if (!args_ok(a, true) || !d_items || !d_n_items || !d_out_pos || !d_out_role || cap_items > PASS_D * uses::MAX_FAN) return hipErrorInvalidValue;
    uses_emit_kernel<<<cap_items, 256, 0, st>>>(d_items, d_n_items, cap_items, a, d_out_pos, d_out_role);
    return hipGetLastError();
}

}  // namespace dvt
