// The snapshot's device passes (snapshot.h) over the cycle records a prepared job holds in HBM: reduce and gather.  (The
// backtrace is the call-tree pass in summary mode over the records before the position, calltree.hip.)
//
// The launch shape of watch.hip: 256 threads, a fixed span of DVT_SNAP_SPAN = 4096 consecutive records of one shard per
// workgroup, 16 rounds of 256.  The ranges and the precompile shapes travel as kernel arguments; a thread reads the first and
// the third 16-byte word of its record and decodes it with watch::decode, the function the host path runs.
//   reduce   every record offers its position to three kinds of slot: register rd and, with for_decided(), every watched word
//            it decides; before the position P the LATEST offer wins (max), at or after P the EARLIEST (min).  The offers of a
//            span meet in LDS first: a position inside a span is its record's number 0 .. 4095, so a u32 per slot holds it
//            (before side and registers: number + 1, 0 = nobody; after side: the number, all ones = nobody), two tables of
//            4096 slots and 32 register slots, 33 KB.  After the barrier the workgroup flushes one 64-bit atomicMax /
//            atomicMin per slot somebody touched: a guest that hammers one word costs one global atomic per span, not per
//            record.  Bad records are counted.  No lane returns before the barriers.
//   gather   one lane per SnapFetch: the record at (shard, row) is read by its position, decoded again and turned into the
//            snap::Side the host asked for (side_of()); a row outside the shard or a record that is not what the winner tables
//            said gives SIDE_BAD.
// Every loop is bounded by the launch, by the 72 words of a call or by the table sizes; every index is checked before the
// store.
#include "kernels.h"
#include "records.cuh"
#include "snapshot.h"

namespace dvt {

namespace {

constexpr uint32_t ROUNDS = snap::SPAN / 256, NOBODY = 0xffffffffu;
static_assert(snap::SPAN <= (1u << 13), "a position inside a span fits 13 bits");

__global__ void __launch_bounds__(256) snap_reduce_kernel(const rv32::CycleRec *recs, size_t n_recs, const SnapArgs a, const SnapTables t) {
    __shared__ uint32_t bef[snap::MAX_WORDS], aft[snap::MAX_WORDS], reg[32], wg_bad;
    const uint32_t n_words = a.rg.n_words < snap::MAX_WORDS ? a.rg.n_words : snap::MAX_WORDS;   // (every slot of a range lies below it: args_ok)
    for (uint32_t s = threadIdx.x; s < n_words; s += 256) { bef[s] = 0; aft[s] = NOBODY; }
    if (threadIdx.x < 32) reg[threadIdx.x] = 0;
    if (threadIdx.x == 0) wg_bad = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * snap::SPAN;
    for (uint32_t k = 0; k < ROUNDS; k++) {
        const uint32_t local = k * 256 + threadIdx.x;
        const size_t r = base + local;
        const rv32::CycleRec rec = read_record(recs, r, n_recs);
        const watch::Decoded d = watch::decode(rec, a.n_instr, a.text_base, a.statics, a.offs, a.sh);
        if (r >= n_recs) continue;   // (no barrier inside the loop)
        if (d.bad) { atomicAdd(&wg_bad, 1u); continue; }
        const bool pre = watch::position(a.shard, (uint32_t)r) < a.P;
        const uint32_t rd = d.st & watch::ST_RD_MASK;   // < 32
        if (pre && rd) atomicMax(&reg[rd], local + 1);
        snap::for_decided(a.rg, d, a.sh, [&](uint32_t slot, uint32_t) {
            if (slot >= n_words) return;
            if (pre) atomicMax(&bef[slot], local + 1);
            else atomicMin(&aft[slot], local);
        });
    }
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < n_words; s += 256) {
        if (bef[s]) atomicMax(&t.before[s], watch::position(a.shard, (uint32_t)(base + bef[s] - 1)));
        if (aft[s] != NOBODY) atomicMin(&t.after[s], watch::position(a.shard, (uint32_t)(base + aft[s])));
    }
    if (threadIdx.x < 32 && reg[threadIdx.x]) atomicMax(&t.regs[threadIdx.x], watch::position(a.shard, (uint32_t)(base + reg[threadIdx.x] - 1)));
    if (threadIdx.x == 0 && wg_bad) atomicAdd(t.bad_records, (unsigned long long)wg_bad);
}

__global__ void __launch_bounds__(256) snap_gather_kernel(const SnapFetch *items, uint32_t n_items, const SnapArgs a, snap::Side *out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_items) return;   // (no barrier in this kernel)
    const SnapFetch it = items[i];
    snap::Side s{snap::SIDE_BAD, 0, it.shard, it.row, 0, 0};
    if (it.recs && it.row < it.n_recs) {
        const rv32::CycleRec rec = read_record(it.recs, it.row, it.n_recs);
        const watch::Decoded d = watch::decode(rec, a.n_instr, a.text_base, a.statics, a.offs, a.sh);
        s = snap::side_of(rec, d, a.sh, it.shard, it.row, it.addr, it.what);
    }
    out[i] = s;
}

bool args_ok(const SnapArgs &a) {
    if (!a.n_instr || !a.statics || !a.offs || a.sh.n > memrep::MAX_PRE || a.rg.n > snap::MAX_RANGES || a.rg.n_words > snap::MAX_WORDS) return false;
    for (uint32_t r = 0; r < a.rg.n; r++)   // every slot of a range lies in the tables
        if (a.rg.lo[r] >= a.rg.hi[r] || ((a.rg.lo[r] | a.rg.hi[r]) & 3) || (unsigned long long)a.rg.at[r] + (a.rg.hi[r] - a.rg.lo[r]) / 4 > a.rg.n_words) return false;
    return true;
}

}  // namespace

hipError_t launch_snapshot_reduce(hipStream_t st, const rv32::CycleRec *d_recs, size_t n_recs, const SnapArgs &a, const SnapTables &t) {
    if (!n_recs) return hipSuccess;
    if (!args_ok(a) || !t.regs || !t.bad_records || (a.rg.n_words && (!t.before || !t.after)) || n_recs > 0xffffffffull) return hipErrorInvalidValue;
    snap_reduce_kernel<<<(unsigned)((n_recs + snap::SPAN - 1) / snap::SPAN), 256, 0, st>>>(d_recs, n_recs, a, t);
    return hipGetLastError();
}

hipError_t launch_snapshot_gather(hipStream_t st, const SnapFetch *d_items, uint32_t n_items, const SnapArgs &a, void *d_out) {
    if (!n_items) return hipSuccess;
    if (!args_ok(a) || !d_items || !d_out) return hipErrorInvalidValue;
    snap_gather_kernel<<<(n_items + 255) / 256, 256, 0, st>>>(d_items, n_items, a, static_cast<snap::Side *>(d_out));
    return hipGetLastError();
}

}  // namespace dvt
