// What the device passes over cycle records share (watch.hip, snapshot.hip, origin.hip, uses.hip, diverge.hip): a thread's read
// of its record, a lane's rank in a ballot, and the LDS staging of a pass over sorted questions (PassArgs, dataflow.h).
#pragma once
#include <hip/hip_runtime.h>

#include "dataflow.h"

namespace dvt {

__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}

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

// the first of the sorted targets [lo, hi) that is >= addr (at most 9 steps for the 256 of a pass)
__device__ __forceinline__ uint32_t first_word(const uint32_t *target, uint32_t lo, uint32_t hi, uint32_t addr) {
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (target[mid] < addr) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Stages the sorted questions of a pass in the LDS arrays of a workgroup of 256 = DVT_ORIGIN_PASS_QUESTIONS threads: pos and target [256], reg_off [33].
// It contains a barrier: every thread of the workgroup calls it, and what the kernel sets in LDS before the call is visible after
// it.  It returns n = min(a.n, PASS_Q); no offset of reg_off exceeds n, whatever the arguments say.
__device__ __forceinline__ uint32_t stage_pass(const PassArgs &a, unsigned long long *pos, uint32_t *target, uint32_t *reg_off) {
    const uint32_t t = threadIdx.x, n = a.n < DVT_ORIGIN_PASS_QUESTIONS ? a.n : DVT_ORIGIN_PASS_QUESTIONS;
    if (t < n) { pos[t] = a.pos[t]; target[t] = a.target[t]; }
    if (t < 33) reg_off[t] = a.reg_off[t] < n ? a.reg_off[t] : n;
    __syncthreads();
    return n;
}

}  // namespace dvt
