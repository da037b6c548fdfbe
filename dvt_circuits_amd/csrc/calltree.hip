// The call-tree report's device pass (calltree.h) over the cycle records a prepared job holds in HBM, and the host's side of
// the report.
//
// The launch shape of the execution report (profile.hip): 256 threads, one workgroup per span of 4096 consecutive records of a
// shard.  One body, two modes.  Every thread reads idx of its 16 records and their successors as profile_records_kernel does
// and looks up the class word; the CALL and RET events of the span are compacted in record order into LDS (ballot / mbcnt
// prefix per wave, the 64 wave counts of the span scanned through LDS), and one lane walks the compacted list with an LDS stack
// of event numbers.
//   summary mode  reduces the span to u unmatched RETs followed by c unmatched CALLs and writes {u, c}; run once more with
//                 host-computed offsets it also writes the c calls as (callee, position in the span)
//   emit mode     is given the top min(u + 1, depth) frames of the stack on entry (the host merges the summaries in
//                 execution order between the modes) and repeats the walk with everything known: a RET at local depth 0 pops
//                 the next incoming frame, whose caller is the one below; a CALL at local depth 0 has the current incoming
//                 top as caller; a RET that finds only the root counts as unmatched.  The deepest stack is taken here, where
//                 the depth on entry is known.  Every closed frame goes into a per-workgroup LDS map (caller << 32 | fn ->
//                 calls, cycles), which all threads flush once into the insert-only open-addressing table in global memory:
//                 at most 64 probes of one atomicCAS, then two 64-bit adds; an arc without a slot adds to the dropped counters.
// No thread waits for another workgroup; every loop is bounded by the span, the LDS map or the 64 probes.  Static LDS: 16 KiB
// event words, 8 KiB positions, 8 KiB stack, 12 KiB map.
#include <algorithm>

#include "calltree.h"
#include "kernels.h"

namespace dvt {

constexpr uint32_t CT_MAP_SLOTS = 512, CT_MAP_PROBES = 16;
constexpr unsigned long long CT_NO_KEY = ~0ull;
constexpr uint32_t CT_ITERS = CALLTREE_SPAN / 256, CT_WAVES = 256 / 64;
constexpr uint32_t CT_FN_MASK = (1u << 28) - 1;   // an event word: the class word's event bits, the callee below them

namespace {

struct ArcSink {
    const CalltreeTables &t;
    unsigned long long *keys, *calls, *cycles;   // [CT_MAP_SLOTS], in LDS

    __device__ void global_add(unsigned long long key, unsigned long long n, unsigned long long cyc) const {
        const uint32_t mask = (1u << t.log_slots) - 1;
        uint32_t s = (uint32_t)((key * 0x9e3779b97f4a7c15ull) >> (64 - t.log_slots));
        for (int k = 0; k < 64; k++, s = (s + 1) & mask) {
            const unsigned long long old = atomicCAS(&t.arc_keys[s], CT_NO_KEY, key);
            if (old == CT_NO_KEY || old == key) {
                atomicAdd(&t.arc_calls[s], n);
                atomicAdd(&t.arc_cycles[s], cyc);
                return;
            }
        }
        atomicAdd(&t.counters[CALLTREE_DROPPED_FRAMES], n);
        atomicAdd(&t.counters[CALLTREE_DROPPED_CYCLES], cyc);
    }
    // the walking lane alone: no atomics on the LDS map
    __device__ void close(uint32_t caller, uint32_t fn, unsigned long long cyc) const {
        const unsigned long long key = (unsigned long long)caller << 32 | fn;
        uint32_t s = (uint32_t)((key * 0x9e3779b97f4a7c15ull) >> 55);   // 9 bits
        for (uint32_t k = 0; k < CT_MAP_PROBES; k++, s = (s + 1) & (CT_MAP_SLOTS - 1)) {
            if (keys[s] == CT_NO_KEY) keys[s] = key;
            if (keys[s] == key) { calls[s]++; cycles[s] += cyc; return; }
        }
        global_add(key, 1, cyc);
    }
};

__global__ void __launch_bounds__(256) calltree_span_kernel(const rv32::CycleRec *recs, size_t n_recs, uint32_t last_succ, size_t span0,
                                                            unsigned long long base_position, bool emit, const CalltreeTables t) {
    __shared__ uint32_t ev_word[CALLTREE_SPAN];     // EV_CALL | callee, or EV_RET
    __shared__ uint16_t ev_pos[CALLTREE_SPAN];      // position in the span
    __shared__ uint16_t stack[CALLTREE_SPAN];       // event numbers of the open local calls
    __shared__ unsigned long long map_keys[CT_MAP_SLOTS], map_calls[CT_MAP_SLOTS], map_cycles[CT_MAP_SLOTS];
    __shared__ uint32_t wave_at[CT_ITERS * CT_WAVES + 1];
    __shared__ uint32_t wg_bad, left_open;
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    if (emit)
        for (uint32_t s = tid; s < CT_MAP_SLOTS; s += 256) { map_keys[s] = CT_NO_KEY; map_calls[s] = 0; map_cycles[s] = 0; }
    if (tid == 0) wg_bad = left_open = 0;
    __syncthreads();
    const size_t span = span0 + blockIdx.x, base = (size_t)blockIdx.x * CALLTREE_SPAN;

    // ---- the events of this thread's records (record base + 256 k + tid), and how many each wave has per k
    uint32_t mine[CT_ITERS];
#pragma unroll
    for (uint32_t k = 0; k < CT_ITERS; k++) {
        const size_t r = base + (size_t)k * 256 + tid;
        uint32_t w = 0;
        if (r < n_recs) {
            const uint32_t idx = recs[r].idx;
            uint32_t succ = r + 1 < n_recs ? recs[r + 1].idx : last_succ;
            // (the executor writes neither: an index outside the text is counted and nothing is indexed with it)
            const bool bad = idx >= t.n_instr || (succ != prof::NO_SUCC && succ >= t.n_instr);
            if (bad) { atomicAdd(&wg_bad, 1u); succ = prof::NO_SUCC; }
            if (idx < t.n_instr) {
                const uint32_t cls = t.classes[idx];
                if (cls & calltree::EV_RET) w = calltree::EV_RET;
                else if ((cls & calltree::EV_CALL) && succ != prof::NO_SUCC) w = calltree::EV_CALL | succ;
            }
        }
        mine[k] = w;
        const unsigned long long has = __ballot(w != 0);
        if ((tid & 63) == 0) wave_at[k * CT_WAVES + wave] = (uint32_t)__popcll(has);
    }
    __syncthreads();
    if (tid == 0) {   // exclusive scan of the 64 counts, in record order
        uint32_t at = 0;
        for (uint32_t i = 0; i < CT_ITERS * CT_WAVES; i++) { const uint32_t n = wave_at[i]; wave_at[i] = at; at += n; }
        wave_at[CT_ITERS * CT_WAVES] = at;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < CT_ITERS; k++) {
        const unsigned long long has = __ballot(mine[k] != 0);
        if (mine[k]) {
            const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(has >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)has, 0));
            const uint32_t e = wave_at[k * CT_WAVES + wave] + before;   // < CALLTREE_SPAN: at most one event per record
            ev_word[e] = mine[k];
            ev_pos[e] = (uint16_t)(k * 256 + tid);
        }
    }
    __syncthreads();
    const uint32_t n_ev = wave_at[CT_ITERS * CT_WAVES];

    // ---- one lane walks the events
    if (!emit) {
        if (tid == 0) {
            uint32_t depth = 0, u = 0;
            for (uint32_t e = 0; e < n_ev; e++) {
                if (ev_word[e] & calltree::EV_CALL) stack[depth++] = (uint16_t)e;
                else if (depth) depth--;
                else u++;
            }
            t.summaries[span] = CalltreeSpanSummary{u, depth};
            left_open = depth;
        }
        if (!t.calls_at) return;
        __syncthreads();
        CalltreeCall *out = t.calls + t.calls_at[span];
        for (uint32_t i = tid; i < left_open; i += 256) out[i] = CalltreeCall{ev_word[stack[i]] & CT_FN_MASK, ev_pos[stack[i]]};
        return;
    }
    const ArcSink sink{t, map_keys, map_calls, map_cycles};
    if (tid == 0) {
        const CalltreeSpanIn in = t.span_in[span];
        const CalltreeFrame *frames = t.frames + in.frames_at;
        const unsigned long long pos0 = base_position + base;
        uint32_t depth = 0, used = 0, global_depth = in.depth, deepest = in.depth, unmatched = 0, short_in = 0;
        for (uint32_t e = 0; e < n_ev; e++) {
            const unsigned long long end = pos0 + ev_pos[e] + 1;
            if (ev_word[e] & calltree::EV_CALL) {
                stack[depth++] = (uint16_t)e;
                deepest = max(deepest, ++global_depth);
            } else if (depth) {
                const uint32_t f = stack[--depth], fn = ev_word[f] & CT_FN_MASK;
                uint32_t caller = calltree::NO_FN;
                if (depth) caller = ev_word[stack[depth - 1]] & CT_FN_MASK;
                else if (used < in.n_frames) caller = frames[used].fn;
                else short_in++;
                sink.close(caller, fn, end - (pos0 + ev_pos[f] + 1));
                global_depth--;
            } else if (global_depth > 1) {
                // (the host hands over min(u + 1, depth) frames: the one below the popped frame is among them)
                if (used + 1 < in.n_frames) sink.close(frames[used + 1].fn, frames[used].fn, end - frames[used].open);
                else short_in++;
                used++;
                global_depth--;
            } else unmatched++;
        }
        if (unmatched) atomicAdd(&t.counters[CALLTREE_UNMATCHED], (unsigned long long)unmatched);
        if (short_in) atomicAdd(&t.counters[CALLTREE_BAD_RECORDS], (unsigned long long)short_in);
        atomicMax(&t.counters[CALLTREE_MAX_DEPTH], (unsigned long long)deepest);
        if (wg_bad) atomicAdd(&t.counters[CALLTREE_BAD_RECORDS], (unsigned long long)wg_bad);
    }
    __syncthreads();
    for (uint32_t s = tid; s < CT_MAP_SLOTS; s += 256)
        if (map_keys[s] != CT_NO_KEY) sink.global_add(map_keys[s], map_calls[s], map_cycles[s]);
}

hipError_t launch(hipStream_t st, const rv32::CycleRec *d_recs, size_t n_recs, uint32_t last_succ, size_t span0, unsigned long long base_position,
                  bool emit, const CalltreeTables &t) {
    if (!n_recs) return hipSuccess;
    if (!t.n_instr || !t.classes || (last_succ != prof::NO_SUCC && last_succ >= t.n_instr)) return hipErrorInvalidValue;
    if (emit ? t.log_slots < prof::MIN_LOG_SLOTS || t.log_slots > prof::MAX_LOG_SLOTS || !t.span_in || !t.frames || !t.arc_keys || !t.counters
             : !t.summaries || (t.calls_at && !t.calls))
        return hipErrorInvalidValue;
    calltree_span_kernel<<<(unsigned)((n_recs + CALLTREE_SPAN - 1) / CALLTREE_SPAN), 256, 0, st>>>(d_recs, n_recs, last_succ, span0, base_position, emit, t);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_calltree_summary(hipStream_t st, const rv32::CycleRec *d_recs, size_t n_recs, uint32_t last_succ, size_t span0, const CalltreeTables &t) {
    return launch(st, d_recs, n_recs, last_succ, span0, 0, false, t);
}
hipError_t launch_calltree_emit(hipStream_t st, const rv32::CycleRec *d_recs, size_t n_recs, uint32_t last_succ, size_t span0,
                                unsigned long long base_position, const CalltreeTables &t) {
    return launch(st, d_recs, n_recs, last_succ, span0, base_position, true, t);
}

// ------------------------------------------------------------------ the host's side
namespace calltree {

void walk_records(const rv32::Program &prog, const rv32::CycleRec *recs, size_t n, uint32_t last_succ, uint64_t base_position, State *st) {
    const uint32_t n_instr = (uint32_t)st->classes.size();
    for (size_t r = 0; r < n; r++) {
        const uint32_t idx = recs[r].idx;
        const uint64_t g = base_position + r;
        if (st->stack.empty() && !st->cycles && !g) st->stack.push_back(Frame{idx, 0});   // the root
        st->cycles = g + 1;
        st->max_depth = std::max(st->max_depth, (uint32_t)st->stack.size());
        if (idx >= n_instr) continue;
        uint32_t succ = r + 1 < n ? recs[r + 1].idx : last_succ;
        if (succ != prof::NO_SUCC && succ >= n_instr) succ = prof::NO_SUCC;
        const uint32_t cls = st->classes[idx];
        if (cls & EV_RET) {
            if (st->stack.size() > 1) st->close_top(g + 1);
            else st->unmatched_returns++;
        } else if ((cls & EV_CALL) && succ != prof::NO_SUCC) {
            st->stack.push_back(Frame{succ, g + 1});
            st->max_depth = std::max(st->max_depth, (uint32_t)st->stack.size());
        }
    }
}

void emit(const rv32::Program &prog, const State &st, uint32_t shards_total, double ms, const Out &out) {
    auto pc_of = [&](uint32_t fn) { return fn == NO_FN ? NO_FN : prog.text_base + 4 * fn; };
    dvt_calltree_summary s{};
    size_t at = 0;
    struct Func { uint64_t calls = 0, inclusive = 0, out = 0; bool called = false; };
    std::map<uint32_t, Func> by_fn;
    for (auto &a : st.arcs) {
        if (at < out.cap_arcs) out.arcs[at] = dvt_calltree_arc{pc_of(a.first.first), pc_of(a.first.second), a.second.calls, a.second.cycles};
        at++;
        s.n_frames += a.second.calls;
        Func &f = by_fn[a.first.second];
        f.calls += a.second.calls;
        f.inclusive += a.second.cycles;
        f.called = true;
        if (a.first.first != NO_FN) by_fn[a.first.first].out += a.second.cycles;
    }
    s.n_arcs = (uint32_t)at;
    s.n_frames += st.dropped_frames;
    if (!st.dropped_frames) {   // (with dropped arcs the sums out of and into a function are unknown)
        std::vector<dvt_calltree_func> funcs;
        for (auto &f : by_fn)
            if (f.second.called) funcs.push_back(dvt_calltree_func{pc_of(f.first), 0, f.second.calls, f.second.inclusive, f.second.inclusive - f.second.out});
        std::stable_sort(funcs.begin(), funcs.end(), [](const dvt_calltree_func &a, const dvt_calltree_func &b) { return a.self > b.self; });   // (pcs ascend already)
        std::copy_n(funcs.begin(), std::min(funcs.size(), out.cap_funcs), out.funcs);
        s.n_funcs = (uint32_t)funcs.size();
    }
    s.cycles = st.cycles;
    s.dropped_frames = st.dropped_frames;
    s.dropped_cycles = st.dropped_cycles;
    s.unmatched_returns = st.unmatched_returns;
    s.text_base = prog.text_base;
    s.n_instr = (uint32_t)st.classes.size();
    s.max_depth = st.max_depth;
    s.open_at_exit = st.open_at_exit;
    s.shards_total = shards_total;
    s.ms = (float)ms;
    *out.summary = s;
}

}  // namespace calltree
}  // namespace dvt
