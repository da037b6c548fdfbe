// The execution report's tally (profile.h) of the cycle records a prepared job holds in HBM, and the host's side of the report.
//
// One thread per record, the launch shape of K0 (256 threads, a fixed span of consecutive records per workgroup).  A thread
// reads the first 16-byte word of its record (idx, b = t0 of an ECALL), the next record's idx, and one word per instruction
// (class and static target, profile.h).  Counting as K0 counts its lookups (rv32_trace.hip): a loop body hits the same dozen
// instructions and the same taken branches, and global atomics on them serialise at the memory side, so every workgroup adds up
// in a direct-mapped LDS cache of (key -> count) first, a conflict falls through to a global atomic, and the cache is flushed
// once per workgroup with 64-bit adds.  K0's own cache (DeviceSink::count) flushes into the two 32-bit multiplicity columns it
// is bound to; this one has the same shape with 64-bit destinations.
//   key i                 instruction i retired                           -> pc_count[i]
//   key n_instr + i       the branch / JAL i went to its static target    -> taken[i]
// Every other transfer (JALR: returns, indirect calls) is an edge with the 64-bit key from << 32 | to: a second, smaller LDS
// cache per workgroup, then an insert-only open-addressing table in global memory, at most 64 probes of one atomicCAS each; an
// edge that finds no slot adds its count to the dropped counter.  ECALL records are rare: a wave without one skips the path by
// ballot, the others CAS into a table of 64 ids.  Nothing here waits for another thread, and every loop is bounded by the launch
// or by the 64 probes.
#include <algorithm>

#include "kernels.h"
#include "profile.h"

namespace dvt {

constexpr uint32_t PROF_RECS_PER_BLOCK = 4096;   // records tallied by one workgroup (16 per thread)
constexpr uint32_t PROF_SLOTS = 4096;            // 32 KiB of LDS: a workgroup sees at most 4096 distinct instructions
constexpr uint32_t PROF_EDGE_SLOTS = 1024;       // 12 KiB: the indirect edges of one span
constexpr uint32_t PROF_EMPTY = 0xffffffffu;
constexpr unsigned long long PROF_NO_KEY = ~0ull;

namespace {

__device__ __forceinline__ bool first_active_lane(unsigned long long active) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(active >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)active, 0)) == 0;
}

struct ProfileSink {
    const ProfileTables &t;
    uint32_t *keys, *counts;             // [PROF_SLOTS]
    unsigned long long *edge_keys;       // [PROF_EDGE_SLOTS]
    uint32_t *edge_counts;

    __device__ void global_add(uint32_t key, uint32_t cnt) {
        if (key < t.n_instr) atomicAdd(&t.pc_count[key], (unsigned long long)cnt);
        else atomicAdd(&t.taken[key - t.n_instr], (unsigned long long)cnt);
    }
    __device__ void count(uint32_t key) {
        // wave-uniform fast path: every active lane has the same key -> one add of the lane count
        const uint32_t first = __builtin_amdgcn_readfirstlane(key);
        const unsigned long long active = __ballot(1), same = __ballot(key == first);
        uint32_t cnt = 1;
        if (same == active) {
            if (!first_active_lane(active)) return;
            cnt = (uint32_t)__popcll(active);
        }
        const uint32_t slot = (key * 2654435761u) >> 20;  // 12 bits
        const uint32_t old = atomicCAS(&keys[slot], PROF_EMPTY, key);
        if (old == PROF_EMPTY || old == key) atomicAdd(&counts[slot], cnt);
        else global_add(key, cnt);
    }
    __device__ void edge_global(unsigned long long key, unsigned long long cnt) {
        const uint32_t mask = (1u << t.log_slots) - 1;
        uint32_t s = (uint32_t)((key * 0x9e3779b97f4a7c15ull) >> (64 - t.log_slots));
        for (int k = 0; k < 64; k++, s = (s + 1) & mask) {
            const unsigned long long old = atomicCAS(&t.edge_keys[s], PROF_NO_KEY, key);
            if (old == PROF_NO_KEY || old == key) { atomicAdd(&t.edge_counts[s], cnt); return; }
        }
        atomicAdd(&t.counters[PROFILE_DROPPED], cnt);
    }
    __device__ void edge(uint32_t from, uint32_t to) {
        const unsigned long long key = (unsigned long long)from << 32 | to;
        const uint32_t slot = (uint32_t)((key * 0x9e3779b97f4a7c15ull) >> 54);  // 10 bits
        const unsigned long long old = atomicCAS(&edge_keys[slot], PROF_NO_KEY, key);
        if (old == PROF_NO_KEY || old == key) atomicAdd(&edge_counts[slot], 1u);
        else edge_global(key, 1);
    }
    __device__ void syscall(uint32_t id) {
        uint32_t s = (id * 2654435761u) >> 26;  // 6 bits
        for (uint32_t k = 0; k < prof::MAX_SYSCALLS; k++, s = (s + 1) & (prof::MAX_SYSCALLS - 1)) {
            const unsigned long long old = atomicCAS(&t.sys_keys[s], PROF_NO_KEY, (unsigned long long)id);
            if (old == PROF_NO_KEY || old == id) { atomicAdd(&t.sys_counts[s], 1ull); return; }
        }
        atomicAdd(&t.counters[PROFILE_SYS_OVERFLOW], 1ull);
    }
};

__global__ void __launch_bounds__(256) profile_records_kernel(const rv32::CycleRec *recs, size_t n_recs, uint32_t last_succ, const ProfileTables t) {
    __shared__ uint32_t keys[PROF_SLOTS], counts[PROF_SLOTS];
    __shared__ unsigned long long edge_keys[PROF_EDGE_SLOTS];
    __shared__ uint32_t edge_counts[PROF_EDGE_SLOTS];
    __shared__ uint32_t wg_transfers, wg_bad;
    for (uint32_t s = threadIdx.x; s < PROF_SLOTS; s += blockDim.x) { keys[s] = PROF_EMPTY; counts[s] = 0; }
    for (uint32_t s = threadIdx.x; s < PROF_EDGE_SLOTS; s += blockDim.x) { edge_keys[s] = PROF_NO_KEY; edge_counts[s] = 0; }
    if (threadIdx.x == 0) wg_transfers = wg_bad = 0;
    __syncthreads();
    ProfileSink sink{t, keys, counts, edge_keys, edge_counts};
    const size_t base = (size_t)blockIdx.x * PROF_RECS_PER_BLOCK;
    for (uint32_t k = 0; k < PROF_RECS_PER_BLOCK / 256; k++) {
        const size_t r = base + (size_t)k * 256 + threadIdx.x;
        if (r >= n_recs) continue;
        const uint4 w = *reinterpret_cast<const uint4 *>(&recs[r]);   // idx, a, b, c
        const uint32_t idx = w.x;
        uint32_t succ = r + 1 < n_recs ? recs[r + 1].idx : last_succ;
        // (the executor writes neither: an index outside the text is counted and nothing is indexed with it)
        const bool bad = idx >= t.n_instr || (succ != prof::NO_SUCC && succ >= t.n_instr);
        if (bad) atomicAdd(&wg_bad, 1u);
        if (idx >= t.n_instr) continue;
        if (bad) succ = prof::NO_SUCC;
        sink.count(idx);
        const uint32_t m = t.classes[idx], cls = m >> prof::CLS_SHIFT;
        const bool transfer = succ != prof::NO_SUCC && succ != idx + 1;
        const unsigned long long active = __ballot(1), moved = __ballot(transfer);
        if (moved && first_active_lane(active)) atomicAdd(&wg_transfers, (uint32_t)__popcll(moved));
        if (transfer) {
            if (cls == prof::CLS_STATIC && succ == (m & prof::TGT_MASK)) sink.count(t.n_instr + idx);
            else sink.edge(idx, succ);
        }
        if (__ballot(cls == prof::CLS_ECALL))
            if (cls == prof::CLS_ECALL) sink.syscall(w.z);
    }
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < PROF_SLOTS; s += blockDim.x)
        if (keys[s] != PROF_EMPTY && counts[s]) sink.global_add(keys[s], counts[s]);
    for (uint32_t s = threadIdx.x; s < PROF_EDGE_SLOTS; s += blockDim.x)
        if (edge_keys[s] != PROF_NO_KEY && edge_counts[s]) sink.edge_global(edge_keys[s], edge_counts[s]);
    if (threadIdx.x == 0) {
        if (wg_transfers) atomicAdd(&t.counters[PROFILE_TRANSFERS], (unsigned long long)wg_transfers);
        if (wg_bad) atomicAdd(&t.counters[PROFILE_BAD_RECORDS], (unsigned long long)wg_bad);
    }
}

}  // namespace

hipError_t launch_profile_records(hipStream_t st, const rv32::CycleRec *d_recs, size_t n_recs, uint32_t last_succ, const ProfileTables &t) {
    if (!n_recs) return hipSuccess;
    if (!t.n_instr || t.log_slots < prof::MIN_LOG_SLOTS || t.log_slots > prof::MAX_LOG_SLOTS || (last_succ != prof::NO_SUCC && last_succ >= t.n_instr))
        return hipErrorInvalidValue;
    profile_records_kernel<<<(unsigned)((n_recs + PROF_RECS_PER_BLOCK - 1) / PROF_RECS_PER_BLOCK), 256, 0, st>>>(d_recs, n_recs, last_succ, t);
    return hipGetLastError();
}

// ------------------------------------------------------------------ the host's side
namespace prof {

void tally_records(const rv32::Program &prog, const rv32::CycleRec *recs, size_t n, uint32_t last_succ, Tally *t) {
    const uint32_t n_instr = (uint32_t)t->pc_count.size();
    for (size_t r = 0; r < n; r++) {
        const uint32_t idx = recs[r].idx;
        if (idx >= n_instr) continue;
        uint32_t succ = r + 1 < n ? recs[r + 1].idx : last_succ;
        if (succ != NO_SUCC && succ >= n_instr) succ = NO_SUCC;
        t->pc_count[idx]++;
        if (succ != NO_SUCC && succ != idx + 1) {
            t->n_transfers++;
            t->edges[{idx, succ}]++;
        }
        if (prog.instrs[idx].kind == rv32::K_ECALL) t->sys[recs[r].b]++;
    }
    t->shards++;
}

const char *mnemonic(uint32_t w) {
    const uint32_t op = w & 0x7f, f3 = (w >> 12) & 7, f7 = w >> 25;
    switch (op) {
    case 0x37: return "lui";
    case 0x17: return "auipc";
    case 0x6f: return "jal";
    case 0x67: return f3 == 0 ? "jalr" : "unknown";
    case 0x63: { static const char *const n[8] = {"beq", "bne", "unknown", "unknown", "blt", "bge", "bltu", "bgeu"}; return n[f3]; }
    case 0x03: { static const char *const n[8] = {"lb", "lh", "lw", "unknown", "lbu", "lhu", "unknown", "unknown"}; return n[f3]; }
    case 0x23: { static const char *const n[8] = {"sb", "sh", "sw", "unknown", "unknown", "unknown", "unknown", "unknown"}; return n[f3]; }
    case 0x13:
        if (f3 == 1) return f7 == 0 ? "slli" : "unknown";
        if (f3 == 5) return f7 == 0 ? "srli" : f7 == 0x20 ? "srai" : "unknown";
        { static const char *const n[8] = {"addi", "", "slti", "sltiu", "xori", "", "ori", "andi"}; return n[f3]; }
    case 0x33:
        if (f7 == 0) { static const char *const n[8] = {"add", "sll", "slt", "sltu", "xor", "srl", "or", "and"}; return n[f3]; }
        if (f7 == 0x20) return f3 == 0 ? "sub" : f3 == 5 ? "sra" : "unknown";
        if (f7 == 1) { static const char *const n[8] = {"mul", "mulh", "mulhsu", "mulhu", "div", "divu", "rem", "remu"}; return n[f3]; }
        return "unknown";
    case 0x0f: return "fence";
    case 0x73: return w == 0x73 ? "ecall" : "unknown";
    default: return "unknown";
    }
}

bool emit(const rv32::Program &prog, const Tally &t, uint32_t shards_total, double ms, const Out &out) {
    if (t.sys.size() > MAX_SYSCALLS) return false;
    const size_t n = t.pc_count.size();
    dvt_profile_summary s{};
    for (size_t i = 0; i < n; i++) s.cycles += t.pc_count[i];
    std::copy_n(t.pc_count.begin(), std::min(n, out.cap_pc), out.pc_count);
    size_t at = 0;
    for (auto &e : t.edges) {
        if (at < out.cap_edges) out.edges[at] = dvt_profile_edge{prog.text_base + 4 * e.first.first, prog.text_base + 4 * e.first.second, e.second};
        at++;
    }
    s.n_edges = (uint32_t)at;
    at = 0;
    for (auto &e : t.sys) {
        if (at < out.cap_sys) out.sys[at] = dvt_profile_syscall{e.first, 0, e.second};
        at++;
    }
    s.n_syscalls = (uint32_t)at;
    std::map<std::string, uint64_t> by_name;
    for (size_t i = 0; i < n; i++)
        if (t.pc_count[i]) by_name[mnemonic(prog.instrs[i].raw)] += t.pc_count[i];
    std::vector<std::pair<std::string, uint64_t>> ops(by_name.begin(), by_name.end());
    std::stable_sort(ops.begin(), ops.end(), [](const auto &a, const auto &b) { return a.second > b.second; });   // (names ascend already)
    for (size_t i = 0; i < ops.size() && i < out.cap_ops; i++) {
        dvt_profile_opcode o{};
        strncpy(o.name, ops[i].first.c_str(), sizeof o.name - 1);
        o.count = ops[i].second;
        out.ops[i] = o;
    }
    s.n_opcodes = (uint32_t)ops.size();
    s.n_transfers = t.n_transfers;
    s.dropped_transfers = t.dropped;
    s.text_base = prog.text_base;
    s.n_instr = (uint32_t)n;
    s.shards_tallied = t.shards;
    s.shards_total = shards_total;
    s.ms = (float)ms;
    *out.summary = s;
    return true;
}

}  // namespace prof
}  // namespace dvt
