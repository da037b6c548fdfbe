// The memory report's pass (memreport.h) over the cycle records a prepared job holds in HBM.
//
// One thread per record, the launch shape of profile_records_kernel (256 threads, a fixed span of 4096 consecutive records per
// workgroup).  A thread reads the first 16-byte word of its record (idx, a, b, c) and two static words per instruction (class
// bits and address offset, memreport.h); m_prev and sh_cm only when the class is a load, a store or an ECALL.
//   page counters   dense 64-bit arrays over the 229 376 pages.  A loop hits the same few pages (its stack frame, one buffer)
//                   from every lane, and global atomics on them would serialise at the memory side: every workgroup adds up
//                   in a direct-mapped LDS cache (page -> loads, stores, first) with the wave-uniform fast path of
//                   ProfileSink::count (profile.hip): lanes that all hit one page with one kind of access cost one add per
//                   wave.  A conflict falls through to a global atomic; the cache is flushed once per workgroup.
//   first_touch     per instruction, the same way through a second small cache (a first touch is rare: once per word).
//   footprint       one bit per word of guest memory.  A thread reads the bitmap word first (a device-scope relaxed load) and
//                   skips the atomicOr when its bit is set.  The read is only a filter: a stale zero costs one redundant
//                   atomic, and correctness rests on the device-scope atomicOr alone.
//   precompiles     ECALL records are rare: a wave without one skips the path by ballot, a lane with one looks its id up in a
//                   table of at most 16 shapes and walks the at most 72 words of the call, one add per page and one OR per
//                   bitmap word it covers.
//   stack           the values written to x2: a wave reduction, then atomicMin / atomicMax in LDS, one pair of global atomics
//                   per workgroup.
// After the shards a second small kernel gathers the counters and the 128-byte bitmap line of every page that has an access
// into a dense array for the host.
// No thread waits for another, and every loop is bounded by the launch, by the 72 words of a call or by the table sizes.
#include "kernels.h"
#include "memreport.h"

namespace dvt {

constexpr uint32_t MEM_RECS_PER_BLOCK = 4096;                    // records tallied by one workgroup (16 per thread)
constexpr uint32_t MEM_LOG_PAGE_SLOTS = 8, MEM_LOG_FT_SLOTS = 8;  // 4 KiB + 2 KiB of LDS
constexpr uint32_t MEM_FT_SLOTS = 1u << MEM_LOG_FT_SLOTS;
constexpr uint32_t MEM_EMPTY = 0xffffffffu;
static_assert(memrep::LDS_PAGE_SLOTS == 1u << MEM_LOG_PAGE_SLOTS, "the slot hash takes the top bits");

namespace {

__device__ __forceinline__ bool first_active_lane(unsigned long long active) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(active >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)active, 0)) == 0;
}

struct MemorySink {
    const MemoryTables &t;
    uint32_t *page_keys, *page_counts;   // [LDS_PAGE_SLOTS], [LDS_PAGE_SLOTS][3]: loads, stores, first
    uint32_t *ft_keys, *ft_counts;       // [MEM_FT_SLOTS]

    __device__ unsigned long long *page_ctr(uint32_t array, uint32_t page) { return &t.page_ctr[(size_t)array * memrep::N_PAGES + page]; }
    // one bit of the footprint (addr below ADDR_LIMIT), mask: bits of the bitmap word addr >> 7
    __device__ void mark(uint32_t word, uint32_t mask) {
        uint32_t *w = &t.bitmap[word];
        if ((__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & mask) != mask) atomicOr(w, mask);
    }
    // a load (kind 0) or a store (kind 1) of a word of `page`
    __device__ void access(uint32_t page, uint32_t kind, bool first) {
        const uint32_t key = page << 1 | kind;
        const unsigned long long active = __ballot(1), same = __ballot(key == (uint32_t)__builtin_amdgcn_readfirstlane(key)), firsts = __ballot(first);
        uint32_t cnt = 1, fcnt = first;
        if (same == active) {   // wave-uniform: one add of the lane count
            if (!first_active_lane(active)) return;
            cnt = (uint32_t)__popcll(active);
            fcnt = (uint32_t)__popcll(firsts);
        }
        const uint32_t slot = (page * 2654435761u) >> (32 - MEM_LOG_PAGE_SLOTS);
        const uint32_t old = atomicCAS(&page_keys[slot], MEM_EMPTY, page);
        if (old == MEM_EMPTY || old == page) {
            atomicAdd(&page_counts[3 * slot + kind], cnt);
            if (fcnt) atomicAdd(&page_counts[3 * slot + 2], fcnt);
        } else {
            atomicAdd(page_ctr(kind ? MEMORY_STORES : MEMORY_LOADS, page), (unsigned long long)cnt);
            if (fcnt) atomicAdd(page_ctr(MEMORY_FIRST, page), (unsigned long long)fcnt);
        }
    }
    __device__ void first_touch(uint32_t idx) {
        const unsigned long long active = __ballot(1), same = __ballot(idx == (uint32_t)__builtin_amdgcn_readfirstlane(idx));
        uint32_t cnt = 1;
        if (same == active) {
            if (!first_active_lane(active)) return;
            cnt = (uint32_t)__popcll(active);
        }
        const uint32_t slot = (idx * 2654435761u) >> (32 - MEM_LOG_FT_SLOTS);
        const uint32_t old = atomicCAS(&ft_keys[slot], MEM_EMPTY, idx);
        if (old == MEM_EMPTY || old == idx) atomicAdd(&ft_counts[slot], cnt);
        else atomicAdd(&t.first_touch[idx], (unsigned long long)cnt);
    }
    // n words from base (the whole array below ADDR_LIMIT): the first r are reads, the last w writes
    __device__ void walk(uint32_t base, uint32_t n, uint32_t r, uint32_t w) {
        uint32_t page = base >> memrep::PAGE_SHIFT, word = base >> 7, reads = 0, writes = 0, mask = 0;
        for (uint32_t k = 0; k < n && k < memrep::MAX_CALL_WORDS; k++) {
            const uint32_t addr = base + 4 * k;
            if ((addr >> 7) != word) { mark(word, mask); word = addr >> 7; mask = 0; }
            if ((addr >> memrep::PAGE_SHIFT) != page) {
                if (reads) atomicAdd(page_ctr(MEMORY_PRE_READS, page), (unsigned long long)reads);
                if (writes) atomicAdd(page_ctr(MEMORY_PRE_WRITES, page), (unsigned long long)writes);
                page = addr >> memrep::PAGE_SHIFT; reads = writes = 0;
            }
            mask |= 1u << ((addr >> 2) & 31);
            reads += k < r;
            writes += k + w >= n;
        }
        if (mask) mark(word, mask);
        if (reads) atomicAdd(page_ctr(MEMORY_PRE_READS, page), (unsigned long long)reads);
        if (writes) atomicAdd(page_ctr(MEMORY_PRE_WRITES, page), (unsigned long long)writes);
    }
    // an ECALL record: 1 = a precompile call was counted, 0 = another syscall, 2 = a call whose arrays leave guest memory
    __device__ uint32_t ecall(uint32_t id, uint32_t a0, uint32_t a1) {
        for (uint32_t k = 0; k < t.n_pre && k < memrep::MAX_PRE; k++) {
            const uint32_t *s = t.pre + 6 * k;
            if (s[0] != id) continue;
            const uint32_t n0 = s[1], n1 = s[4];
            a0 &= ~3u; a1 &= ~3u;
            if (n0 + n1 > memrep::MAX_CALL_WORDS || (unsigned long long)a0 + 4 * n0 > rv32::ADDR_LIMIT || (unsigned long long)a1 + 4 * n1 > rv32::ADDR_LIMIT) return 2;
            walk(a0, n0, s[2], s[3]);
            walk(a1, n1, n1, s[5]);
            return 1;
        }
        return 0;
    }
};

__global__ void __launch_bounds__(256) memory_records_kernel(const rv32::CycleRec *recs, size_t n_recs, const MemoryTables t) {
    __shared__ uint32_t page_keys[memrep::LDS_PAGE_SLOTS], page_counts[3 * memrep::LDS_PAGE_SLOTS];
    __shared__ uint32_t ft_keys[MEM_FT_SLOTS], ft_counts[MEM_FT_SLOTS];
    __shared__ uint32_t wg_cycles, wg_bad, wg_calls, wg_sp, wg_sp_min, wg_sp_max;
    for (uint32_t s = threadIdx.x; s < memrep::LDS_PAGE_SLOTS; s += blockDim.x) { page_keys[s] = MEM_EMPTY; page_counts[3 * s] = page_counts[3 * s + 1] = page_counts[3 * s + 2] = 0; }
    for (uint32_t s = threadIdx.x; s < MEM_FT_SLOTS; s += blockDim.x) { ft_keys[s] = MEM_EMPTY; ft_counts[s] = 0; }
    if (threadIdx.x == 0) { wg_cycles = wg_bad = wg_calls = wg_sp = wg_sp_max = 0; wg_sp_min = 0xffffffffu; }
    __syncthreads();
    MemorySink sink{t, page_keys, page_counts, ft_keys, ft_counts};
    const size_t base = (size_t)blockIdx.x * MEM_RECS_PER_BLOCK;
    const bool lane0 = (threadIdx.x & 63) == 0;
    for (uint32_t k = 0; k < MEM_RECS_PER_BLOCK / 256; k++) {   // (every thread runs every round: the wave steps below need all lanes)
        const size_t r = base + (size_t)k * 256 + threadIdx.x;
        uint4 w = make_uint4(MEM_EMPTY, 0, 0, 0);   // idx, a, b, c
        if (r < n_recs) w = *reinterpret_cast<const uint4 *>(&recs[r]);
        const uint32_t idx = w.x;
        // (the executor writes no index outside the text: such a record is counted and nothing is indexed with it)
        const bool real = r < n_recs && idx < t.n_instr;
        uint32_t bad = r < n_recs && !real;
        const uint32_t cls = real ? t.classes[idx] : 0;
        const unsigned long long reals = __ballot(real);
        if (reals && lane0) atomicAdd(&wg_cycles, (uint32_t)__popcll(reals));
        // ---- the stack pointer
        const bool sp = cls & memrep::CLS_SP;
        const unsigned long long sps = __ballot(sp);
        if (sps) {
            uint32_t lo = sp ? w.y : 0xffffffffu, hi = sp ? w.y : 0u;
            for (int m = 32; m > 0; m >>= 1) {
                lo = min(lo, (uint32_t)__shfl_xor((int)lo, m));
                hi = max(hi, (uint32_t)__shfl_xor((int)hi, m));
            }
            if (lane0) { atomicMin(&wg_sp_min, lo); atomicMax(&wg_sp_max, hi); atomicAdd(&wg_sp, (uint32_t)__popcll(sps)); }
        }
        // ---- loads and stores
        if (cls & (memrep::CLS_LOAD | memrep::CLS_STORE)) {
            const uint32_t addr = (w.z + t.offs[idx]) & ~3u;
            if (addr >= rv32::ADDR_LIMIT) bad = 1;
            else {
                const bool first = (recs[r].sh_cm >> 16) == 0;
                sink.access(addr >> memrep::PAGE_SHIFT, cls & memrep::CLS_STORE ? 1 : 0, first);
                if (first) sink.first_touch(idx);
                sink.mark(addr >> 7, 1u << ((addr >> 2) & 31));
            }
        }
        // ---- precompile calls
        const bool is_ecall = cls & memrep::CLS_ECALL;
        if (__ballot(is_ecall)) {
            if (is_ecall) {
                const uint32_t rc = sink.ecall(w.z, w.w, recs[r].m_prev);
                if (rc == 1) atomicAdd(&wg_calls, 1u);
                else if (rc == 2) bad = 1;
            }
        }
        if (bad) atomicAdd(&wg_bad, 1u);
    }
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < memrep::LDS_PAGE_SLOTS; s += blockDim.x) {
        const uint32_t page = page_keys[s];
        if (page == MEM_EMPTY) continue;
        if (page_counts[3 * s]) atomicAdd(sink.page_ctr(MEMORY_LOADS, page), (unsigned long long)page_counts[3 * s]);
        if (page_counts[3 * s + 1]) atomicAdd(sink.page_ctr(MEMORY_STORES, page), (unsigned long long)page_counts[3 * s + 1]);
        if (page_counts[3 * s + 2]) atomicAdd(sink.page_ctr(MEMORY_FIRST, page), (unsigned long long)page_counts[3 * s + 2]);
    }
    for (uint32_t s = threadIdx.x; s < MEM_FT_SLOTS; s += blockDim.x)
        if (ft_keys[s] != MEM_EMPTY && ft_counts[s]) atomicAdd(&t.first_touch[ft_keys[s]], (unsigned long long)ft_counts[s]);
    if (threadIdx.x == 0) {
        if (wg_cycles) atomicAdd(&t.counters[MEMORY_CYCLES], (unsigned long long)wg_cycles);
        if (wg_calls) atomicAdd(&t.counters[MEMORY_PRE_CALLS], (unsigned long long)wg_calls);
        if (wg_bad) atomicAdd(&t.counters[MEMORY_BAD_RECORDS], (unsigned long long)wg_bad);
        if (wg_sp) {
            atomicAdd(&t.counters[MEMORY_SP_WRITES], (unsigned long long)wg_sp);
            atomicMin(&t.sp[0], wg_sp_min);
            atomicMax(&t.sp[1], wg_sp_max);
        }
    }
}

// one thread per page of the address space
__global__ void __launch_bounds__(256) memory_gather_kernel(const MemoryTables t, MemoryDensePage *dense, uint32_t cap, uint32_t *n_dense) {
    const uint32_t page = blockIdx.x * 256 + threadIdx.x;
    if (page >= memrep::N_PAGES) return;
    unsigned long long c[MEMORY_PAGE_ARRAYS];
    for (uint32_t a = 0; a < MEMORY_PAGE_ARRAYS; a++) c[a] = t.page_ctr[(size_t)a * memrep::N_PAGES + page];
    if (!(c[MEMORY_LOADS] | c[MEMORY_STORES] | c[MEMORY_PRE_READS] | c[MEMORY_PRE_WRITES])) return;
    const uint32_t at = atomicAdd(n_dense, 1u);
    if (at >= cap) return;
    MemoryDensePage &d = dense[at];
    d.page = page; d.first = (uint32_t)c[MEMORY_FIRST];
    d.loads = c[MEMORY_LOADS]; d.stores = c[MEMORY_STORES]; d.pre_reads = c[MEMORY_PRE_READS]; d.pre_writes = c[MEMORY_PRE_WRITES];
    for (uint32_t k = 0; k < memrep::LINE_WORDS; k++) d.bits[k] = t.bitmap[(size_t)page * memrep::LINE_WORDS + k];
}

}  // namespace

hipError_t launch_memory_records(hipStream_t st, const rv32::CycleRec *d_recs, size_t n_recs, const MemoryTables &t) {
    if (!n_recs) return hipSuccess;
    if (!t.n_instr || t.n_pre > memrep::MAX_PRE) return hipErrorInvalidValue;
    memory_records_kernel<<<(unsigned)((n_recs + MEM_RECS_PER_BLOCK - 1) / MEM_RECS_PER_BLOCK), 256, 0, st>>>(d_recs, n_recs, t);
    return hipGetLastError();
}

hipError_t launch_memory_gather(hipStream_t st, const MemoryTables &t, MemoryDensePage *d_dense, uint32_t cap, uint32_t *d_n_dense) {
    memory_gather_kernel<<<(memrep::N_PAGES + 255) / 256, 256, 0, st>>>(t, d_dense, cap, d_n_dense);
    return hipGetLastError();
}

}  // namespace dvt
