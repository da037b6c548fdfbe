// The memory report (include/dvt_prover.h: dvt_rv32_job_memory, dvt_execute_memory): which pages an execution loads from and
// stores to, how many distinct words it accesses (every one of them is a row of the mem_init table), which
// instruction accessed a word first, and how far the stack pointer moves; from the cycle records of the execution.  The rule,
// here in plain C++ for the host path and in memreport.hip for the records a prepared job holds in HBM:
//
//   Words are the 4-byte aligned guest addresses below ADDR_LIMIT; a page is PAGE_BYTES = 4096 bytes = 1024 words, N_PAGES of
//   them.  The registers (REG_BASE ...) are never part of the report: not the ports of an instruction, and not the a1 read
//   that COMMIT and the precompile ECALLs make through the memory port.
//
//   Loads and stores.  A record whose instruction is lb lh lw lbu lhu is one load, one whose instruction is sb sh sw one
//   store, of the word (rec.b + instr.off) & ~3: loads / stores of its page += 1.  When (rec.sh_cm >> 16) == 0 (shards are
//   numbered from 1: no shard accessed the word before) the access is a FIRST TOUCH, the first access of the word in the whole
//   execution, whether the word belongs to the image, was hinted (HINT_READ sets initial values without an access: a hinted
//   word is first touched by the load that reads it) or neither: first_touch[rec.idx] += 1 and first of its page += 1.
//
//   Precompile calls, from the ECALL record alone: id = rec.b (t0), a0 = rec.c, a1 = rec.m_prev (the value the a1 port read).
//     SHA_EXTEND    64 words at a0: words 0..15 are reads, words 16..63 writes
//     SHA_COMPRESS  64 reads at a0; 8 reads and 8 writes at a1
//     a field, curve or u256 call (bigop_info(id): words_a, words_b)   words_b reads at a1; words_a reads and words_a writes at a0
//   pre_reads / pre_writes of the page of each such word += 1 (an array may straddle a page), pre_calls += 1 per call.
//   Nothing else touches memory in this sense: HALT, WRITE (it peeks at the bytes without an access), COMMIT,
//   COMMIT_DEFERRED_PROOFS, HINT_LEN and HINT_READ (initial values, no access) count nothing.
//
//   Footprint.  words of a page = the distinct words any counted access hit (loads, stores, precompile reads and writes).
//   Whether a precompile word is a first touch is not in the records (the events that carried its previous access are freed
//   after K0), so it is not reported; but on a whole execution
//       words - sum of first_touch = the words first touched by a precompile call
//   because every word is first touched exactly once, by a load, a store or a call.  The identity is documented, not stored.
//
//   Stack.  Over the records whose instruction has rd == x2: sp_writes, and the minimum and the maximum of the value written
//   (rec.a).  Without such a record all three are 0.
//
//   Summary.  The totals of the above; image_words = the words of the program image (what Vm::mem_rows() lists before the
//   first touches, without the 32 registers); image_words_accessed = those among them that were accessed; and, when the
//   records are those of a whole execution, mem_init_rows = 32 + image_words + words - image_words_accessed: the height of the
//   mem_init table before padding (else 0).
//
// Every figure is an exact integer; nothing is bounded, sampled or dropped.
#pragma once
#include <algorithm>
#include <map>
#include <vector>

#include "../../include/dvt_prover.h"
#include "rv32.h"

namespace dvt {
namespace memrep {

constexpr uint32_t PAGE_SHIFT = 12, PAGE_BYTES = 1u << PAGE_SHIFT;
constexpr uint32_t N_PAGES = rv32::ADDR_LIMIT >> PAGE_SHIFT;        // 229 376
constexpr uint32_t LINE_WORDS = PAGE_BYTES / 4 / 32;                // a page's line of the footprint bitmap: 32 words = 128 bytes
constexpr uint32_t BITMAP_WORDS = rv32::ADDR_LIMIT / 4 / 32;        // one bit per word of guest memory: 29.4 MB
static_assert(N_PAGES * LINE_WORDS == BITMAP_WORDS && rv32::ADDR_LIMIT % PAGE_BYTES == 0, "pages tile the address space");

// What the device pass reads per instruction besides the records: the class bits and the address offset.
enum : uint32_t { CLS_LOAD = 1, CLS_STORE = 2, CLS_ECALL = 4, CLS_SP = 8 };
inline uint32_t instr_class(const rv32::Instr &in) {
    const bool load = in.kind >= rv32::K_LW && in.kind <= rv32::K_LHU, store = in.kind >= rv32::K_SW && in.kind <= rv32::K_SH;
    return (load ? CLS_LOAD : 0) | (store ? CLS_STORE : 0) | (in.kind == rv32::K_ECALL ? CLS_ECALL : 0) | (in.rd == 2 ? CLS_SP : 0);
}

// The shape of a precompile call: n0 words at a0, of which the first r0 are reads and the last w0 writes; n1 words at a1, all
// reads, the last w1 also writes.  At most MAX_PRE of them, MAX_CALL_WORDS words per call.
struct PreShape { uint32_t id, n0, r0, w0, n1, w1; };
constexpr uint32_t MAX_PRE = 16, MAX_CALL_WORDS = 72;
// One array of a call as every loop and range test over a call's words takes it: `n` words at `base` (capped at MAX_CALL_WORDS),
// the words [0, n_read) are read, the words [first_written, n) written.
struct CallArray { uint32_t base, n, n_read, first_written; };
DVT_HD CallArray call_array(const PreShape &s, uint32_t arr, uint32_t a0, uint32_t a1) {
    const uint32_t full = arr ? s.n1 : s.n0, r = arr ? s.n1 : s.r0, w = arr ? s.w1 : s.w0;
    const uint32_t n = full < MAX_CALL_WORDS ? full : MAX_CALL_WORDS, first = w < full ? full - w : 0;
    return CallArray{arr ? a1 : a0, n, r < n ? r : n, first < n ? first : n};
}
// every word of a call, array 0 first: f(address, is it read, is it written)
template <class F>
DVT_HD void for_call_words(const PreShape &s, uint32_t a0, uint32_t a1, F f) {
    for (uint32_t arr = 0; arr < 2; arr++) {
        const CallArray e = call_array(s, arr, a0, a1);
#pragma nounroll   // (calls are rare and f is inlined into every pass: one copy of it per array)
        for (uint32_t k = 0; k < e.n; k++) f(e.base + 4 * k, k < e.n_read, k >= e.first_written);
    }
}
constexpr uint32_t LDS_PAGE_SLOTS = 256;   // the device pass: slots of a workgroup's direct-mapped page cache (memreport.hip)
inline std::vector<PreShape> pre_shapes() {
    std::vector<PreShape> t{{rv32::SYS_SHA_EXTEND, 64, 16, 48, 0, 0}, {rv32::SYS_SHA_COMPRESS, 64, 64, 0, 8, 8}};
    for (uint32_t id : {rv32::SYS_SECP256K1_ADD, rv32::SYS_SECP256K1_DOUBLE, rv32::SYS_BLS12381_ADD, rv32::SYS_BLS12381_DOUBLE, rv32::SYS_BLS12381_FP_ADD,
                        rv32::SYS_BLS12381_FP_SUB, rv32::SYS_BLS12381_FP_MUL, rv32::SYS_BLS12381_FP2_ADD, rv32::SYS_BLS12381_FP2_SUB,
                        rv32::SYS_BLS12381_FP2_MUL, rv32::SYS_UINT256_MUL}) {
        rv32::BigOpInfo bi;
        if (rv32::bigop_info(id, &bi)) t.push_back({id, (uint32_t)bi.words_a, (uint32_t)bi.words_a, (uint32_t)bi.words_a, (uint32_t)bi.words_b, 0});
    }
    return t;
}
// Host only: what the device pass takes in one upload, [classes | offs | the shapes, six words each].
inline std::vector<uint32_t> device_table(const rv32::Program &prog, const std::vector<PreShape> &shapes) {
    const size_t n = prog.instrs.size() - 1;
    std::vector<uint32_t> t(2 * n);
    for (size_t i = 0; i < n; i++) {
        t[i] = instr_class(prog.instrs[i]);
        t[n + i] = prog.instrs[i].off;
    }
    for (auto &s : shapes) t.insert(t.end(), {s.id, s.n0, s.r0, s.w0, s.n1, s.w1});
    return t;
}

// one page while it is added up; bits: its line of the footprint bitmap
struct Page {
    uint64_t loads = 0, stores = 0, pre_reads = 0, pre_writes = 0;
    uint32_t first = 0;
    uint32_t bits[LINE_WORDS] = {};
    uint32_t words() const {
        uint32_t n = 0;
        for (uint32_t w : bits) n += (uint32_t)__builtin_popcount(w);
        return n;
    }
};
struct Tally {
    std::vector<uint64_t> first_touch;
    std::map<uint32_t, Page> pages;   // by page number
    uint64_t cycles = 0, pre_calls = 0, sp_writes = 0;
    uint32_t sp_min = 0xffffffffu, sp_max = 0, shards = 0;
    explicit Tally(const rv32::Program &prog) : first_touch(prog.instrs.size() - 1, 0) {}
    // one counted access of the word at byte address addr (below ADDR_LIMIT); the page it belongs to
    Page &touch(uint32_t addr) {
        Page &p = pages[addr >> PAGE_SHIFT];
        p.bits[(addr >> 7) & (LINE_WORDS - 1)] |= 1u << ((addr >> 2) & 31);
        return p;
    }
};

// the records of one shard; a record that names no instruction of the text or an address outside guest memory (the executor
// writes neither) counts nothing
inline void tally_records(const rv32::Program &prog, const std::vector<PreShape> &shapes, const rv32::CycleRec *recs, size_t n, Tally *t) {
    const uint32_t n_instr = (uint32_t)t->first_touch.size();
    for (size_t r = 0; r < n; r++) {
        const rv32::CycleRec &rec = recs[r];
        if (rec.idx >= n_instr) continue;
        const rv32::Instr &in = prog.instrs[rec.idx];
        const uint32_t cls = instr_class(in);
        t->cycles++;
        if (cls & CLS_SP) {
            t->sp_writes++;
            t->sp_min = std::min(t->sp_min, rec.a);
            t->sp_max = std::max(t->sp_max, rec.a);
        }
        if (cls & (CLS_LOAD | CLS_STORE)) {
            const uint32_t addr = (rec.b + in.off) & ~3u;
            if (addr >= rv32::ADDR_LIMIT) continue;
            Page &p = t->touch(addr);
            (cls & CLS_LOAD ? p.loads : p.stores)++;
            if ((rec.sh_cm >> 16) == 0) {
                p.first++;
                t->first_touch[rec.idx]++;
            }
        } else if (cls & CLS_ECALL) {
            for (const PreShape &s : shapes) {
                if (s.id != rec.b) continue;
                const uint32_t a0 = rec.c & ~3u, a1 = rec.m_prev & ~3u;
                if ((uint64_t)a0 + 4 * s.n0 > rv32::ADDR_LIMIT || (uint64_t)a1 + 4 * s.n1 > rv32::ADDR_LIMIT) break;
                t->pre_calls++;
                for (uint32_t k = 0; k < s.n0; k++) {
                    Page &p = t->touch(a0 + 4 * k);
                    p.pre_reads += k < s.r0;
                    p.pre_writes += k >= s.n0 - s.w0;
                }
                for (uint32_t k = 0; k < s.n1; k++) {
                    Page &p = t->touch(a1 + 4 * k);
                    p.pre_reads++;
                    p.pre_writes += k >= s.n1 - s.w1;
                }
                break;
            }
        }
    }
    t->shards++;
}

// the caller's arrays of both entry points
struct Out {
    uint64_t *first_touch; size_t cap_instr;
    dvt_memory_page *pages; size_t cap_pages;
    dvt_memory_summary *summary;
    bool null_array() const { return (cap_instr && !first_touch) || (cap_pages && !pages); }
};

// a finished tally into the caller's arrays; whole: the records were those of every shard of the execution
inline void emit(const rv32::Program &prog, const Tally &t, uint32_t shards_total, bool whole, double ms, const Out &out) {
    dvt_memory_summary s{};
    const size_t n = t.first_touch.size();
    std::copy_n(t.first_touch.begin(), std::min(n, out.cap_instr), out.first_touch);
    for (size_t i = 0; i < n; i++) s.first_touches += t.first_touch[i];
    size_t at = 0;
    for (auto &kv : t.pages) {
        const Page &p = kv.second;
        const uint32_t words = p.words();
        if (at < out.cap_pages) out.pages[at] = dvt_memory_page{kv.first << PAGE_SHIFT, words, p.first, 0, p.loads, p.stores, p.pre_reads, p.pre_writes};
        at++;
        s.loads += p.loads; s.stores += p.stores; s.pre_reads += p.pre_reads; s.pre_writes += p.pre_writes; s.words += words;
    }
    for (auto &kv : prog.image) {
        if (kv.first >= rv32::ADDR_LIMIT) continue;   // (the registers)
        s.image_words++;
        const auto it = t.pages.find(kv.first >> PAGE_SHIFT);
        if (it != t.pages.end() && (it->second.bits[(kv.first >> 7) & (LINE_WORDS - 1)] >> ((kv.first >> 2) & 31) & 1)) s.image_words_accessed++;
    }
    s.mem_init_rows = whole ? 32 + s.image_words + s.words - s.image_words_accessed : 0;
    s.cycles = t.cycles;
    s.pre_calls = t.pre_calls;
    s.sp_writes = t.sp_writes;
    s.sp_min = t.sp_writes ? t.sp_min : 0;
    s.sp_max = t.sp_writes ? t.sp_max : 0;
    s.text_base = prog.text_base;
    s.n_instr = (uint32_t)n;
    s.n_pages = (uint32_t)at;
    s.page_bytes = PAGE_BYTES;
    s.shards_tallied = t.shards;
    s.shards_total = shards_total;
    s.ms = (float)ms;
    *out.summary = s;
}

}  // namespace memrep
}  // namespace dvt
