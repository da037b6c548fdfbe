// Snapshots (include/dvt_prover.h: dvt_rv32_job_snapshot, dvt_execute_snapshot): the registers, chosen memory words and the call
// stack of an execution as they are BEFORE the record at a position P = (shard, row) executes, from the cycle records of the
// execution.  The rule, in plain C++ for the host path (Taker) and, through the same decode(), for_decided(), side_of() and
// cell_of(), for the kernels of snapshot.hip over the records a prepared job holds in HBM:
//
//   Positions are watch.h's: shard = ShardJob::index (from 1), row = the record's index within its shard, compared
//   lexicographically (watch::position).  A P past the last record is the state after the last record; (0xffffffff, 0xffffffff)
//   is the state at exit, on the host path at the trap.
//
//   Registers.  x_k, k = 1..31: rec.a of the last record before P whose instruction has rd == k (the model and the executor
//   write registers nowhere else: ECALL is decoded with rd = t0), flags FROM_BEFORE and the record's (shard, row, pc).  Without
//   such a record: 0 and INITIAL.  x0 is 0.  Register values are always exact.
//
//   Memory.  Up to MAX_RANGES ranges [lo, hi) of word addresses, 4-aligned and below ADDR_LIMIT, MAX_WORDS words in all; slot s
//   of the answer is word (s - at[r]) of range r, the ranges concatenated (a word that two ranges hold has two slots with equal
//   cells).  The DECIDING accesses of a word are the ones that can change or reveal it: loads, stores (watch::decode gives the
//   word before and after) and the words a precompile call WRITES (the PRE_WRITE entries of memrep::pre_shapes(), found with
//   watch::call_match); the words a call only reads stay as they were and are skipped.  B = the last deciding access of the word
//   before P, A = the first at or after P.  The first case that applies (cell_of):
//       B is a store              `after` of B        FROM_BEFORE | STORE                          source B
//       B is a load               `after` of B        FROM_BEFORE | LOAD                           source B
//       A is a load or a store    `before` of A       FROM_AFTER, and INITIAL when there is no B   source A
//       no B, an image word       the image's word    IMAGE | INITIAL                              no source
//       otherwise                 0                   NO_VALUE                                     source B if there is one, else A
//   UNTOUCHED is added when neither B nor A exists.  NO_VALUE: a precompile call wrote the word and nothing loads it before the
//   next such write; the values a call writes are not in the records (the limit DVT_WATCH_HIT_NO_VALUE states), the cell names
//   the call.  An untouched word outside the image is NO_VALUE too: a hint may have filled it without an access.
//   INITIAL: nothing accessed the word before P, and the value is the one the memory argument starts the word with: image, hint
//   or 0.  HINT_READ sets initial values without an access, so a hinted word holds its value in the real machine only from its
//   HINT_READ on: a snapshot taken before that call shows the hinted value early.  That is the one place where a cell that
//   carries a value can differ from the machine.
//
//   Call stack.  calltree.h's rule over the records before P (the successor of the last of them is the record at P); the
//   frames open after them are the backtrace, innermost first.  A frame: fn, the global position `open` of its first record,
//   and of the call record at open - 1 its pc and rec.a (the value written to ra); the root has call_pc 0xffffffff, ra 0.
//   Without a record before P there is no frame.
//
//   Summary.  position = the number of records before P; (shard, row) = where record `position` lies (locate()), at the end
//   the last shard and its record count; pc = that record's pc, at the end the last shard's next_pc.
//
// A record the executor never writes (watch::decode's bad) decides nothing and is counted: the call fails with DVT_ERR_INPUT.
#pragma once
#include <string>

#include "calltree.h"
#include "watch.h"

namespace dvt {
namespace snap {

constexpr uint32_t SPAN = DVT_SNAP_SPAN, MAX_RANGES = DVT_SNAP_MAX_RANGES, MAX_WORDS = DVT_SNAP_MAX_WORDS;

// the ranges as the passes take them (by value on the device); at: the slot of the range's first word
struct Ranges {
    uint32_t n, n_words;
    uint32_t lo[MAX_RANGES], hi[MAX_RANGES], at[MAX_RANGES];
};

// One side of a word (B or A), a register's writer or a frame's call record: what the record at (shard, row) says.
enum : uint32_t { SIDE_NONE = 0, SIDE_LOAD = 1, SIDE_STORE = 2, SIDE_PRE = 3, SIDE_REG = 4, SIDE_BAD = 5 };
enum : uint32_t { WHAT_REG = 0, WHAT_BEFORE = 1, WHAT_AFTER = 2, WHAT_FRAME = 3 };
struct Side { uint32_t kind, value, shard, row, pc, pad; };

// every watched slot the record decides: f(slot, word address)
template <class F>
DVT_HD void for_decided(const Ranges &rg, const watch::Decoded &d, const watch::Shapes &sh, F f) {
    if (d.bad) return;
    if (d.dir) {
        for (uint32_t r = 0; r < rg.n && r < MAX_RANGES; r++)
            if (d.addr >= rg.lo[r] && d.addr < rg.hi[r]) f(rg.at[r] + (d.addr - rg.lo[r]) / 4, d.addr);
    } else if (d.shape >= 0 && d.shape < (int)memrep::MAX_PRE) {
        const memrep::PreShape &s = sh.s[d.shape];
        for (uint32_t r = 0; r < rg.n && r < MAX_RANGES; r++) {
            if (!watch::call_match(s, d.a0, d.a1, rg.lo[r], rg.hi[r], DVT_WATCH_PRE_WRITE).n) continue;   // (most calls write nothing of a range)
            memrep::for_call_words(s, d.a0, d.a1, [&](uint32_t addr, bool, bool written) {
                if (written && addr >= rg.lo[r] && addr < rg.hi[r]) f(rg.at[r] + (addr - rg.lo[r]) / 4, addr);
            });
        }
    }
}

// What the record at (shard, row) says as `what` of addr (a register number for WHAT_REG): SIDE_BAD when it is no such record.
DVT_HD Side side_of(const rv32::CycleRec &rec, const watch::Decoded &d, const watch::Shapes &sh, uint32_t shard, uint32_t row, uint32_t addr, uint32_t what) {
    Side s{SIDE_BAD, 0, shard, row, d.pc, 0};
    if (d.bad) return s;
    if (what == WHAT_FRAME || (what == WHAT_REG && addr && (d.st & watch::ST_RD_MASK) == addr)) {
        s.kind = SIDE_REG;
        s.value = rec.a;
    } else if (what == WHAT_BEFORE || what == WHAT_AFTER) {
        if (d.dir && d.addr == addr) {
            s.kind = d.dir == DVT_WATCH_STORE ? SIDE_STORE : SIDE_LOAD;
            s.value = what == WHAT_BEFORE ? d.after : d.before;
        } else if (!d.dir && d.shape >= 0 && d.shape < (int)memrep::MAX_PRE && watch::call_match(sh.s[d.shape], d.a0, d.a1, addr, addr + 4, DVT_WATCH_PRE_WRITE).n)
            s.kind = SIDE_PRE;
    }
    return s;
}

// the cell of a word from its two sides; image_word: nullptr when the word is not part of the program image
inline dvt_snap_cell cell_of(uint32_t addr, const Side &B, const Side &A, const uint32_t *image_word) {
    dvt_snap_cell c{addr, 0, 0, 0, 0, 0};
    const Side *src = nullptr;
    if (B.kind == SIDE_STORE || B.kind == SIDE_LOAD) {
        c.value = B.value;
        c.flags = DVT_SNAP_FROM_BEFORE | (B.kind == SIDE_STORE ? DVT_SNAP_STORE : DVT_SNAP_LOAD);
        src = &B;
    } else if (A.kind == SIDE_STORE || A.kind == SIDE_LOAD) {
        c.value = A.value;
        c.flags = DVT_SNAP_FROM_AFTER | (B.kind == SIDE_NONE ? DVT_SNAP_INITIAL : 0);
        src = &A;
    } else if (B.kind == SIDE_NONE && image_word) {
        c.value = *image_word;
        c.flags = DVT_SNAP_IMAGE | DVT_SNAP_INITIAL;
    } else {
        c.flags = DVT_SNAP_NO_VALUE;
        src = B.kind != SIDE_NONE ? &B : A.kind != SIDE_NONE ? &A : nullptr;
    }
    if (B.kind == SIDE_NONE && A.kind == SIDE_NONE) c.flags |= DVT_SNAP_UNTOUCHED;
    if (src) { c.shard = src->shard; c.row = src->row; c.pc = src->pc; }
    return c;
}

inline dvt_snap_cell reg_cell(uint32_t k, const Side &w) {
    if (!k) return dvt_snap_cell{0, 0, 0, 0, 0, 0};
    if (w.kind != SIDE_REG) return dvt_snap_cell{k, 0, DVT_SNAP_INITIAL, 0, 0, 0};
    return dvt_snap_cell{k, w.value, DVT_SNAP_FROM_BEFORE, w.shard, w.row, w.pc};
}

}  // namespace snap

// What the kernels of snapshot.hip take by value (kernels.h declares the launches).
struct SnapArgs {
    snap::Ranges rg;
    watch::Shapes sh;
    const uint32_t *statics, *offs;   // [n_instr], device
    uint32_t n_instr, text_base, shard;
    unsigned long long P;
};
// the winners of a member: positions, zeroed (before, regs: none = 0, every position has shard >= 1) or all ones (after)
struct SnapTables {
    unsigned long long *before, *after;   // [rg.n_words]
    unsigned long long *regs;             // [32]
    unsigned long long *bad_records;
};
// one record to look at again: `what` of addr at (shard, row) of the shard whose records are recs
struct SnapFetch {
    const rv32::CycleRec *recs;
    uint32_t n_recs, shard, row, addr, what, pad;
};

namespace snap {

// ---------------------------------------------------------------- host only
// nullptr, or what is wrong with the ranges of a call; *out: the ranges with their slots
inline const char *input_error(const dvt_snap_range *ranges, size_t n, const dvt_snap_cell *regs, const dvt_snap_cell *words, size_t cap_words,
                               const dvt_snap_frame *frames, size_t cap_frames, Ranges *out, std::string *text) {
    auto say = [&](size_t i, const char *what) { *text = "range " + std::to_string(i) + ": " + what; return text->c_str(); };
    *out = Ranges{};
    if (n > MAX_RANGES) return (*text = "n_ranges " + std::to_string(n) + " (at most " + std::to_string(MAX_RANGES) + ")").c_str();
    if (!regs || (n && !ranges) || (cap_frames && !frames)) return (*text = "null array").c_str();
    unsigned long long total = 0;
    for (size_t i = 0; i < n; i++) {
        if ((ranges[i].lo | ranges[i].hi) & 3) return say(i, "not 4-aligned");
        if (ranges[i].lo >= ranges[i].hi) return say(i, "lo >= hi");
        if (ranges[i].hi > rv32::ADDR_LIMIT) return say(i, "reaches past the address limit");
        out->lo[i] = ranges[i].lo; out->hi[i] = ranges[i].hi; out->at[i] = (uint32_t)total;
        total += (ranges[i].hi - ranges[i].lo) / 4;
        if (total > MAX_WORDS) return (*text = "more than " + std::to_string(MAX_WORDS) + " words").c_str();
    }
    if (total > cap_words) return (*text = "cap_words " + std::to_string(cap_words) + " below the " + std::to_string(total) + " words of the ranges").c_str();
    if (total && !words) return (*text = "null array").c_str();
    out->n = (uint32_t)n;
    out->n_words = (uint32_t)total;
    return nullptr;
}

// where the record with global number g lies, given the record counts of the shards in order: past the last record, the last
// shard and its count ((1, 0) when there is no shard)
inline void locate(const std::vector<uint64_t> &shard_n, uint64_t g, uint32_t *shard, uint32_t *row) {
    uint64_t base = 0;
    for (size_t k = 0; k < shard_n.size(); k++) {
        if (g < base + shard_n[k] || k + 1 == shard_n.size()) {
            *shard = (uint32_t)k + 1;
            *row = (uint32_t)std::min<uint64_t>(g - base, shard_n[k]);
            return;
        }
        base += shard_n[k];
    }
    *shard = 1; *row = 0;
}

inline const uint32_t *image_word(const rv32::Program &prog, uint32_t addr) {
    const auto it = std::lower_bound(prog.image.begin(), prog.image.end(), std::make_pair(addr, 0u));
    return it != prog.image.end() && it->first == addr ? &it->second : nullptr;
}

// of a frame of the stack besides calltree::Frame: its call record
struct CallRec { uint32_t call_pc = 0xffffffffu, ra = 0; };

// The answer from its parts, for both entry points: the registers' writers, the sides of every slot, the stack (outermost
// first, calltree::Frame::open global) with the call record of every frame that will be returned.
struct Parts {
    const Side *reg;                       // [32]
    const Side *before, *after;            // [rg.n_words]
    const std::vector<calltree::Frame> *stack;
    const std::vector<CallRec> *calls;     // parallel to *stack; only the innermost cap_frames are read
    const std::vector<uint64_t> *shard_n;
    uint64_t position, cycles, unmatched_returns;
    uint32_t pc;
};
inline void emit(const rv32::Program &prog, const Ranges &rg, const Parts &in, double ms, dvt_snap_cell regs[32], dvt_snap_cell *words, dvt_snap_frame *frames,
                 size_t cap_frames, dvt_snap_summary *summary) {
    dvt_snap_summary s{};
    for (uint32_t k = 0; k < 32; k++) regs[k] = reg_cell(k, in.reg[k]);
    for (uint32_t r = 0; r < rg.n; r++)
        for (uint32_t addr = rg.lo[r]; addr < rg.hi[r]; addr += 4) {
            const uint32_t slot = rg.at[r] + (addr - rg.lo[r]) / 4;
            const dvt_snap_cell c = cell_of(addr, in.before[slot], in.after[slot], image_word(prog, addr));
            words[slot] = c;
            s.no_value += (c.flags & DVT_SNAP_NO_VALUE) != 0;
            s.initial += (c.flags & DVT_SNAP_INITIAL) != 0;
            s.untouched += (c.flags & DVT_SNAP_UNTOUCHED) != 0;
        }
    const size_t depth = in.stack->size(), nf = std::min(depth, cap_frames);
    for (size_t f = 0; f < nf; f++) {
        const calltree::Frame &fr = (*in.stack)[depth - 1 - f];
        const CallRec &cr = (*in.calls)[depth - 1 - f];
        dvt_snap_frame o{prog.text_base + 4 * fr.fn, cr.call_pc, 0, 0, cr.ra, 0};
        locate(*in.shard_n, fr.open, &o.open_shard, &o.open_row);
        frames[f] = o;
    }
    s.position = in.position; s.cycles = in.cycles;
    locate(*in.shard_n, in.position, &s.shard, &s.row);
    s.pc = in.pc;
    s.depth = (uint32_t)std::min<size_t>(depth, 0xffffffffu); s.n_frames = (uint32_t)nf;
    s.unmatched_returns = (uint32_t)std::min<uint64_t>(in.unmatched_returns, 0xffffffffu);
    s.n_words = rg.n_words;
    s.shards_total = (uint32_t)in.shard_n->size();
    s.text_base = prog.text_base; s.n_instr = (uint32_t)prog.instrs.size() - 1; s.span = SPAN;
    s.ms = (float)ms;
    *summary = s;
}

// The host path's state: the shards of an execution in order, one at a time.
struct Taker {
    Ranges rg;
    unsigned long long P;
    watch::Statics stat;
    watch::Shapes sh;
    Side reg[32] = {};
    std::vector<Side> before, after;
    calltree::State st;
    std::vector<CallRec> calls;   // parallel to st.stack
    std::vector<uint64_t> shard_n;
    uint64_t cycles = 0, bad = 0, position = 0;
    uint32_t pc = 0;
    bool pc_known = false;
    Taker(const rv32::Program &prog, const Ranges &ranges, uint32_t shard, uint32_t row)
        : rg(ranges), P(watch::position(shard, row)), stat(prog), sh(watch::shapes()), before(ranges.n_words, Side{}), after(ranges.n_words, Side{}), st(prog) {}
    // the records of shard `shard` (numbered from 1) and the pc the shard hands on
    void scan(const rv32::Program &prog, const rv32::CycleRec *recs, size_t n, uint32_t shard, uint32_t next_pc) {
        const uint32_t n_instr = (uint32_t)stat.n();
        const uint32_t p_shard = (uint32_t)(P >> 32), p_row = (uint32_t)P;
        const size_t n_pre = shard < p_shard ? n : shard == p_shard ? std::min<size_t>(n, p_row) : 0;   // the records of this shard before P
        for (size_t r = 0; r < n; r++) {
            const watch::Decoded d = watch::decode(recs[r], n_instr, prog.text_base, stat.statics(), stat.offs(), sh);
            if (d.bad) { bad++; continue; }
            const uint32_t rd = d.st & watch::ST_RD_MASK;
            if (r < n_pre) {
                if (rd) reg[rd] = side_of(recs[r], d, sh, shard, (uint32_t)r, rd, WHAT_REG);
                for_decided(rg, d, sh, [&](uint32_t slot, uint32_t addr) {
                    if (slot < before.size()) before[slot] = side_of(recs[r], d, sh, shard, (uint32_t)r, addr, WHAT_BEFORE);
                });
            } else
                for_decided(rg, d, sh, [&](uint32_t slot, uint32_t addr) {
                    if (slot < after.size() && after[slot].kind == SIDE_NONE) after[slot] = side_of(recs[r], d, sh, shard, (uint32_t)r, addr, WHAT_AFTER);
                });
        }
        if (n_pre < n && !pc_known) {
            pc_known = true;
            pc = prog.text_base + 4 * recs[n_pre].idx;
        }
        if (!pc_known) pc = next_pc;
        if (n_pre) {
            const uint64_t base = cycles;
            calltree::walk_records(prog, recs, n_pre, n_pre < n ? recs[n_pre].idx : prof::index_of_pc(prog, next_pc), base, &st);
            calls.resize(st.stack.size());
            for (size_t k = 0; k < st.stack.size(); k++) {   // the frames this shard opened: their call record is at open - 1
                const uint64_t open = st.stack[k].open;
                if (open <= base || open - 1 - base >= n_pre) continue;
                const rv32::CycleRec &call = recs[open - 1 - base];
                calls[k] = CallRec{prog.text_base + 4 * call.idx, call.a};
            }
            if (!calls.empty() && st.stack[0].open == 0) calls[0] = CallRec{};
        }
        position += n_pre;
        cycles += n;
        shard_n.push_back(n);
    }
    void emit(const rv32::Program &prog, double ms, dvt_snap_cell regs[32], dvt_snap_cell *words, dvt_snap_frame *frames, size_t cap_frames,
              dvt_snap_summary *summary) const {
        const Parts parts{reg, before.data(), after.data(), &st.stack, &calls, &shard_n, position, cycles, st.unmatched_returns, pc};
        snap::emit(prog, rg, parts, ms, regs, words, frames, cap_frames, summary);
    }
};

}  // namespace snap
}  // namespace dvt
