// The data-flow rule of the origin search (origin.h) and the uses search (uses.h), stated once for the host and the device:
// which registers and words a cycle record WRITES and which it READS.  The kernels of origin.hip and uses.hip, the two host
// searches and their Keepers all go through the two visitors below; the words of a precompile call come from
// memrep::for_call_words, as they do for watch::call_match and snap::for_decided.
//
//   for_written   rd when non-zero (so ECALL writes t0); the word of a store (sw / sh / sb); every PRE_WRITE word of a call, in
//                 call_match order.  Loads are no writers.
//   for_read      in this order: ADDR (loads and stores: rs1, only with FOLLOW_ADDR), RS1 (every other instruction whose decode
//                 sets F_RS1_EN, except ECALL), RS2 (F_RS2_EN and not ECALL; of a store the data), MEM (the word of a load; of a
//                 sb / sh, whose kept bytes come from the earlier word; never of a sw), MEM for every word a call reads, in
//                 call_match order.  A register x0 is never visited.
// A bad record (watch.h) writes and reads nothing.  What the two searches share on the host follows: the kind and the fields of a
// node, the checks of a call's target, and the records a host path keeps of an execution.
#pragma once
#include <string>

#include "snapshot.h"

namespace dvt {
namespace flow {

// What the rule reads per instruction besides watch::Statics: the source registers and whether the instruction reads them.
enum : uint32_t { OS_RS1_MASK = 31, OS_RS2_SHIFT = 5, OS_RS1_EN = 1u << 10, OS_RS2_EN = 1u << 11 };

// the shape of a record that is a precompile call, else nullptr
DVT_HD const memrep::PreShape *call_shape(const watch::Decoded &d, const watch::Shapes &sh) {
    return !d.bad && !d.dir && d.shape >= 0 && d.shape < (int)memrep::MAX_PRE ? &sh.s[d.shape] : nullptr;
}

// every target the record writes, in the rule's order: f(DVT_ORIGIN_REG | _WORD, target).  words: false leaves the words out, for a
// pass that asks about registers only (a call has up to 72 of them).
template <class F>
DVT_HD void for_written(const watch::Decoded &d, const watch::Shapes &sh, bool words, F f) {
    if (d.bad) return;
    if (const uint32_t rd = d.st & watch::ST_RD_MASK) f((uint32_t)DVT_ORIGIN_REG, rd);
    if (!words) return;
    if (d.dir == DVT_WATCH_STORE) f((uint32_t)DVT_ORIGIN_WORD, d.addr);
    if (const memrep::PreShape *ps = call_shape(d, sh))
        memrep::for_call_words(*ps, d.a0, d.a1, [&](uint32_t addr, bool, bool written) {
            if (written) f((uint32_t)DVT_ORIGIN_WORD, addr);
        });
}

// the inputs of the record that are no words of a call, in the rule's order: f(role, DVT_ORIGIN_REG | _WORD, target).
// ow: the record's word of Statics; flags: DVT_ORIGIN_FOLLOW_ADDR or 0; words: as for_written.
template <class F>
DVT_HD void for_read_direct(const watch::Decoded &d, uint32_t ow, uint32_t flags, bool words, F f) {
    if (d.bad) return;
    const uint32_t rs1 = ow & OS_RS1_MASK, rs2 = ow >> OS_RS2_SHIFT & 31;
    const bool ecall = (d.st & watch::ST_ECALL) != 0, mem = (d.st & (watch::ST_LOAD | watch::ST_STORE)) != 0;
    if (mem) {
        if ((flags & DVT_ORIGIN_FOLLOW_ADDR) && rs1) f((uint32_t)DVT_ORIGIN_ADDR, (uint32_t)DVT_ORIGIN_REG, rs1);
    } else if (!ecall && (ow & OS_RS1_EN) && rs1)
        f((uint32_t)DVT_ORIGIN_RS1, (uint32_t)DVT_ORIGIN_REG, rs1);
    if (!ecall && (ow & OS_RS2_EN) && rs2) f((uint32_t)DVT_ORIGIN_RS2, (uint32_t)DVT_ORIGIN_REG, rs2);
    if (words && (d.dir == DVT_WATCH_LOAD || (d.dir && (d.st & (watch::ST_HALF | watch::ST_BYTE))))) f((uint32_t)DVT_ORIGIN_MEM, (uint32_t)DVT_ORIGIN_WORD, d.addr);
}
// every input of the record
template <class F>
DVT_HD void for_read(const watch::Decoded &d, uint32_t ow, const watch::Shapes &sh, uint32_t flags, bool words, F f) {
    for_read_direct(d, ow, flags, words, f);
    if (!words) return;
    if (const memrep::PreShape *ps = call_shape(d, sh))
        memrep::for_call_words(*ps, d.a0, d.a1, [&](uint32_t addr, bool read, bool) {
            if (read) f((uint32_t)DVT_ORIGIN_MEM, (uint32_t)DVT_ORIGIN_WORD, addr);
        });
}

}  // namespace flow

// What a pass of origin.hip or uses.hip over sorted questions takes by value (kernels.h declares the launches).  The questions
// are sorted (origin::sorts_before): target / pos [n], n <= DVT_ORIGIN_PASS_QUESTIONS; the questions of register k are [reg_off[k], reg_off[k + 1]),
// the word questions [reg_off[32], n).
struct PassArgs {
    watch::Shapes sh;
    const uint32_t *statics, *offs;   // [n_instr], device
    const uint32_t *target;           // device
    const unsigned long long *pos;    // device: Q of a question, F of a definition
    uint32_t reg_off[33];
    uint32_t n_instr, text_base, shard, n;
};
// what a launch checks of them: the arrays are there, the offsets ascend from 0 and end within n
inline bool pass_ok(const PassArgs &a) {
    if (!a.n_instr || !a.statics || !a.offs || a.sh.n > memrep::MAX_PRE || !a.n || a.n > DVT_ORIGIN_PASS_QUESTIONS || !a.target || !a.pos) return false;
    for (uint32_t k = 0; k < 32; k++)
        if (a.reg_off[k] > a.reg_off[k + 1]) return false;
    return a.reg_off[0] == 0 && a.reg_off[32] <= a.n;
}

namespace flow {

// does the record write (what, target)?
inline bool writes(const watch::Decoded &d, const watch::Shapes &sh, uint32_t what, uint32_t target) {
    bool yes = false;
    for_written(d, sh, true, [&](uint32_t w, uint32_t t) { yes = yes || (w == what && t == target); });
    return yes;
}

// ---------------------------------------------------------------- host only
struct Statics {
    std::vector<uint32_t> words;
    explicit Statics(const rv32::Program &prog) : words(prog.instrs.size() - 1) {
        for (size_t i = 0; i < words.size(); i++) {
            const rv32::Instr &in = prog.instrs[i];
            words[i] = (in.rs1 & OS_RS1_MASK) | (in.rs2 & 31) << OS_RS2_SHIFT | (in.flags >> rv32::F_RS1_EN & 1 ? OS_RS1_EN : 0) |
                       (in.flags >> rv32::F_RS2_EN & 1 ? OS_RS2_EN : 0);
        }
    }
};

// the kind of the node a record makes (DVT_ORIGIN_* = DVT_USES_*)
inline uint32_t kind_of(const watch::Decoded &d) {
    return d.st & watch::ST_LOAD ? DVT_ORIGIN_LOAD : d.st & watch::ST_STORE ? DVT_ORIGIN_STORE : !(d.st & watch::ST_ECALL) ? DVT_ORIGIN_OP :
           d.shape >= 0 ? DVT_ORIGIN_CALL : DVT_ORIGIN_SYSCALL;
}
// the fields a dvt_origin_node and a dvt_uses_node share, of the record at pos
template <class Node>
Node node_of(unsigned long long pos, const watch::Decoded &d, const rv32::CycleRec &rec, uint32_t depth) {
    Node n{};
    n.shard = (uint32_t)(pos >> 32); n.row = (uint32_t)pos; n.pc = d.pc; n.idx = rec.idx; n.depth = depth;
    n.kind = kind_of(d);
    n.rd_value = rec.a; n.rs1 = rec.b; n.rs2 = rec.c;
    if (d.dir) { n.addr = d.addr; n.before = d.before; n.after = d.after; }
    return n;
}

// nullptr, or what is wrong with the target, the flags or the depth of a call
inline const char *target_error(uint32_t what, uint32_t target, uint32_t flags, uint32_t max_depth, uint32_t depth_limit, std::string *text) {
    if (what == DVT_ORIGIN_REG) {
        if (target < 1 || target > 31) return (*text = "register " + std::to_string(target) + " outside 1..31").c_str();
    } else if (what == DVT_ORIGIN_WORD) {
        if (target & 3) return (*text = "word address not 4-aligned").c_str();
        if (target >= rv32::ADDR_LIMIT) return (*text = "word address at or past the address limit").c_str();
    } else
        return (*text = "unknown target kind " + std::to_string(what)).c_str();
    if (flags & ~(uint32_t)DVT_ORIGIN_FOLLOW_ADDR) return (*text = "unknown flag").c_str();
    if (max_depth > depth_limit) return (*text = "max_depth " + std::to_string(max_depth) + " (at most " + std::to_string(depth_limit) + ")").c_str();
    return nullptr;
}

// What a host path keeps of the shards of an execution around the position P: the records before P (origin) or those at and
// after it (uses), and what the summary says of P.
struct Keeper {
    static constexpr uint64_t MAX_KEPT = (uint64_t)1 << 24;
    unsigned long long P;
    bool before;
    watch::Statics wst;
    watch::Shapes sh;
    Statics ost;
    std::vector<std::vector<rv32::CycleRec>> kept;   // kept[k]: the kept records of shard k + 1, from its row first_row[k] on
    std::vector<uint32_t> first_row;
    std::vector<uint64_t> shard_n;
    uint64_t cycles = 0, position = 0, n_kept = 0, bad = 0;
    bool too_many = false;
    Keeper(const rv32::Program &prog, uint32_t shard, uint32_t row, bool before)
        : P(watch::position(shard, row)), before(before), wst(prog), sh(watch::shapes()), ost(prog) {}
    watch::Decoded decode(const rv32::Program &prog, const rv32::CycleRec &rec) const {
        return watch::decode(rec, (uint32_t)wst.n(), prog.text_base, wst.statics(), wst.offs(), sh);
    }
    // the records of shard `shard` (numbered from 1, in order)
    void scan(const rv32::Program &prog, const rv32::CycleRec *recs, size_t n, uint32_t shard) {
        const uint32_t p_shard = (uint32_t)(P >> 32), p_row = (uint32_t)P;
        const size_t n_pre = shard < p_shard ? n : shard == p_shard ? std::min<size_t>(n, p_row) : 0;
        const size_t lo = before ? 0 : n_pre, hi = before ? n_pre : n;
        if (n_kept + (hi - lo) > MAX_KEPT) too_many = true;
        kept.resize(shard);
        first_row.resize(shard, 0);
        first_row[shard - 1] = (uint32_t)lo;
        if (hi > lo && !too_many) {
            kept[shard - 1].assign(recs + lo, recs + hi);
            for (size_t r = lo; r < hi; r++) bad += decode(prog, recs[r]).bad;
        }
        n_kept += hi - lo;
        position += n_pre;
        cycles += n;
        shard_n.push_back(n);
    }
    // position, cycles, shard, row and shards_total of a summary
    template <class Summary>
    void place(Summary *s) const {
        s->position = position; s->cycles = cycles;
        snap::locate(shard_n, position, &s->shard, &s->row);
        s->shards_total = (uint32_t)shard_n.size();
    }
};

}  // namespace flow
}  // namespace dvt
