// The call-tree report (include/dvt_prover.h: dvt_rv32_job_calltree, dvt_execute_calltree): inclusive and self cycles per
// function and per caller -> callee arc, from the cycle records of an execution.  One rule, here in plain C++ for the host
// path and in calltree.hip for the records a prepared job holds in HBM.
//
// Records are taken in execution order over the whole execution, global position g = 0 .. C - 1 across shards.  The successor
// of a record is profile.h's.  Events come from the raw instruction word alone:
//   CALL   jal / jalr with rd == x1 (a CALL whose successor is NO_SUCC is no event)
//   RET    jalr with rd == x0, rs1 == x1, immediate 0
// Everything else (jal x0, jalr x0 through another register, branches) stays in the current frame: a tail jump is charged to
// the function that was called.  A function is named by the instruction index of its entry.  The stack starts with the root
// frame {fn = the instruction the first record names, open = 0, caller NO_FN}.
//   CALL at g, successor s    push {fn = s, open = g + 1, caller = top.fn}: the call instruction belongs to the caller
//   RET at g, depth > 1       pop F; the arc (F.caller, F.fn) gets calls += 1, cycles += g + 1 - F.open
//   RET at g, depth == 1      unmatched_returns += 1, the root stays
//   after the last record     every open frame is closed at position C, top first, the root last (its arc (NO_FN, entry)
//                             has cycles = C); open_at_exit counts them, the root included
// A RET pops the top frame whatever address it returns to: the rule follows the instruction stream, not the value of ra, so
// a guest that returns past a frame (longjmp style) or rewrites ra is attributed as if every `ret` left one function.
// Per function f: calls and inclusive are the sums over the arcs into f, self = inclusive - the cycles of the arcs out of f.
// Nested frames of one function count more than once in inclusive, never in self, and the self cycles of all functions sum
// to C.
#pragma once
#include <map>
#include <utility>
#include <vector>

#include "profile.h"

namespace dvt {
namespace calltree {

constexpr uint32_t NO_FN = 0xffffffffu;
// The class word per instruction: profile.h's (static target in bits 0..27, its class in 30..31) with the two event bits
// beside it.  (An index is below 2^28.)
constexpr uint32_t EV_CALL = 1u << 28, EV_RET = 1u << 29;
inline uint32_t event_of(uint32_t raw) {
    const uint32_t op = raw & 0x7f, rd = (raw >> 7) & 31;
    if ((op == 0x6f || op == 0x67) && rd == 1) return EV_CALL;
    if (op == 0x67 && rd == 0 && ((raw >> 15) & 31) == 1 && (raw >> 20) == 0) return EV_RET;
    return 0;
}
inline std::vector<uint32_t> instr_classes(const rv32::Program &prog) {
    std::vector<uint32_t> m = prof::instr_classes(prog);
    for (size_t i = 0; i < m.size(); i++) m[i] = (m[i] & ~(EV_CALL | EV_RET)) | event_of(prog.instrs[i].raw);
    return m;
}

struct Frame {
    uint32_t fn;
    uint64_t open;
};
struct Arc {
    uint64_t calls = 0, cycles = 0;
};
// the report while it is added up (functions by instruction index; the caller of stack[k] is stack[k - 1].fn)
struct State {
    std::vector<uint32_t> classes;
    std::vector<Frame> stack;
    std::map<std::pair<uint32_t, uint32_t>, Arc> arcs;
    uint64_t cycles = 0, dropped_frames = 0, dropped_cycles = 0, unmatched_returns = 0;
    uint32_t max_depth = 0, open_at_exit = 0;
    explicit State(const rv32::Program &prog) : classes(instr_classes(prog)) {}
    void close_top(uint64_t end) {
        const Frame f = stack.back();
        stack.pop_back();
        Arc &a = arcs[{stack.empty() ? NO_FN : stack.back().fn, f.fn}];
        a.calls++;
        a.cycles += end - f.open;
    }
    // after the last record: the frames still open end at `cycles`
    void finish() {
        open_at_exit = (uint32_t)stack.size();
        while (!stack.empty()) close_top(cycles);
    }
};

// the records of one shard, in execution order, the first of them at global position base_position; last_succ: the
// instruction index of the shard's next_pc or NO_SUCC
void walk_records(const rv32::Program &prog, const rv32::CycleRec *recs, size_t n, uint32_t last_succ, uint64_t base_position, State *st);

// the caller's arrays of both entry points
struct Out {
    dvt_calltree_arc *arcs; size_t cap_arcs;
    dvt_calltree_func *funcs; size_t cap_funcs;
    dvt_calltree_summary *summary;
    bool null_array() const { return (cap_arcs && !arcs) || (cap_funcs && !funcs); }
};
// a finished State into the caller's arrays: arcs by (caller_pc, callee_pc), functions by self descending, then by pc
void emit(const rv32::Program &prog, const State &st, uint32_t shards_total, double ms, const Out &out);

}  // namespace calltree
}  // namespace dvt
