// The execution report (include/dvt_prover.h: dvt_rv32_job_profile, dvt_execute_profile): how often every instruction retired,
// every control transfer was taken and every syscall was made, from the cycle records of an execution.  One rule per record,
// here in plain C++ for the host path and in profile.hip for the records a prepared job holds in HBM:
//   pc_count[rec.idx] += 1
//   the successor of a record is the next record's idx; of a shard's last record the instruction at the shard's next_pc
//   (NO_SUCC when that is none of the text: after HALT); a record with a successor other than idx + 1 is a transfer and
//   adds one to its edge (idx, successor)
//   an ECALL record adds one to the entry of its syscall id (rec.b = t0)
#pragma once
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/dvt_prover.h"
#include "rv32.h"

namespace dvt {
namespace prof {

constexpr uint32_t NO_SUCC = 0xffffffffu;
constexpr uint32_t MAX_SYSCALLS = 64;   // distinct syscall ids of one report
constexpr uint32_t MIN_LOG_SLOTS = 3, MAX_LOG_SLOTS = 24, DEFAULT_MIN_LOG_SLOTS = 10;

// What the device pass reads per instruction besides the records: bits 0..29 the index of the static target (branches, JAL),
// bits 30..31 the class.  (Addresses are below 2^30, so an index is below 2^28.)
constexpr uint32_t CLS_SHIFT = 30, TGT_MASK = (1u << CLS_SHIFT) - 1;
enum : uint32_t { CLS_OTHER = 0, CLS_ECALL = 1, CLS_STATIC = 2 };
inline std::vector<uint32_t> instr_classes(const rv32::Program &prog) {
    std::vector<uint32_t> m(prog.instrs.size() - 1);
    for (size_t i = 0; i < m.size(); i++) {
        const rv32::Instr &in = prog.instrs[i];
        const bool stat = in.kind == rv32::K_JAL || (in.kind >= rv32::K_BEQ && in.kind <= rv32::K_BGEU);
        m[i] = stat ? (CLS_STATIC << CLS_SHIFT) | (in.tgt_idx & TGT_MASK) : in.kind == rv32::K_ECALL ? CLS_ECALL << CLS_SHIFT : 0;
    }
    return m;
}
// instruction index of a pc, NO_SUCC when it is no instruction of the text
inline uint32_t index_of_pc(const rv32::Program &prog, uint32_t pc) {
    const uint32_t n = (uint32_t)prog.instrs.size() - 1, i = (pc - prog.text_base) >> 2;
    return pc >= prog.text_base && !(pc & 3) && i < n ? i : NO_SUCC;
}

// the tables of a report while they are added up (edges by instruction index)
struct Tally {
    std::vector<uint64_t> pc_count;
    std::map<std::pair<uint32_t, uint32_t>, uint64_t> edges;
    std::map<uint32_t, uint64_t> sys;
    uint64_t n_transfers = 0, dropped = 0;
    uint32_t shards = 0;
    explicit Tally(const rv32::Program &prog) : pc_count(prog.instrs.size() - 1, 0) {}
};

// the records of one shard, in execution order; last_succ: the instruction index of the shard's next_pc or NO_SUCC
void tally_records(const rv32::Program &prog, const rv32::CycleRec *recs, size_t n, uint32_t last_succ, Tally *t);

// the caller's arrays of both entry points
struct Out {
    uint64_t *pc_count; size_t cap_pc;
    dvt_profile_edge *edges; size_t cap_edges;
    dvt_profile_syscall *sys; size_t cap_sys;
    dvt_profile_opcode *ops; size_t cap_ops;
    dvt_profile_summary *summary;
    bool null_array() const { return (cap_pc && !pc_count) || (cap_edges && !edges) || (cap_sys && !sys) || (cap_ops && !ops); }
};
// the lowercase mnemonic of a raw instruction word ("unknown" when it is none of RV32IM, ecall or fence)
const char *mnemonic(uint32_t raw);
// a finished tally into the caller's arrays; false when it holds more than MAX_SYSCALLS syscall ids
bool emit(const rv32::Program &prog, const Tally &t, uint32_t shards_total, double ms, const Out &out);

}  // namespace prof
}  // namespace dvt
