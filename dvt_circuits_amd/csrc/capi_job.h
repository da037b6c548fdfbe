// Private to the rv32-aware units of the C-ABI layer: the prepared job capi_rv32.hip makes and proves, whose trace rows
// capi_inspect.hip reads and whose cycle records capi_report.hip reads.
#pragma once
#include <chrono>

#include "capi_internal.h"

namespace dvt {
constexpr uint32_t N_PUB = rv32::N_PUBLIC;           // start_pc, next_pc, exit_code, shard, is_last
constexpr uint32_t HEADER_WORDS = 8 + N_PUB;         // per-shard commitment header: main root + public values (canonical)
constexpr uint32_t PV_BUS = 5;                       // tools/airgen/rv32.py BUSES["sys"]
using Clock = std::chrono::steady_clock;
inline double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

struct ShardJob {
    uint32_t index = 0;       // shard number (1-based) = position in the execution + 1
    size_t n_recs = 0;
    uint32_t next_pc = 0;
    rv32::CycleRec *d_recs = nullptr;
    uint32_t log_n[rv32::N_CHIPS] = {};
    bool present[rv32::N_CHIPS] = {};
    uint32_t *d_aux[rv32::N_CHIPS] = {};  // main traces except cpu
    uint32_t device_rows = 1u << RV32_CHIP_CPU;   // bit c: the rows of chip c were (and on every K0 are) built on the GPU from events
    std::vector<Fp> pubs;
    MainCache cache;  // phase-1 LDEs + tree of the main traces (or the tree alone), consumed by phase 2
    // K0 output of this shard kept from phase 1 to phase 2 (with a full cache, while HBM allows); otherwise (tree-only
    // cache or none) the job's working buffers are used and phase 2 runs K0 again
    uint32_t *d_cpu = nullptr, *d_byte = nullptr, *d_prog = nullptr;
    bool traces_valid = false;
    int kept = -1;            // the tier of the last phase 1 (KEEP_*, keep_plan.h): what the shard holds in HBM until the job is freed; -1 before
    int lane = 0;             // the lane that first committed the shard: cache and kept K0 output are from its pool
    uint32_t header[HEADER_WORDS] = {};
    bool header_valid = false;   // phase 1 ran (inside the prepare pipeline, or by commit_shard) and no phase 2 has consumed it
};
// the shards of a job that one member of the handle holds (first, first + stride, ... of the execution), resident in that
// member's HBM, ready for K0..K9
struct JobPart {
    size_t first = 0, stride = 1;
    std::vector<ShardJob> shards;
    struct Work {   // K0 working buffers of one lane (largest shard seen), from that lane's pool
        uint32_t *d_cpu = nullptr, *d_byte = nullptr, *d_prog = nullptr;
        uint32_t log_cpu = 0;
    } work[MAX_LANES];
    double t_exec_wait = 0;   // seconds the member's GPU thread spent waiting for the executor inside prepare
    ShardJob *at(size_t pos) { return pos >= first && (pos - first) % stride == 0 && (pos - first) / stride < shards.size() ? &shards[(pos - first) / stride] : nullptr; }
};
// The one wrong-handle check of the entry points that take a key and/or a job (either may be null): both were made by a
// handle with as many members as this one, so member m finds its DeviceKey and its JobPart.
int same_members(dvt_prover *p, const dvt_pk *pk, const dvt_job *j);
// the check of every entry point that takes an rv32 key
inline int rv32_key(dvt_prover *p, const dvt_pk *pk) { return pk->is_rv32 ? DVT_OK : fail(p, DVT_ERR_INPUT, "proving key was not made by dvt_setup"); }
// One pass over the members of the handle: fn(m, lane 0 of member m) -> int under member m's turn, until one returns non-zero.
// Then member 0's device is current again; DVT_ERR_DEVICE when that fails and nothing else did.
template <class Fn>
int for_members(dvt_prover *p, Fn fn) {
    int rc = DVT_OK;
    for (size_t m = 0; m < n_members(p) && !rc; m++) {
        rc = turn_to(p, m);
        if (!rc) rc = fn(m, lane0(p, m));
    }
    if (turn_to(p, 0) && !rc) rc = DVT_ERR_DEVICE;
    return rc;
}
// K0 of a shard (into the shard's own buffers when it has them, else the job's working buffers); fills the chip
// trace list of that shard.  `reuse`: phase 2 takes the traces phase 1 left behind instead of generating them again.
int shard_traces(const Lane &c, const DeviceKey &key, dvt_job *j, ShardJob &s, std::vector<ChipTrace> *traces, bool reuse);
// The receiving side of the COMMIT rows' sys-bus tuples, from the claimed public-value bytes: an SP1 guest commits
// the eight words of SHA-256(public-value bytes) with COMMIT(k, word k); the cpu chip sends
// (t0 bytes = 0x10 0 0 0, a0 bytes = k 0 0 0, a1 bytes = the bytes of digest word k, 0, 0), tuple k contributes
// 1 / (alpha + bus + beta 0x10 + beta^5 k + beta^9 b0 + ... + beta^12 b3).  What the LogUp sums of all chips and shards
// must add up to (the verifier), and the sys bus alone (the job check).
Fp4 commit_digest_term(const PermChallenges &gc, const std::vector<uint8_t> &public_values);
}  // namespace dvt

// One prepared execution, cut into shards by the executor.  Of the shards this job holds (first, first + stride, ...) the
// k-th lives on member k mod G of the handle that prepared it: parts[m] is member m's (first + m stride, then G stride apart).
struct dvt_job {
    int exit_code = -1;
    uint64_t cycles = 0;
    std::vector<uint8_t> public_values;
    size_t n_total = 0, first = 0, stride = 1;   // shards of the execution / which of them this job holds
    size_t byte_words = 0, prog_words = 0;
    double t_exec_wait = 0;   // the longest executor wait of a member
    std::vector<dvt::JobPart> parts;   // one per member
    // Per physical device (index & 63, as the devices' turns): the shards its members have committed in the prepare, and the
    // shards of this job kept in full on it.  Written at the admission of a shard (shard_commit), under the device's turn
    // whenever another thread commits on the device.
    struct DeviceTally { size_t committed = 0, full = 0; } tally[64];
    size_t held() const {
        size_t n = 0;
        for (auto &q : parts) n += q.shards.size();
        return n;
    }
    // the shard at pos and the member that holds it; nullptr when this job does not hold it
    dvt::ShardJob *at(size_t pos, size_t *m) {
        if (pos < first || (pos - first) % stride) return nullptr;
        *m = (pos - first) / stride % parts.size();
        return parts[*m].at(pos);
    }
};
