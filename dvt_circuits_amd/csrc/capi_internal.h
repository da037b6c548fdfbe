// Private to the C-ABI layer: what capi.hip (the handle, the stage and machine-level entry points), capi_rv32.hip (the rv32 boundary:
// setup, the job of capi_job.h and its pipelines, prove, assemble, verify), capi_inspect.hip (the inspectors of trace rows) and
// capi_report.hip (the reports over a job's cycle records) share.
#pragma once
#include "../../include/dvt_prover.h"

#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>

#include "engine.h"
#include "rv32.h"

namespace dvt { namespace vq { struct Stage; void stage_free(Stage *); } }
constexpr int MAX_LANES = 3;
// Lanes that commit (phase 1) unless the handle's config says otherwise; capped at the handle's lanes, so every lane commits:
// two lanes beat one by 2.2-3.8 % per call in every A/B pair (profiles/README.md, round 6).
constexpr int PHASE1_LANES_DEFAULT = MAX_LANES;
constexpr int MAX_MEMBERS = 8;   // devices of one handle ("devices")

struct DeviceKey;
// what dvt_rv32_prove_shard is about to collect from a running phase-2 pipeline
struct PipeClaim {
    const dvt_job *job;
    const DeviceKey *pk;
    const uint32_t *ch;   // the challenges, canonical
    size_t shard;         // index into the shards of the member's part of the job
};

// Phase 2 of the shards a member holds of a job, run ahead of the caller on the member's prover lanes: one worker thread per
// lane takes the next shard in job order (that shard then stays on that lane), at most `lanes` shards past the last one the
// caller asked for.  Worker threads never touch p->err: each slot keeps its own result.  Everything here is guarded by mu;
// the API thread holds the prover's mutex while it creates, claims from or drains the pipeline.
struct Phase2Pipe {
    struct Slot {
        size_t shard = 0;               // index into the shards of the member's part
        int state = 0;                  // 0 waiting, 1 running, 2 done
        bool claimed = false;
        int rc = 0;
        std::string err;
        std::vector<uint32_t> words;
    };
    dvt_job *job = nullptr;
    const DeviceKey *pk = nullptr;
    uint32_t ch[8] = {};                // the challenges, canonical
    std::vector<Slot> slots;            // in proving order
    size_t next = 0;                    // the next slot a worker starts
    size_t limit = 0;                   // slots below this may start
    bool stop = false, failed = false;
    std::mutex mu;
    std::condition_variable cv;
    std::vector<std::thread> workers;

    // the unclaimed slot of the claimed shard when this pipeline proves that job under that key and those challenges, else -1
    long slot_of(const PipeClaim &c) const {
        if (c.job != job || c.pk != pk || memcmp(c.ch, ch, sizeof ch)) return -1;
        for (size_t i = 0; i < slots.size(); i++)
            if (slots[i].shard == c.shard) return slots[i].claimed ? -1 : (long)i;
        return -1;
    }
};

// What one device of a handle ("devices": [d0, d1, ...]) owns.  Settings are the handle's.
struct Member {
    size_t index = 0;                 // position in the handle
    dvt::Engine eng;                  // lane 0: phase 1 and phase 2 of the shards it takes; on member 0 also the stage entry points
    // Further prover lanes: own stream, ring, arena, pool and tables each, sharing the proving key's read-only device
    // buffers.  Lane k is created when phase 1 has a k-th shard waiting and no lane free for it (k < phase1_lanes), else on
    // the first job that has at least two shards to prove in phase 2.  A job of one shard never creates one.
    std::unique_ptr<dvt::Engine> more[MAX_LANES - 1];
    std::unique_ptr<Phase2Pipe> pipe;   // the phase-2 pipeline of the current job, if one runs (see Phase2Pipe)
    // record uploads overlap the lanes' kernels; with several phase-1 lanes the auxiliary uploads and their K0 launches too
    hipStream_t copy_stream = nullptr;
    // Pinned staging of everything a shard uploads besides its records (auxiliary traces, precompile calls).  Handing the
    // runtime PAGEABLE memory makes it pin the pages on the fly; when the vectors are freed afterwards the driver quiesces
    // every queue of the process to drop that mapping - measured as a 20-30 ms stall of the GPU right before phase 1 of a
    // single-shard proof.
    uint8_t *aux_pinned = nullptr;
    size_t aux_pinned_bytes = 0;
    bool shares_device = false;       // another member of the handle proves on the same physical device
};

struct dvt_prover {
    std::vector<std::unique_ptr<Member>> members;   // one per device, never empty; a one-device handle runs the one-device path
    int lanes = 2;                    // prover lanes of every member ("lanes")
    int phase1_lanes = 1;             // lanes that also commit (phase 1) inside a prepare, 1..lanes ("phase1_lanes")
    dvt::StarkConfig cfg;
    uint32_t log_shard = 21;          // cycles per shard = 2^log_shard (SP1's default shard size)
    uint64_t max_cycles = 1ull << 36;
    // what phase 1 keeps in HBM for phase 2 ("keep_phase1", keep_plan.h): 0 nothing (phase 2 recomputes), 1 K0 output, main LDEs
    // and tree while they fit, 2 the same, then the tree alone, then nothing
    int keep_phase1 = 1;
    int keep_full_max = -1;           // diagnostic ("keep_full_max"): shards kept in full per physical device and job at most; -1 = no cap
    uint32_t exec_threads = 0;        // trace-mode executor threads of the prove pipeline ("exec_threads", 0 = from the host's core count)
    std::vector<dvt::rv32::CycleRec *> pinned;    // pinned staging buffers of 2^log_shard records each, reused across calls
    // the device verifier's pinned staging and events (verify_query.hip, on member 0), made by the first dvt_prover_verify; its last times
    dvt::vq::Stage *vq_stage = nullptr;
    double vq_times[9] = {};
    double calltree_ms[3] = {};       // the last dvt_rv32_job_calltree: summary mode, the host's merge, emit mode (dvt_rv32_job_calltree_times)
    double watch_ms[4] = {};          // the last dvt_rv32_job_watch: count, scan and emit launches by stream events, the shards the emit pass ran over (dvt_rv32_job_watch_times)
    double snap_ms[3] = {};           // the last dvt_rv32_job_snapshot: reduce, gather and backtrace launches by stream events (dvt_rv32_job_snapshot_times)
    double diverge_ms[4] = {};        // the last dvt_rv32_job_diverge: classify, merge, emit + gather launches by stream events, the host's share (dvt_rv32_job_diverge_times)
    double uses_ms[5] = {};           // the last dvt_rv32_job_uses: next, count + scan, emit and gather launches by stream events, the host's share (dvt_rv32_job_uses_times)
    double origin_ms[3] = {};         // the last dvt_rv32_job_origin: reduce and gather launches by stream events, the host's share (dvt_rv32_job_origin_times)
    size_t vq_chunk_words = 0;       // proof words per chunk of the device verifier ("verify_chunk_words", default vq::CHUNK_WORDS)
    std::string err;
    std::mutex mu;
};

// a proving key on one member's device
struct DeviceKey {
    dvt::ProvingKey key;
    dvt::rv32::Instr *d_instrs = nullptr;   // device copy of prog.instrs (K0)
    uint32_t *d_prog_row = nullptr;    // instruction index -> program-table row
};
struct dvt_pk {
    bool is_rv32 = false;
    dvt::rv32::Program prog;
    dvt::rv32::HostPrep prep;
    std::vector<DeviceKey> dev;   // in member order; a machine-level key (dvt_machine_setup) has member 0's only
};

namespace dvt {   // (the helpers the two units share stay out of the library's global namespace)
inline size_t n_members(const dvt_prover *p) { return p->members.size(); }
inline Member &member(dvt_prover *p, size_t m) { return *p->members[m]; }
inline Engine &lane_engine(Member &mem, int k) { return k == 0 ? mem.eng : *mem.more[k - 1]; }
inline Engine &eng0(dvt_prover *p) { return p->members[0]->eng; }   // lane 0 of member 0: the stage and machine-level entry points
inline const DeviceKey &member_key(const dvt_pk *pk, size_t m) { return pk->dev[m]; }

// ---- errors: every message of the ABI layer goes through one formatter into one string
int fail(std::string &err, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
// into p->err; with p == nullptr into the calling thread's creation error (dvt_last_error(NULL))
int fail(dvt_prover *p, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
// an engine call failed: its message, as DVT_ERR_DEVICE
inline int engine_fail(std::string &err, const Engine &e) { return fail(err, DVT_ERR_DEVICE, "%s", e.err.c_str()); }
#define HIP_TRY(to, expr)                                                                              \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(to, DVT_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// every lane's stream of a member is idle (its device is current); the first error
hipError_t sync_lanes(Member &mem);
// Stops the pipeline of one member (running shards finish, nothing new starts; unclaimed results are discarded) and waits
// for every lane's stream.  With first_err != nullptr: the error of the lowest failed slot, if any.  Caller holds the
// handle's mutex.
int pipe_drain(Member &mem, std::string *first_err = nullptr);
// the same on every member of the handle (the API thread is left on member 0's device)
void pipe_drain_all(dvt_prover *p);
// The API thread turns to member m: its device becomes the calling thread's.
int select_member(dvt_prover *p, size_t m);
// the same before it touches a member; on a one-device handle the entry guard has done it
inline int turn_to(dvt_prover *p, size_t m) { return n_members(p) > 1 ? select_member(p, m) : DVT_OK; }

// Built first by every entry point that works on a handle: holds p->mu for the whole call, drains the phase-2 pipelines of
// every member and selects member 0's device (rc: DVT_ERR_DEVICE when that fails).  With a claim (dvt_rv32_prove_shard
// only, on member `claim_member`) pipelines that hold the claimed shard keep running, and `slot` is that shard's slot.
struct Guard {
    dvt_prover *p;
    std::lock_guard<std::mutex> lk;
    long slot = -1;
    int rc;
    explicit Guard(dvt_prover *p, const PipeClaim *claim = nullptr, size_t claim_member = 0);
    ~Guard() { if (n_members(p) > 1) (void)hipSetDevice(eng0(p).device); }   // (a call may have turned to another member)
};

// A lane's view of the prover for K0 and both phases: the handle (settings), the member, its engine, and the error string
// it reports to (p->err on the API thread; a worker thread's own string: worker threads never write p->err).  Passed as
// `const Lane &`: what it refers to stays writable.
struct Lane {
    dvt_prover *p;
    Member &mem;
    int k;
    Engine &eng;
    std::string &err;
};
inline Lane lane0(dvt_prover *p, size_t m = 0) { return {p, member(p, m), 0, member(p, m).eng, p->err}; }

// device scratch of an entry point from a lane's buffer cache, given back at scope exit (stream-ordered: the next user of a
// cached buffer runs on the same stream)
struct StageBuf {
    DevPool &pool;
    void *ptr = nullptr;
    ~StageBuf() { pool.free(ptr); }
};

// ---- the trace-row checks (check.cuh) of a list of chip tables that share their public values, on one lane:
// dvt_stage_check_constraints, dvt_stage_bus_sums and dvt_rv32_check_job go through this (capi_inspect.hip).  One download,
// which synchronises the lane's stream, for the whole list.
struct CheckTable {
    const ChipDesc *d;
    const uint32_t *main, *prep;   // device, Montgomery, column-major (prep may be null when the chip has no such column)
    uint32_t log_n;
};
struct CheckChallenges {
    Fp4 xi;                 // where the closed-form big-integer identities are evaluated
    Fp4 perm_alpha, beta;   // of the LogUp terms
};
struct CheckTableOut {
    dvt_check_result r;
    std::vector<uint32_t> counts;    // [n_constraints] rows violating each unit (with want_counts)
    Fp4 bus[DVT_CHECK_BUSES];        // the table's signed LogUp terms summed over its rows, by bus id
};
int check_tables(const Lane &c, const MachineDesc *m, const std::vector<CheckTable> &tabs, const std::vector<uint32_t> &pub_mont,
                 const CheckChallenges &ch, bool constraints, bool buses, std::vector<CheckTableOut> *out);

// ---- the arguments of the stage entry points that take one chip table: the checks of machine, chip, log_n, path, pub and the
// two LogUp challenges that K4 / K5 make (dvt_stage_perm, dvt_stage_quotient), and for the inspectors (capi_inspect.hip) the
// same checks and then the table's matrices; a call that has no challenges leaves them out
inline bool ext_from_canonical(const uint32_t w[4], Fp4 *out) {
    for (int k = 0; k < 4; k++) {
        if (w[k] >= P) return false;
        out->c[k] = Fp::from_canonical(w[k]);
    }
    return true;
}
struct ChipStageArgs {
    const MachineDesc *m = nullptr;
    const ChipDesc *d = nullptr;
    std::vector<uint32_t> pub;   // Montgomery words, at least one (the table's pub_mont)
    Fp4 perm_alpha, beta;
    int n_beta = 0, n_alpha = 0;   // challenge powers the machine's kernels read
    CheckTable t = {};             // (stage_table only)
};
int chip_stage_args(dvt_prover *p, const char *machine, uint32_t chip, uint32_t log_n, const uint32_t *pub, const uint32_t perm_alpha[4],
                    const uint32_t beta[4], uint32_t path, ChipStageArgs *out);
constexpr uint32_t NO_CHALLENGE[4] = {0, 0, 0, 0};
int stage_table(dvt_prover *p, const char *machine, uint32_t chip, const uint32_t *d_main, const uint32_t *d_prep, uint32_t log_n,
                const uint32_t *pub, ChipStageArgs *out, const uint32_t *perm_alpha = NO_CHALLENGE, const uint32_t *beta = NO_CHALLENGE);

// ---- the bus ledger (ledger.cuh) on one lane: dvt_stage_bus_ledger_* and dvt_rv32_job_bus_tuples go through this
// (ledger.hip).  Buffers come from the lane's pool and go back in ledger_release.
struct LedgerDev {
    uint32_t log_buckets = 0, cap_slots = 0;
    uint64_t seed = 0;
    DevPool *pool = nullptr;
    unsigned long long *d_tally = nullptr;   // [2^log_buckets][3]
    uint32_t *d_dirty = nullptr;             // [2^log_buckets / 32]
    uint32_t *d_flags = nullptr;             // dirty buckets, overflow
    void *d_slots = nullptr;                 // [cap_slots] records, made by the first COLLECT launch
};
int ledger_init(const Lane &c, LedgerDev *l, uint32_t log_buckets, uint32_t cap_slots, uint64_t seed);
void ledger_release(LedgerDev *l);
// one pass (mode: LEDGER_TALLY = 0, LEDGER_COLLECT = 1) over a chip table
int ledger_rows(const Lane &c, LedgerDev &l, const CheckTable &t, uint32_t chip, const std::vector<uint32_t> &pub_mont, uint32_t tag, uint32_t mode);
// a tuple the host adds (canonical values), keyed on the host
int ledger_tuple(const Lane &c, LedgerDev &l, uint32_t bus, const uint32_t *values, uint32_t arity, int sign, uint32_t mult, uint32_t tag, uint32_t mode);
int ledger_close(const Lane &c, LedgerDev &l, uint32_t *n_dirty);   // the bitmap on the device from the ledger's own tallies
// several ledgers of one shape and seed: their tallies to the host, the bitmap of the sum back to each
int ledger_tallies(const Lane &c, LedgerDev &l, std::vector<uint64_t> *out);
uint32_t ledger_dirty_of(const std::vector<uint64_t> &tallies, std::vector<uint32_t> *bitmap);
int ledger_set_dirty(const Lane &c, LedgerDev &l, const std::vector<uint32_t> &bitmap);
// appends the used records (balanced ones included); sets *overflow when an occurrence was dropped
int ledger_records(const Lane &c, LedgerDev &l, std::vector<dvt_bus_tuple> *out, bool *overflow);
// records of one tuple added up, the balanced ones dropped, the rest sorted by (bus, values)
void ledger_finish(std::vector<dvt_bus_tuple> *tuples);
// the caller's share of a finished list
inline void ledger_copy_out(const std::vector<dvt_bus_tuple> &all, bool overflow, dvt_bus_tuple *out, size_t cap, size_t *n_tuples, uint32_t *truncated) {
    const size_t n = std::min(all.size(), out ? cap : 0);
    for (size_t i = 0; i < n; i++) out[i] = all[i];
    *n_tuples = n;
    if (truncated) *truncated = overflow || n < all.size();
}

// ---- the forgery hunt (hunt.cuh) of one chip table on one lane: dvt_stage_hunt_cells, dvt_stage_hunt_pairs and
// dvt_rv32_hunt_shard go through this (hunt.hip).  Synchronises the lane's stream.
// One evaluation = one row evaluated for one candidate; a lane slot = one lane of a workgroup for one touched row, live or not
// (256 x touched rows per candidate and row block).  The rates per chip are measured in profiles/README.md ("Forgery hunt"):
// a launch is cut at 2^24 lane slots, which is a few milliseconds on the chips whose tables fill their workgroups and a
// fraction of a second on the slowest precompile chip; a call without a max_evals of its own stops at 2^33 evaluations, which
// admits the cpu chip's adjacent hunt over all 8192 rows of the smallest guest (8.2 10^9, under 3 s).
constexpr uint64_t HUNT_LAUNCH_EVALS = 1ull << 24, HUNT_DEFAULT_MAX_EVALS = 1ull << 33;
constexpr uint64_t HUNT_MAX_RECORDS = 1ull << 22;   // records a call brings back at most (include/dvt_prover.h)
struct HuntRequest {   // (filled member by member: see hunt_request)
    uint64_t seed = 0;
    const uint32_t *deltas = nullptr;   // canonical, 1 <= delta < p
    uint32_t n_deltas = 0;
    uint32_t row_first = 0, row_count = 0;
    uint64_t max_evals = 0;             // 0: HUNT_DEFAULT_MAX_EVALS
    uint32_t pairs = 0;                 // 0: single cells -> free_counts, free_map; 1: pairs -> out, n_reported, n_tried
    uint32_t *free_counts = nullptr;    // [main_w][n_deltas]
    uint8_t *free_map = nullptr;        // [n_deltas][main_w][row_count] or nullptr
    const uint32_t *cols = nullptr;     // pairs: the columns both cells are taken from (nullptr: every main column)
    uint32_t n_cols = 0, adjacent = 0;
    dvt_escape *out = nullptr;
    size_t cap = 0;
    uint64_t *n_reported = nullptr, *n_tried = nullptr;
};
// what every hunt has
inline HuntRequest hunt_request(uint64_t seed, const uint32_t *deltas, uint32_t n_deltas, uint32_t row_first, uint32_t row_count, uint64_t max_evals) {
    HuntRequest rq;
    rq.seed = seed; rq.deltas = deltas; rq.n_deltas = n_deltas;
    rq.row_first = row_first; rq.row_count = row_count; rq.max_evals = max_evals;
    return rq;
}
inline void hunt_want_cells(HuntRequest *rq, uint32_t *free_counts, uint8_t *free_map) {
    rq->pairs = 0; rq->free_counts = free_counts; rq->free_map = free_map;
}
inline void hunt_want_pairs(HuntRequest *rq, const uint32_t *cols, uint32_t n_cols, uint32_t adjacent, dvt_escape *out, size_t cap, uint64_t *n_reported,
                            uint64_t *n_tried) {
    rq->pairs = 1; rq->cols = cols; rq->n_cols = n_cols; rq->adjacent = adjacent;
    rq->out = out; rq->cap = cap; rq->n_reported = n_reported; rq->n_tried = n_tried;
}
// what a checked request comes to: made once per call by hunt_plan, read by hunt_table
struct HuntPlan {
    std::vector<uint32_t> cols;    // the columns the cells are taken from, sorted, each once
    std::vector<uint32_t> pairs;   // positions in cols, k0 | k1 << 16
    uint32_t map_rows = 0;         // window indices of the single-cell map
    uint64_t cell_evals = 0, pair_evals = 0;
};
// the DVT_ERR_INPUT / DVT_ERR_UNSUPPORTED cases of a request (nothing is launched), and its plan
int hunt_plan(std::string &err, const ChipDesc &d, uint32_t log_n, const HuntRequest &rq, HuntPlan *out);
int hunt_table(const Lane &c, const MachineDesc *m, const CheckTable &t, const std::vector<uint32_t> &pub_mont, const HuntRequest &rq,
               const HuntPlan &plan);

// ---- the join hunt (hunt_join.cuh) over windows of several tables on one lane: dvt_stage_hunt_join_* go through this
// (hunt_join.hip).  Buffers come from the lane's pool and go back in join_release.  The bounds of a launch and of a call are
// the hunt's (HUNT_LAUNCH_EVALS, HUNT_DEFAULT_MAX_EVALS, HUNT_MAX_RECORDS).
struct JoinSupplyRef {   // a supply table, kept until the first window is added: the set is sized and built then
    const ChipDesc *d;
    const uint32_t *main, *prep;
    uint32_t log_n;
    std::vector<uint32_t> pub_mont;
};
struct JoinInstance {    // a hunted (tag, chip) and its windows [first, first + count)
    uint32_t tag, chip, log_n;
    std::vector<std::pair<uint32_t, uint32_t>> windows;
};
struct JoinDev {
    const MachineDesc *m = nullptr;
    uint64_t seed = 0;
    uint32_t n_deltas = 0, deltas[DVT_HUNT_MAX_DELTAS] = {};   // canonical
    size_t cap_open = 0, cap_absorbed = 0;
    uint32_t log_slots = 0;
    DevPool *pool = nullptr;
    void *d_open = nullptr, *d_absorbed = nullptr, *d_counters = nullptr, *d_flags = nullptr, *d_supply = nullptr;
    uint32_t supply_mask = 0;
    std::vector<JoinSupplyRef> supply;
    std::vector<JoinInstance> instances;
    bool sealed = false;    // a window was added: no further supply table
    bool matched = false;
    bool broken = false;    // a window failed after its first launch: its records are in the arrays, add and match are refused
    dvt_join_summary summary = {};
    std::vector<dvt_join_cell> cells, absorbed;   // what match found, in the result's order
};
// the DVT_ERR_INPUT cases of new (nothing is allocated), then the buffers
int join_check_new(std::string &err, uint32_t n_deltas, const uint32_t *deltas, size_t cap_records, size_t cap_absorbed, uint32_t log_slots);
int join_init(const Lane &c, JoinDev *j, const MachineDesc *m, uint64_t seed, const uint32_t *deltas, uint32_t n_deltas, size_t cap_records,
              size_t cap_absorbed, uint32_t log_slots);
void join_release(JoinDev *j);
int join_supply(std::string &err, JoinDev &j, const CheckTable &t, const std::vector<uint32_t> &pub_mont);
// the DVT_ERR_INPUT / DVT_ERR_UNSUPPORTED cases of a window (nothing is launched); *cols_out: its columns, sorted, each once
int join_check_add(std::string &err, const JoinDev &j, uint32_t tag, uint32_t chip, const ChipDesc &d, uint32_t log_n, uint32_t row_first,
                   uint32_t row_count, const uint32_t *cols, uint32_t n_cols, uint64_t max_evals, std::vector<uint32_t> *cols_out);
int join_add(const Lane &c, JoinDev &j, uint32_t tag, uint32_t chip, const CheckTable &t, const std::vector<uint32_t> &pub_mont, uint32_t row_first,
             uint32_t row_count, const std::vector<uint32_t> &cols);
int join_match(const Lane &c, JoinDev &j);

// a library-allocated copy of w (release with dvt_free); *len = its bytes
inline uint8_t *copy_out(const std::vector<uint32_t> &w, size_t *len) {
    uint8_t *b = (uint8_t *)malloc(w.size() * 4 + 1);
    if (!b) return nullptr;
    memcpy(b, w.data(), w.size() * 4);
    *len = w.size() * 4;
    return b;
}
// the one teardown of a proving key, complete or half built by a setup
void pk_release(dvt_prover *p, dvt_pk *pk);
// the end of every setup: with rc == DVT_OK the vk (when asked for) and the key go to the caller; otherwise, or when the vk
// cannot be copied out, the key is released.  Returns the setup's code.
int setup_finish(dvt_prover *p, dvt_pk *pk, int rc, dvt_pk **pk_out, uint8_t **vk, size_t *vk_len);
// the verifying key's encoding ("DVK1")
std::vector<uint32_t> vk_words(const VerifyingKey &vk);
bool vk_parse(const uint8_t *b, size_t len, VerifyingKey *vk);
// verify entry points: the reason (strdup'ed, when the caller asks for one) and the code
inline int reject(char **reason, int code, const std::string &why) {
    if (reason) *reason = strdup(why.c_str());
    return code;
}
// Their common part: the proof's bytes as words, read by `check` (a reader over the words, the reason to fill -> a code)
// inside a try-block: a malformed proof throws, and its message is the reason.
int verify_words(const uint8_t *proof, size_t len, int len_code, char **reason,
                 const std::function<int(WordReader &, std::string &)> &check);
// The query part of the shards of one verify call on lane 0 of member 0 (verify_query.hip), behind an interface the two
// verify entry points share: add() after a shard's host part has passed, finish() once, then why() per shard.  A device
// failure is kept in rc (its text in p->err) and makes every later call a no-op.
struct DeviceQueries {
    explicit DeviceQueries(dvt_prover *p);
    ~DeviceQueries();
    void add(const ShardQueryCtx &ctx, const uint32_t *words, size_t nwords);
    void finish(double host_ms);
    std::string why(size_t shard) const;
    int rc = 0;
    dvt_prover *p;
    void *batch;
};
}  // namespace dvt

// a join hunt of the stage entry points (dvt_stage_hunt_join_*): on lane 0 of member 0
struct dvt_hunt_join {
    dvt::JoinDev dev;
};
// a bus ledger of the stage entry points (dvt_stage_bus_ledger_*): on lane 0 of member 0
struct dvt_bus_ledger {
    dvt::LedgerDev dev;
    const dvt::MachineDesc *m = nullptr;
    bool closed = false;       // TALLY is over: add is refused, collect and result are allowed
    uint32_t n_dirty = 0;      // what close found
};
