// The inspectors of trace rows of the C ABI (include/dvt_prover.h): row checks, bus ledger, forgery hunt, join hunt.  Each has
// stage entry points (dvt_stage_*) on a table the caller uploaded (stage_table) and job entry points (dvt_rv32_*) on the
// tables of a prepared job's held shards (shard_view).  The execution report (profile.h), the call-tree report (calltree.h)
// and the memory report (memreport.h) are the inspectors that read a job's cycle records instead of its tables; the watchpoint
// search (watch.h) reads the same records and returns the ones that match; the snapshot (snapshot.h) reduces them to the state
// of the machine at one position.
#include <algorithm>
#include <type_traits>

#include "calltree.h"
#include "capi_job.h"
#include "ledger_key.h"
#include "memreport.h"
#include "profile.h"
#include "sha256.h"
#include "snapshot.h"
#include "watch.h"

using namespace dvt;

int dvt::check_tables(const Lane &c, const MachineDesc *m, const std::vector<CheckTable> &tabs, const std::vector<uint32_t> &pub_mont,
                 const CheckChallenges &ch, bool constraints, bool buses, std::vector<CheckTableOut> *out) {
    Engine &e = c.eng;
    constexpr size_t BW = 4 * DVT_CHECK_BUSES;
    // result words: one 64-bit key per table, then per table its counts and its bus sums
    std::vector<size_t> at(tabs.size());
    size_t words = 2 * tabs.size();
    for (size_t i = 0; i < tabs.size(); i++) {
        if (!tabs[i].d->launch_check || !tabs[i].d->launch_bus) return fail(c.err, DVT_ERR_UNSUPPORTED, "chip %s has no trace-row check", tabs[i].d->name);
        at[i] = words;
        words += (size_t)tabs[i].d->n_constraints + BW;
    }
    out->assign(tabs.size(), CheckTableOut{});
    for (auto &o : *out) {
        o.r = dvt_check_result{0, 0, -1};
        for (auto &b : o.bus) b = Fp4::zero();
    }
    if (tabs.empty()) return DVT_OK;
    StageBuf res{e.pool}, partial{e.pool};
    HIP_TRY(c.err, e.pool.alloc_bytes(&res.ptr, words * 4));
    if (buses) HIP_TRY(c.err, e.pool.alloc_bytes(&partial.ptr, BUS_PARTIAL_WORDS * 4));
    uint32_t *d_res = static_cast<uint32_t *>(res.ptr);
    HIP_TRY(c.err, hipMemsetAsync(d_res, 0xff, 8 * tabs.size(), e.stream));
    HIP_TRY(c.err, hipMemsetAsync(d_res + 2 * tabs.size(), 0, (words - 2 * tabs.size()) * 4, e.stream));
    int n_beta, n_alpha;
    challenge_power_counts(m, &n_beta, &n_alpha);
    const Fp4 *d_xi = nullptr, *d_beta = nullptr;
    const double *d_xi_f64 = nullptr, *d_beta_f64 = nullptr;
    const uint32_t *d_pub = static_cast<const uint32_t *>(e.upload_vec(pub_mont));
    if (!d_pub || (constraints && !e.upload_powers(ch.xi, (size_t)n_alpha, true, &d_xi, &d_xi_f64)) ||
        (buses && !e.upload_powers(ch.beta, (size_t)n_beta, false, &d_beta, &d_beta_f64)))
        return engine_fail(c.err, e);
    for (size_t i = 0; i < tabs.size(); i++) {
        const CheckTable &t = tabs[i];
        if (constraints) {
            const CheckArgs ca{t.main, t.prep, d_pub, d_xi, d_xi_f64, t.log_n, d_res + at[i], reinterpret_cast<unsigned long long *>(d_res) + i};
            HIP_TRY(c.err, t.d->launch_check(e.stream, ca));
        }
        if (buses) {
            const BusArgs ba{t.main, t.prep, d_pub, d_beta_f64, ch.perm_alpha, t.log_n, static_cast<uint32_t *>(partial.ptr), d_res + at[i] + t.d->n_constraints};
            HIP_TRY(c.err, t.d->launch_bus(e.stream, ba));
        }
    }
    std::vector<uint32_t> h(words);
    if (!e.download(h.data(), d_res, words * 4)) return engine_fail(c.err, e);
    for (size_t i = 0; i < tabs.size(); i++) {
        CheckTableOut &o = (*out)[i];
        const uint32_t *cw = h.data() + at[i];
        o.counts.assign(cw, cw + tabs[i].d->n_constraints);
        for (uint32_t x : o.counts) o.r.violations += x;
        const uint64_t key = (uint64_t)h[2 * i] | ((uint64_t)h[2 * i + 1] << 32);
        if (key != CHECK_NO_KEY) { o.r.first_row = (uint32_t)(key >> 32); o.r.first_constraint = (int32_t)(uint32_t)key; }
        for (uint32_t b = 0; b < DVT_CHECK_BUSES; b++)
            for (int k = 0; k < 4; k++) o.bus[b].c[k] = Fp::raw(cw[tabs[i].d->n_constraints + 4 * b + k]);
    }
    return DVT_OK;
}

// ------------------------------------------------------------------ the tables of a held shard
// What every job-level inspector reads, on lane 0 of the member that holds the shard (its device is current): the chip tables
// as phase 2 would take them, each with its preprocessed trace from the proving key.  The job stays as found.  The next K0 on
// the lane may write the buffers a view points into: the caller synchronises the lane's stream before the next shard's view.
struct ShardView {
    std::vector<ChipTrace> traces;
    std::vector<CheckTable> tabs;   // parallel to traces
    std::vector<uint32_t> pub_mont;
    const CheckTable *table(uint32_t chip) const {   // nullptr: the shard has no table of that chip
        for (size_t i = 0; i < tabs.size(); i++)
            if (traces[i].chip_id == (int)chip) return &tabs[i];
        return nullptr;
    }
};
static int shard_view(const Lane &c, const DeviceKey &key, dvt_job *j, ShardJob &s, size_t pos, ShardView *out) {
    *out = {};
    const bool kept = s.traces_valid;
    const int rc = shard_traces(c, key, j, s, &out->traces, true);
    s.traces_valid = kept;   // (K0 into a kept buffer whose content had been consumed: the job stays as it was found)
    if (rc) return rc;
    for (auto &t : out->traces) {
        const ChipDesc &d = machine_rv32()->chips[t.chip_id];
        const uint32_t *prep = nullptr;
        for (auto &pr : key.key.prep)
            if (pr.chip_id == t.chip_id && pr.log_n == t.log_n) prep = pr.d_trace;
        if (d.prep_w && !prep) return fail(c.err, DVT_ERR_INPUT, "chip %s of shard %zu has no preprocessed trace of its height in the proving key", d.name, pos);
        out->tabs.push_back({&d, t.d_main, prep, t.log_n});
    }
    for (auto x : s.pubs) out->pub_mont.push_back(x.v);
    return DVT_OK;
}

// ------------------------------------------------------------------ the job check (dvt_rv32_check_job)
// The point of the closed-form identities and the LogUp challenges of a check: a transcript over a domain tag, the key, the
// job's public-value bytes and its shard count.  Not the headers: the check needs no phase 1 (and is no soundness boundary).
static CheckChallenges check_challenges(const VerifyingKey &vk, const dvt_job *j) {
    Challenger g;
    for (const char *t = "dvt-check-rows-1"; *t; t++) g.observe_u32((uint8_t)*t);
    g.observe(vk.prep_root);
    g.observe_u32((uint32_t)vk.extra.size());
    for (auto x : vk.extra) g.observe_u32(x);
    g.observe_u32((uint32_t)j->public_values.size());
    for (auto b : j->public_values) g.observe_u32(b);
    g.observe_u32((uint32_t)j->n_total);
    CheckChallenges c;
    c.xi = g.sample_ext();
    c.perm_alpha = g.sample_ext();
    c.beta = g.sample_ext();
    return c;
}

// the tables of one shard on lane 0 of the member that holds it (its device is current): findings and the shard's per-bus sums
static int shard_check(const Lane &c, const DeviceKey &key, dvt_job *j, ShardJob &s, size_t pos, const CheckChallenges &ch,
                       std::vector<dvt_check_finding> *findings, Fp4 bus[DVT_CHECK_BUSES]) {
    ShardView v;
    if (int rc = shard_view(c, key, j, s, pos, &v)) return rc;
    std::vector<CheckTableOut> res;
    if (int rc = check_tables(c, machine_rv32(), v.tabs, v.pub_mont, ch, true, true, &res)) return rc;
    for (size_t i = 0; i < v.tabs.size(); i++) {
        if (res[i].r.violations) findings->push_back({(uint32_t)pos, (uint32_t)v.traces[i].chip_id, v.tabs[i].log_n, res[i].r});
        for (uint32_t b = 0; b < DVT_CHECK_BUSES; b++) bus[b] += res[i].bus[b];
    }
    return DVT_OK;
}

static int job_check(dvt_prover *p, const dvt_pk *pk, dvt_job *j, dvt_check_finding *findings, size_t cap, dvt_check_summary *summary) {
    if (int rc = same_members(p, pk, j)) return rc;
    const auto t0 = Clock::now();
    const CheckChallenges ch = check_challenges(pk->dev[0].key.vk, j);
    std::vector<dvt_check_finding> all;
    Fp4 bus[DVT_CHECK_BUSES];
    for (auto &b : bus) b = Fp4::zero();
    int rc = DVT_OK;
    for (size_t m = 0; m < n_members(p) && !rc; m++) {
        JobPart &part = j->parts[m];
        rc = turn_to(p, m);
        for (size_t k = 0; k < part.shards.size() && !rc; k++)
            rc = shard_check(lane0(p, m), member_key(pk, m), j, part.shards[k], part.first + k * part.stride, ch, &all, bus);
    }
    if (turn_to(p, 0) && !rc) rc = DVT_ERR_DEVICE;
    if (rc) return rc;
    std::sort(all.begin(), all.end(), [](const dvt_check_finding &a, const dvt_check_finding &b) { return a.shard != b.shard ? a.shard < b.shard : a.chip < b.chip; });
    *summary = dvt_check_summary{};
    for (auto &f : all) summary->violations += f.r.violations;
    summary->n_findings = (uint32_t)all.size();
    for (size_t i = 0; i < all.size() && i < cap; i++) findings[i] = all[i];
    if (j->held() == j->n_total) {
        summary->bus_checked = 1;
        const Fp4 sys = commit_digest_term(PermChallenges{ch.perm_alpha, ch.beta}, j->public_values);
        for (uint32_t b = 0; b < DVT_CHECK_BUSES; b++)
            if (bus[b] != (b == PV_BUS ? sys : Fp4::zero())) summary->unbalanced_buses |= 1u << b;
    }
    summary->ms = (float)ms_since(t0);
    if (!all.empty())
        return fail(p, DVT_ERR_REJECTED, "shard %u, chip %s: row %u violates constraint %d (%llu violations in %u chip tables)", all[0].shard,
                    machine_rv32()->chips[all[0].chip].name, all[0].r.first_row, all[0].r.first_constraint, (unsigned long long)summary->violations,
                    summary->n_findings);
    if (summary->unbalanced_buses) return fail(p, DVT_ERR_REJECTED, "the LogUp sums of the job do not balance (bus mask 0x%x)", summary->unbalanced_buses);
    return DVT_OK;
}

// ------------------------------------------------------------------ the job's bus ledger (dvt_rv32_job_bus_tuples)
// one pass (LEDGER_TALLY = 0 or LEDGER_COLLECT = 1, ledger.cuh) over the tables of one shard on lane 0 of the member that holds
// it (its device is current), into that member's ledger
static int shard_ledger(const Lane &c, const DeviceKey &key, dvt_job *j, ShardJob &s, size_t pos, LedgerDev &l, uint32_t mode) {
    ShardView v;
    if (int rc = shard_view(c, key, j, s, pos, &v)) return rc;
    for (size_t i = 0; i < v.tabs.size(); i++)
        if (int rc = ledger_rows(c, l, v.tabs[i], (uint32_t)v.traces[i].chip_id, v.pub_mont, (uint32_t)pos, mode)) return rc;
    HIP_TRY(c.err, hipStreamSynchronize(c.eng.stream));   // (the next shard's K0 may write the working buffers these launches read)
    return DVT_OK;
}

// one pass over every held shard, and the verifier's side of the eight COMMIT tuples (what commit_digest_term stands for:
// receives of (0x10 0 0 0, k 0 0 0, the bytes of digest word k, 0, 0) on the sys bus) into member 0's ledger
static int job_ledger_pass(dvt_prover *p, const dvt_pk *pk, dvt_job *j, std::vector<LedgerDev> &ledgers, uint32_t mode) {
    for (size_t m = 0; m < ledgers.size(); m++) {
        JobPart &part = j->parts[m];
        if (int rc = turn_to(p, m)) return rc;
        for (size_t k = 0; k < part.shards.size(); k++)
            if (int rc = shard_ledger(lane0(p, m), member_key(pk, m), j, part.shards[k], part.first + k * part.stride, ledgers[m], mode)) return rc;
    }
    if (int rc = turn_to(p, 0)) return rc;
    uint8_t dg[32];
    sha256(j->public_values.data(), j->public_values.size(), dg);
    for (uint32_t k = 0; k < 8; k++) {
        const uint32_t v[14] = {rv32::SYS_COMMIT, 0, 0, 0, k, 0, 0, 0, dg[4 * k], dg[4 * k + 1], dg[4 * k + 2], dg[4 * k + 3], 0, 0};
        if (int rc = ledger_tuple(lane0(p), ledgers[0], PV_BUS, v, 14, -1, 1, 0, mode)) return rc;
    }
    HIP_TRY(p, hipStreamSynchronize(eng0(p).stream));
    return DVT_OK;
}

static int job_ledger_run(dvt_prover *p, const dvt_pk *pk, dvt_job *j, std::vector<LedgerDev> &ledgers, uint64_t seed, std::vector<dvt_bus_tuple> *all,
                          bool *overflow) {
    constexpr uint32_t LOG_BUCKETS = 20, CAP_SLOTS = 1u << 16;
    const size_t G = ledgers.size();
    for (size_t m = 0; m < G; m++) {
        if (int rc = turn_to(p, m)) return rc;
        if (int rc = ledger_init(lane0(p, m), &ledgers[m], LOG_BUCKETS, CAP_SLOTS, seed)) return rc;
    }
    if (int rc = job_ledger_pass(p, pk, j, ledgers, 0)) return rc;
    uint32_t n_dirty = 0;
    if (G == 1) {
        if (int rc = ledger_close(lane0(p), ledgers[0], &n_dirty)) return rc;
    } else {   // the members' tallies added mod p on the host; the one bitmap back to every member
        std::vector<uint64_t> sum, one;
        for (size_t m = 0; m < G; m++) {
            if (int rc = turn_to(p, m)) return rc;
            if (int rc = ledger_tallies(lane0(p, m), ledgers[m], m ? &one : &sum)) return rc;
            for (size_t i = 0; m && i < sum.size(); i++) sum[i] = (sum[i] + one[i]) % P;
        }
        std::vector<uint32_t> bitmap;
        n_dirty = ledger_dirty_of(sum, &bitmap);
        for (size_t m = 0; n_dirty && m < G; m++) {
            if (int rc = turn_to(p, m)) return rc;
            if (int rc = ledger_set_dirty(lane0(p, m), ledgers[m], bitmap)) return rc;
        }
    }
    all->clear();
    *overflow = false;
    if (!n_dirty) return DVT_OK;
    if (int rc = job_ledger_pass(p, pk, j, ledgers, 1)) return rc;
    for (size_t m = 0; m < G; m++) {
        if (int rc = turn_to(p, m)) return rc;
        if (int rc = ledger_records(lane0(p, m), ledgers[m], all, overflow)) return rc;
    }
    ledger_finish(all);
    return DVT_OK;
}

static int job_bus_tuples(dvt_prover *p, const dvt_pk *pk, dvt_job *j, dvt_bus_tuple *out, size_t cap, size_t *n_tuples, uint32_t *truncated) {
    if (int rc = same_members(p, pk, j)) return rc;
    if (j->n_total > (1u << 16)) return fail(p, DVT_ERR_INPUT, "a job of %zu shards: the ledger tags at most 2^16", (size_t)j->n_total);
    const CheckChallenges ch = check_challenges(pk->dev[0].key.vk, j);
    uint64_t seed = (uint64_t)ch.xi.c[0].v | ((uint64_t)ch.xi.c[1].v << 32);
    std::vector<dvt_bus_tuple> all;
    bool overflow = false;
    int rc = DVT_OK;
    for (int attempt = 0; attempt < 2 && !rc; attempt++) {   // records overflowed: once more with another seed
        std::vector<LedgerDev> ledgers(n_members(p));
        rc = job_ledger_run(p, pk, j, ledgers, seed, &all, &overflow);
        for (size_t m = ledgers.size(); m-- > 0;) {   // member 0 last: its device stays current
            if (turn_to(p, m)) continue;
            (void)hipStreamSynchronize(member(p, m).eng.stream);
            ledger_release(&ledgers[m]);
        }
        if (!overflow) break;
        seed = seed * 0x9e3779b97f4a7c15ull + 1;
    }
    if (rc) return rc;
    ledger_copy_out(all, overflow, out, cap, n_tuples, truncated);
    return DVT_OK;
}

// ------------------------------------------------------------------ the execution report (dvt_rv32_job_profile)
// One member's share: its tables from lane 0's pool (counts zeroed, keys all ones), one launch per shard it holds on lane 0's
// stream, one download (which synchronises), everything added into *t.  The buffer goes back to the pool at scope exit.
static int member_profile(const Lane &c, const dvt_pk *pk, JobPart &part, uint32_t log_slots, const std::vector<uint32_t> &classes, prof::Tally *t) {
    if (part.shards.empty()) return DVT_OK;
    Engine &e = c.eng;
    const size_t n = classes.size(), S = (size_t)1 << log_slots;
    // 64-bit words: pc_count, taken, edge counts, syscall counts, counters | edge keys, syscall keys; then the classes
    const size_t zero_words = 2 * n + S + prof::MAX_SYSCALLS + PROFILE_COUNTERS, key_words = S + prof::MAX_SYSCALLS;
    StageBuf buf{e.pool};
    HIP_TRY(c.err, e.pool.alloc_bytes(&buf.ptr, (zero_words + key_words) * 8 + n * 4));
    unsigned long long *d = static_cast<unsigned long long *>(buf.ptr);
    ProfileTables tb{};
    tb.pc_count = d; tb.taken = d + n; tb.edge_counts = d + 2 * n; tb.sys_counts = tb.edge_counts + S; tb.counters = tb.sys_counts + prof::MAX_SYSCALLS;
    tb.edge_keys = d + zero_words; tb.sys_keys = tb.edge_keys + S;
    uint32_t *d_classes = reinterpret_cast<uint32_t *>(d + zero_words + key_words);
    tb.classes = d_classes; tb.n_instr = (uint32_t)n; tb.log_slots = log_slots;
    HIP_TRY(c.err, hipMemsetAsync(d, 0, zero_words * 8, e.stream));
    HIP_TRY(c.err, hipMemsetAsync(tb.edge_keys, 0xff, key_words * 8, e.stream));
    HIP_TRY(c.err, hipMemcpyAsync(d_classes, classes.data(), n * 4, hipMemcpyHostToDevice, e.stream));
    for (auto &s : part.shards) HIP_TRY(c.err, launch_profile_records(e.stream, s.d_recs, s.n_recs, prof::index_of_pc(pk->prog, s.next_pc), tb));
    std::vector<unsigned long long> h(zero_words + key_words);
    if (!e.download(h.data(), d, h.size() * 8)) return engine_fail(c.err, e);
    const unsigned long long *counters = h.data() + 2 * n + S + prof::MAX_SYSCALLS;
    if (counters[PROFILE_BAD_RECORDS]) return fail(c.err, DVT_ERR_INPUT, "%llu cycle records name an instruction outside the text", counters[PROFILE_BAD_RECORDS]);
    if (counters[PROFILE_SYS_OVERFLOW]) return fail(c.err, DVT_ERR_UNSUPPORTED, "more than %u distinct syscall ids", prof::MAX_SYSCALLS);
    for (size_t i = 0; i < n; i++) {
        t->pc_count[i] += h[i];
        if (h[n + i]) t->edges[{(uint32_t)i, classes[i] & prof::TGT_MASK}] += h[n + i];
    }
    const unsigned long long *ek = h.data() + zero_words, *ec = h.data() + 2 * n;
    for (size_t k = 0; k < S; k++)
        if (ek[k] != ~0ull && ec[k]) t->edges[{(uint32_t)(ek[k] >> 32), (uint32_t)ek[k]}] += ec[k];
    for (size_t k = 0; k < prof::MAX_SYSCALLS; k++)
        if (ek[S + k] != ~0ull && ec[S + k]) t->sys[(uint32_t)ek[S + k]] += ec[S + k];
    t->n_transfers += counters[PROFILE_TRANSFERS];
    t->dropped += counters[PROFILE_DROPPED];
    t->shards += (uint32_t)part.shards.size();
    return DVT_OK;
}

static int job_profile(dvt_prover *p, const dvt_pk *pk, dvt_job *j, uint32_t log_edge_slots, const prof::Out &out) {
    if (int rc = same_members(p, pk, j)) return rc;
    const auto t0 = Clock::now();
    const std::vector<uint32_t> classes = prof::instr_classes(pk->prog);
    uint32_t log_slots = log_edge_slots;
    if (!log_slots)
        for (log_slots = prof::DEFAULT_MIN_LOG_SLOTS; log_slots < prof::MAX_LOG_SLOTS && ((size_t)1 << log_slots) < 4 * classes.size();) log_slots++;
    prof::Tally t(pk->prog);
    int rc = DVT_OK;
    for (size_t m = 0; m < n_members(p) && !rc; m++) {
        rc = turn_to(p, m);
        if (!rc) rc = member_profile(lane0(p, m), pk, j->parts[m], log_slots, classes, &t);
    }
    if (turn_to(p, 0) && !rc) rc = DVT_ERR_DEVICE;
    if (rc) return rc;
    if (!prof::emit(pk->prog, t, (uint32_t)j->n_total, ms_since(t0), out)) return fail(p, DVT_ERR_UNSUPPORTED, "more than %u distinct syscall ids", prof::MAX_SYSCALLS);
    return DVT_OK;
}

// ------------------------------------------------------------------ the call-tree report (dvt_rv32_job_calltree)
// Three runs of one kernel body over every span of every shard (calltree.hip), each member on lane 0's stream with buffers
// from lane 0's pool, and the host between them: summary mode for {u, c} per span; summary mode again, writing the unmatched
// calls at the offsets the host made of the c's; the merge of the spans in execution order, which keeps the global stack and
// hands every span the frames it can pop; emit mode.  The frames still open after the last record are closed on the host.
namespace {
struct CalltreeMember {
    StageBuf base, calls, frames;
    std::vector<size_t> span0;                        // of the member's k-th shard
    std::vector<size_t> n_of;                         // the records of the k-th shard the pass takes (a prefix of the shard)
    std::vector<uint32_t> succ_of;                    // the successor of the last of them
    size_t spans = 0, total_calls = 0;
    std::vector<CalltreeSpanSummary> summaries;
    std::vector<unsigned long long> calls_at;
    std::vector<CalltreeCall> h_calls;
    std::vector<CalltreeSpanIn> span_in;
    std::vector<CalltreeFrame> h_frames;
    CalltreeTables tb{};
    unsigned long long *d_calls_at = nullptr;
    CalltreeSpanIn *d_span_in = nullptr;
    hipEvent_t ev[4] = {};                            // a timed run: the summaries [0, 1], the unmatched calls [2, 3]
    bool timed_calls = false;
    explicit CalltreeMember(DevPool &pool) : base{pool}, calls{pool}, frames{pool} {}
    ~CalltreeMember() {
        for (hipEvent_t x : ev)
            if (x) (void)hipEventDestroy(x);
    }
};
// the members' buffers go back to their pools under their own device's turn
struct CalltreeRun {
    dvt_prover *p;
    std::vector<std::unique_ptr<CalltreeMember>> mem;
    ~CalltreeRun() {
        for (size_t m = 0; m < mem.size(); m++) {
            (void)turn_to(p, m);
            mem[m].reset();
        }
        (void)turn_to(p, 0);
    }
};
}  // namespace

// Summary mode over a prefix of every held shard, for the call tree (all records) and the snapshot's backtrace (the records
// before its position): prefix(shard, &n, &succ) names the first n records the pass takes and the successor of the last of
// them.  {u, c} of every span; then summary mode again, writing the unmatched calls of the shards that have any at the offsets
// the host made of the c's.  S = 2^log_slots arc slots are laid out for emit mode (log_slots 0: none).  timed: stream events
// around both runs.
template <class Prefix>
static int calltree_summaries(dvt_prover *p, dvt_job *j, const std::vector<uint32_t> &classes, uint32_t log_slots, bool timed, Prefix prefix, CalltreeRun *run_out) {
    CalltreeRun &run = *run_out;
    const size_t n = classes.size(), G = n_members(p), S = log_slots ? (size_t)1 << log_slots : 0;
    // ---- summary mode: {u, c} of every span
    for (size_t m = 0; m < G; m++) {
        if (int rc = turn_to(p, m)) return rc;
        const Lane c = lane0(p, m);
        Engine &e = c.eng;
        run.mem.emplace_back(new CalltreeMember(e.pool));
        CalltreeMember &cm = *run.mem.back();
        for (auto &s : j->parts[m].shards) {
            size_t take = 0;
            uint32_t succ = prof::NO_SUCC;
            prefix(s, &take, &succ);
            cm.n_of.push_back(std::min(take, s.n_recs));
            cm.succ_of.push_back(succ);
            cm.span0.push_back(cm.spans);
            cm.spans += (cm.n_of.back() + CALLTREE_SPAN - 1) / CALLTREE_SPAN;
        }
        if (!cm.spans) continue;
        if (timed)
            for (auto &x : cm.ev) HIP_TRY(c.err, hipEventCreate(&x));
        // 64-bit words: counters, arc calls, arc cycles | arc keys | calls_at | span_in (two each) | summaries; then the classes
        const size_t zero_words = CALLTREE_COUNTERS + 2 * S, words = zero_words + S + 4 * cm.spans;
        HIP_TRY(c.err, e.pool.alloc_bytes(&cm.base.ptr, words * 8 + n * 4));
        unsigned long long *d = static_cast<unsigned long long *>(cm.base.ptr);
        CalltreeTables &tb = cm.tb;
        tb.counters = d; tb.arc_calls = d + CALLTREE_COUNTERS; tb.arc_cycles = tb.arc_calls + S; tb.arc_keys = d + zero_words;
        cm.d_calls_at = tb.arc_keys + S;
        cm.d_span_in = reinterpret_cast<CalltreeSpanIn *>(cm.d_calls_at + cm.spans);
        tb.summaries = reinterpret_cast<CalltreeSpanSummary *>(cm.d_calls_at + 3 * cm.spans);
        uint32_t *d_classes = reinterpret_cast<uint32_t *>(d + words);
        tb.classes = d_classes; tb.n_instr = (uint32_t)n; tb.log_slots = log_slots;
        HIP_TRY(c.err, hipMemsetAsync(d, 0, zero_words * 8, e.stream));
        if (S) HIP_TRY(c.err, hipMemsetAsync(tb.arc_keys, 0xff, S * 8, e.stream));
        HIP_TRY(c.err, hipMemcpyAsync(d_classes, classes.data(), n * 4, hipMemcpyHostToDevice, e.stream));
        if (timed) HIP_TRY(c.err, hipEventRecord(cm.ev[0], e.stream));
        for (size_t k = 0; k < cm.span0.size(); k++)
            HIP_TRY(c.err, launch_calltree_summary(e.stream, j->parts[m].shards[k].d_recs, cm.n_of[k], cm.succ_of[k], cm.span0[k], tb));
        if (timed) HIP_TRY(c.err, hipEventRecord(cm.ev[1], e.stream));
        cm.summaries.resize(cm.spans);
        if (!e.download(cm.summaries.data(), tb.summaries, cm.spans * sizeof(CalltreeSpanSummary))) return engine_fail(c.err, e);
        cm.calls_at.resize(cm.spans);
        for (size_t i = 0; i < cm.spans; i++) {
            if (cm.summaries[i].u > CALLTREE_SPAN || cm.summaries[i].c > CALLTREE_SPAN) return fail(p, DVT_ERR_DEVICE, "span summary out of range");
            cm.calls_at[i] = cm.total_calls;
            cm.total_calls += cm.summaries[i].c;
        }
    }
    // ---- summary mode again: the unmatched calls of the shards that have any, at those offsets
    for (size_t m = 0; m < G; m++) {
        CalltreeMember &cm = *run.mem[m];
        if (!cm.total_calls) continue;
        if (int rc = turn_to(p, m)) return rc;
        const Lane c = lane0(p, m);
        Engine &e = c.eng;
        HIP_TRY(c.err, e.pool.alloc_bytes(&cm.calls.ptr, cm.total_calls * sizeof(CalltreeCall)));
        CalltreeTables tb = cm.tb;
        tb.calls_at = cm.d_calls_at;
        tb.calls = static_cast<CalltreeCall *>(cm.calls.ptr);
        HIP_TRY(c.err, hipMemcpyAsync(cm.d_calls_at, cm.calls_at.data(), cm.spans * 8, hipMemcpyHostToDevice, e.stream));
        if (timed) HIP_TRY(c.err, hipEventRecord(cm.ev[2], e.stream));
        for (size_t k = 0; k < cm.span0.size(); k++) {
            const size_t end = k + 1 < cm.span0.size() ? cm.span0[k + 1] : cm.spans;
            size_t n_calls = 0;
            for (size_t i = cm.span0[k]; i < end; i++) n_calls += cm.summaries[i].c;
            if (n_calls) HIP_TRY(c.err, launch_calltree_summary(e.stream, j->parts[m].shards[k].d_recs, cm.n_of[k], cm.succ_of[k], cm.span0[k], tb));
        }
        if (timed) {
            HIP_TRY(c.err, hipEventRecord(cm.ev[3], e.stream));
            cm.timed_calls = true;
        }
        cm.h_calls.resize(cm.total_calls);
        if (!e.download(cm.h_calls.data(), tb.calls, cm.total_calls * sizeof(CalltreeCall))) return engine_fail(c.err, e);
    }
    return DVT_OK;
}

// The merge of one span into the global stack (depth >= 1), the spans taken in execution order: the span's u unmatched RETs
// pop, the root stays; its c unmatched CALLs push, each frame opening after its call.  Returns the RETs that found only the
// root.  The frames open after the last span are the stack at that point: the snapshot's backtrace.
static uint32_t calltree_merge_span(std::vector<calltree::Frame> &stack, const CalltreeSpanSummary &sum, const CalltreeCall *calls, uint64_t span_pos) {
    const size_t depth = stack.size(), pops = std::min<size_t>(sum.u, depth - 1);
    stack.resize(depth - pops);
    for (uint32_t q = 0; q < sum.c; q++) stack.push_back(calltree::Frame{calls[q].fn, span_pos + calls[q].pos + 1});
    return (uint32_t)(sum.u - pops);
}

static int job_calltree(dvt_prover *p, const dvt_pk *pk, dvt_job *j, uint32_t log_arc_slots, const calltree::Out &out) {
    if (int rc = same_members(p, pk, j)) return rc;
    if (j->first != 0 || j->stride != 1 || j->held() != j->n_total)
        return fail(p, DVT_ERR_UNSUPPORTED, "the job holds %zu of the %zu shards of its execution (first %zu, stride %zu): the call stack across a gap is unknown",
                    j->held(), j->n_total, j->first, j->stride);
    const auto t0 = Clock::now();
    calltree::State st(pk->prog);
    const size_t n = st.classes.size(), G = n_members(p);
    uint32_t log_slots = log_arc_slots;
    if (!log_slots)
        for (log_slots = prof::DEFAULT_MIN_LOG_SLOTS; log_slots < prof::MAX_LOG_SLOTS && ((size_t)1 << log_slots) < 4 * n;) log_slots++;
    const size_t S = (size_t)1 << log_slots;
    const uint32_t entry = prof::index_of_pc(pk->prog, pk->prog.entry);
    if (entry == prof::NO_SUCC) return fail(p, DVT_ERR_INPUT, "the entry 0x%08x is no instruction of the text", pk->prog.entry);
    auto succ_of = [&](const ShardJob &s) { return prof::index_of_pc(pk->prog, s.next_pc); };
    CalltreeRun run{p, {}};
    if (int rc = calltree_summaries(p, j, st.classes, log_slots, false, [&](const ShardJob &s, size_t *take, uint32_t *succ) { *take = s.n_recs; *succ = succ_of(s); }, &run))
        return rc;
    const double ms_summary = ms_since(t0);

    // ---- the merge: the spans in execution order, over all shards in job order, whichever member holds them
    const auto t1 = Clock::now();
    std::vector<uint64_t> base_of(j->n_total);   // global position of the shard's first record
    uint64_t cycles = 0;
    st.stack.push_back(calltree::Frame{entry, 0});
    for (size_t pos = 0; pos < j->n_total; pos++) {
        size_t m = 0;
        const ShardJob *s = j->at(pos, &m);
        if (!s) return fail(p, DVT_ERR_UNSUPPORTED, "the job does not hold shard %zu", pos);
        CalltreeMember &cm = *run.mem[m];
        const size_t k = (size_t)(s - j->parts[m].shards.data());
        base_of[pos] = cycles;
        const size_t n_spans = (s->n_recs + CALLTREE_SPAN - 1) / CALLTREE_SPAN;
        if (cm.span_in.empty()) cm.span_in.resize(cm.spans);
        for (size_t i = 0; i < n_spans; i++) {
            const size_t span = cm.span0[k] + i;
            const CalltreeSpanSummary sum = cm.summaries[span];
            const size_t depth = st.stack.size(), n_in = std::min<size_t>((size_t)sum.u + 1, depth);
            cm.span_in[span] = CalltreeSpanIn{cm.h_frames.size(), (uint32_t)n_in, (uint32_t)std::min<size_t>(depth, 0xffffffffu)};
            for (size_t f = 0; f < n_in; f++) cm.h_frames.push_back(CalltreeFrame{st.stack[depth - 1 - f].open, st.stack[depth - 1 - f].fn, 0});
            (void)calltree_merge_span(st.stack, sum, cm.h_calls.data() + cm.calls_at[span], cycles + i * CALLTREE_SPAN);
        }
        cycles += s->n_recs;
    }
    const double ms_merge = ms_since(t1);

    // ---- emit mode
    const auto t2 = Clock::now();
    unsigned long long bad = 0;
    for (size_t m = 0; m < G; m++) {
        CalltreeMember &cm = *run.mem[m];
        if (!cm.spans) continue;
        if (int rc = turn_to(p, m)) return rc;
        const Lane c = lane0(p, m);
        Engine &e = c.eng;
        HIP_TRY(c.err, e.pool.alloc_bytes(&cm.frames.ptr, cm.h_frames.size() * sizeof(CalltreeFrame)));
        CalltreeTables tb = cm.tb;
        tb.span_in = cm.d_span_in;
        tb.frames = static_cast<const CalltreeFrame *>(cm.frames.ptr);
        HIP_TRY(c.err, hipMemcpyAsync(cm.d_span_in, cm.span_in.data(), cm.spans * sizeof(CalltreeSpanIn), hipMemcpyHostToDevice, e.stream));
        HIP_TRY(c.err, hipMemcpyAsync(cm.frames.ptr, cm.h_frames.data(), cm.h_frames.size() * sizeof(CalltreeFrame), hipMemcpyHostToDevice, e.stream));
        for (size_t k = 0; k < cm.span0.size(); k++) {
            const ShardJob &s = j->parts[m].shards[k];
            HIP_TRY(c.err, launch_calltree_emit(e.stream, s.d_recs, s.n_recs, succ_of(s), cm.span0[k], base_of[s.index - 1], tb));
        }
        std::vector<unsigned long long> h(CALLTREE_COUNTERS + 3 * S);
        if (!e.download(h.data(), tb.counters, h.size() * 8)) return engine_fail(c.err, e);
        const unsigned long long *calls = h.data() + CALLTREE_COUNTERS, *cyc = calls + S, *keys = cyc + S;
        for (size_t q = 0; q < S; q++)
            if (keys[q] != ~0ull && calls[q]) {
                calltree::Arc &a = st.arcs[{(uint32_t)(keys[q] >> 32), (uint32_t)keys[q]}];
                a.calls += calls[q];
                a.cycles += cyc[q];
            }
        st.dropped_frames += h[CALLTREE_DROPPED_FRAMES];
        st.dropped_cycles += h[CALLTREE_DROPPED_CYCLES];
        st.unmatched_returns += h[CALLTREE_UNMATCHED];
        st.max_depth = std::max(st.max_depth, (uint32_t)h[CALLTREE_MAX_DEPTH]);
        bad += h[CALLTREE_BAD_RECORDS];
    }
    if (turn_to(p, 0)) return DVT_ERR_DEVICE;
    if (bad) return fail(p, DVT_ERR_INPUT, "%llu cycle records name an instruction outside the text", bad);
    st.cycles = cycles;
    if (!cycles) st.stack.clear();   // (nothing retired: no root)
    st.max_depth = std::max(st.max_depth, (uint32_t)st.stack.size());
    st.finish();
    p->calltree_ms[0] = ms_summary; p->calltree_ms[1] = ms_merge; p->calltree_ms[2] = ms_since(t2);
    calltree::emit(pk->prog, st, (uint32_t)j->n_total, ms_since(t0), out);
    return DVT_OK;
}

// ------------------------------------------------------------------ the memory report (dvt_rv32_job_memory)
// One member's share: its tables, the footprint bitmap and the dense array from lane 0's pool (zeroed in stream order), one
// launch per shard it holds on lane 0's stream, the gather, two downloads (which synchronise); counters added and bitmap lines
// ORed into *t.  The buffers go back to the pool at scope exit.
static int member_memory(const Lane &c, JobPart &part, const std::vector<uint32_t> &statics, size_t n, uint32_t n_pre, memrep::Tally *t) {
    if (part.shards.empty()) return DVT_OK;
    Engine &e = c.eng;
    // 64-bit words: first_touch, counters, the page arrays; then sp[2], the dense count and a pad; then the static words
    const size_t zero_words = n + MEMORY_COUNTERS + (size_t)MEMORY_PAGE_ARRAYS * memrep::N_PAGES;
    size_t n_recs = 0;
    for (auto &s : part.shards) n_recs += s.n_recs;
    const uint32_t cap = (uint32_t)std::min<size_t>(memrep::N_PAGES, 4 * n_recs);   // (a record touches at most four pages)
    StageBuf buf{e.pool}, bitmap{e.pool}, dense{e.pool};
    HIP_TRY(c.err, e.pool.alloc_bytes(&buf.ptr, zero_words * 8 + 16 + statics.size() * 4));
    HIP_TRY(c.err, e.pool.alloc_bytes(&bitmap.ptr, (size_t)memrep::BITMAP_WORDS * 4));
    HIP_TRY(c.err, e.pool.alloc_bytes(&dense.ptr, std::max<size_t>(cap, 1) * sizeof(MemoryDensePage)));
    unsigned long long *d = static_cast<unsigned long long *>(buf.ptr);
    uint32_t *d32 = reinterpret_cast<uint32_t *>(d + zero_words);
    MemoryTables tb{};
    tb.first_touch = d; tb.counters = d + n; tb.page_ctr = d + n + MEMORY_COUNTERS;
    tb.sp = d32; tb.bitmap = static_cast<uint32_t *>(bitmap.ptr);
    tb.classes = d32 + 4; tb.offs = d32 + 4 + n; tb.pre = d32 + 4 + 2 * n;
    tb.n_instr = (uint32_t)n; tb.n_pre = n_pre;
    const uint32_t head[4] = {0xffffffffu, 0, 0, 0};
    HIP_TRY(c.err, hipMemsetAsync(d, 0, zero_words * 8, e.stream));
    HIP_TRY(c.err, hipMemsetAsync(bitmap.ptr, 0, (size_t)memrep::BITMAP_WORDS * 4, e.stream));
    HIP_TRY(c.err, hipMemcpyAsync(d32, head, sizeof head, hipMemcpyHostToDevice, e.stream));
    HIP_TRY(c.err, hipMemcpyAsync(d32 + 4, statics.data(), statics.size() * 4, hipMemcpyHostToDevice, e.stream));
    for (auto &s : part.shards) HIP_TRY(c.err, launch_memory_records(e.stream, s.d_recs, s.n_recs, tb));
    HIP_TRY(c.err, launch_memory_gather(e.stream, tb, static_cast<MemoryDensePage *>(dense.ptr), cap, d32 + 2));
    std::vector<unsigned long long> h(n + MEMORY_COUNTERS + 2);   // first_touch, counters | sp, the dense count, the pad
    if (!e.download(h.data(), d, (n + MEMORY_COUNTERS) * 8) || !e.download(h.data() + n + MEMORY_COUNTERS, d32, 16)) return engine_fail(c.err, e);
    const unsigned long long *counters = h.data() + n;
    uint32_t tail[4];
    memcpy(tail, h.data() + n + MEMORY_COUNTERS, sizeof tail);
    if (counters[MEMORY_BAD_RECORDS])
        return fail(c.err, DVT_ERR_INPUT, "%llu cycle records name an instruction outside the text or an address outside guest memory", counters[MEMORY_BAD_RECORDS]);
    if (tail[2] > cap) return fail(c.err, DVT_ERR_DEVICE, "%u pages with accesses, room for %u", tail[2], cap);
    std::vector<MemoryDensePage> pages(tail[2]);
    if (!pages.empty() && !e.download(pages.data(), dense.ptr, pages.size() * sizeof(MemoryDensePage))) return engine_fail(c.err, e);
    for (size_t i = 0; i < n; i++) t->first_touch[i] += h[i];
    for (const MemoryDensePage &dp : pages) {
        if (dp.page >= memrep::N_PAGES) return fail(c.err, DVT_ERR_DEVICE, "page %u out of range", dp.page);
        memrep::Page &pg = t->pages[dp.page];
        pg.loads += dp.loads; pg.stores += dp.stores; pg.pre_reads += dp.pre_reads; pg.pre_writes += dp.pre_writes; pg.first += dp.first;
        for (uint32_t k = 0; k < memrep::LINE_WORDS; k++) pg.bits[k] |= dp.bits[k];
    }
    t->cycles += counters[MEMORY_CYCLES];
    t->pre_calls += counters[MEMORY_PRE_CALLS];
    if (counters[MEMORY_SP_WRITES]) {
        t->sp_writes += counters[MEMORY_SP_WRITES];
        t->sp_min = std::min(t->sp_min, tail[0]);
        t->sp_max = std::max(t->sp_max, tail[1]);
    }
    t->shards += (uint32_t)part.shards.size();
    return DVT_OK;
}

static int job_memory(dvt_prover *p, const dvt_pk *pk, dvt_job *j, const memrep::Out &out) {
    if (int rc = same_members(p, pk, j)) return rc;
    const auto t0 = Clock::now();
    const size_t n = pk->prog.instrs.size() - 1;
    const std::vector<memrep::PreShape> shapes = memrep::pre_shapes();
    std::vector<uint32_t> statics(2 * n);   // classes, offsets, then the shapes
    for (size_t i = 0; i < n; i++) {
        statics[i] = memrep::instr_class(pk->prog.instrs[i]);
        statics[n + i] = pk->prog.instrs[i].off;
    }
    for (auto &s : shapes) statics.insert(statics.end(), {s.id, s.n0, s.r0, s.w0, s.n1, s.w1});
    memrep::Tally t(pk->prog);
    int rc = DVT_OK;
    for (size_t m = 0; m < n_members(p) && !rc; m++) {
        rc = turn_to(p, m);
        if (!rc) rc = member_memory(lane0(p, m), j->parts[m], statics, n, (uint32_t)shapes.size(), &t);
    }
    if (turn_to(p, 0) && !rc) rc = DVT_ERR_DEVICE;
    if (rc) return rc;
    memrep::emit(pk->prog, t, (uint32_t)j->n_total, j->held() == j->n_total, ms_since(t0), out);
    return DVT_OK;
}

// ------------------------------------------------------------------ watchpoints (dvt_rv32_job_watch)
// Count and scan per member on lane 0's stream with buffers from lane 0's pool (one count launch and one scan launch per shard
// it holds); the host downloads n_queries totals per shard, adds them in execution order over all members and derives, per
// query, the ranks to keep; the emit pass runs again over those shards alone that have a kept rank, and every member's kept
// hits are copied from its own array to the caller's slots.  Nothing is sorted: a slot is a rank.
namespace {
struct WatchMember {
    StageBuf base, hits;
    std::vector<size_t> span0;            // of the member's k-th shard
    size_t spans = 0;
    uint32_t *d_counts = nullptr, *d_offs = nullptr, *d_totals = nullptr;
    std::vector<uint32_t> totals;         // [shard k][query]
    std::vector<dvt_watch_hit> h_hits;
    hipEvent_t ev[5] = {};                // count [0, 1], scan [1, 2], emit [3, 4]
    bool emitted = false;
    explicit WatchMember(DevPool &pool) : base{pool}, hits{pool} {}
    ~WatchMember() {
        for (hipEvent_t x : ev)
            if (x) (void)hipEventDestroy(x);
    }
};
// the members' buffers go back to their pools under their own device's turn
struct WatchRun {
    dvt_prover *p;
    std::vector<std::unique_ptr<WatchMember>> mem;
    ~WatchRun() {
        for (size_t m = 0; m < mem.size(); m++) {
            (void)turn_to(p, m);
            mem[m].reset();
        }
        (void)turn_to(p, 0);
    }
};
}  // namespace

static int job_watch(dvt_prover *p, const dvt_pk *pk, dvt_job *j, const dvt_watch_query *queries, size_t nq, uint32_t K, dvt_watch_hit *hits,
                     uint64_t *totals, dvt_watch_summary *summary) {
    if (int rc = same_members(p, pk, j)) return rc;
    const auto t0 = Clock::now();
    const size_t n = pk->prog.instrs.size() - 1, G = n_members(p);
    std::vector<uint32_t> statics(2 * n);   // the static words, then the offsets
    for (size_t i = 0; i < n; i++) {
        statics[i] = watch::instr_static(pk->prog.instrs[i]);
        statics[n + i] = pk->prog.instrs[i].off;
    }
    WatchArgs args{};
    std::copy_n(queries, nq, args.q);
    args.sh = watch::shapes();
    args.n_instr = (uint32_t)n; args.text_base = pk->prog.text_base; args.n_queries = (uint32_t)nq;
    WatchRun run{p, {}};
    std::vector<const uint32_t *> d_statics(G, nullptr);
    uint64_t cycles = 0;
    unsigned long long bad = 0;

    // ---- count and scan
    for (size_t m = 0; m < G; m++) {
        if (int rc = turn_to(p, m)) return rc;
        const Lane c = lane0(p, m);
        Engine &e = c.eng;
        run.mem.emplace_back(new WatchMember(e.pool));
        WatchMember &wm = *run.mem.back();
        JobPart &part = j->parts[m];
        for (auto &s : part.shards) {
            wm.span0.push_back(wm.spans);
            wm.spans += (s.n_recs + watch::SPAN - 1) / watch::SPAN;
            cycles += s.n_recs;
        }
        if (part.shards.empty()) continue;
        for (auto &x : wm.ev) HIP_TRY(c.err, hipEventCreate(&x));
        // the bad-record counter (64 bits), then u32: span counts, span offsets, shard totals, the static words
        const size_t span_words = std::max<size_t>(wm.spans, 1) * nq, total_words = part.shards.size() * nq;
        HIP_TRY(c.err, e.pool.alloc_bytes(&wm.base.ptr, 8 + (2 * span_words + total_words + statics.size()) * 4));
        unsigned long long *d_bad = static_cast<unsigned long long *>(wm.base.ptr);
        wm.d_counts = reinterpret_cast<uint32_t *>(d_bad + 1);
        wm.d_offs = wm.d_counts + span_words;
        wm.d_totals = wm.d_offs + span_words;
        uint32_t *d_stat = wm.d_totals + total_words;
        d_statics[m] = d_stat;
        args.statics = d_stat; args.offs = d_stat + n;
        HIP_TRY(c.err, hipMemsetAsync(wm.base.ptr, 0, 8 + (2 * span_words + total_words) * 4, e.stream));
        HIP_TRY(c.err, hipMemcpyAsync(d_stat, statics.data(), statics.size() * 4, hipMemcpyHostToDevice, e.stream));
        HIP_TRY(c.err, hipEventRecord(wm.ev[0], e.stream));
        for (size_t k = 0; k < part.shards.size(); k++) {
            const ShardJob &s = part.shards[k];
            args.shard = s.index;
            HIP_TRY(c.err, launch_watch_count(e.stream, s.d_recs, s.n_recs, args, wm.d_counts + wm.span0[k] * nq, d_bad));
        }
        HIP_TRY(c.err, hipEventRecord(wm.ev[1], e.stream));
        for (size_t k = 0; k < part.shards.size(); k++) {
            const size_t n_spans = (part.shards[k].n_recs + watch::SPAN - 1) / watch::SPAN;
            HIP_TRY(c.err, launch_watch_scan(e.stream, wm.d_counts + wm.span0[k] * nq, wm.d_offs + wm.span0[k] * nq, (uint32_t)n_spans, (uint32_t)nq,
                                             wm.d_totals + k * nq));
        }
        HIP_TRY(c.err, hipEventRecord(wm.ev[2], e.stream));
        wm.totals.resize(total_words);
        unsigned long long h_bad = 0;
        if (!e.download(wm.totals.data(), wm.d_totals, total_words * 4) || !e.download(&h_bad, d_bad, 8)) return engine_fail(c.err, e);
        bad += h_bad;
    }
    if (turn_to(p, 0)) return DVT_ERR_DEVICE;
    if (bad) return fail(p, DVT_ERR_INPUT, "%llu cycle records name an instruction outside the text or an address outside guest memory", bad);

    // ---- the ranks: the held shards in execution order, whichever member holds them
    struct Held { uint32_t index; size_t m, k; };
    std::vector<Held> held;
    for (size_t m = 0; m < G; m++)
        for (size_t k = 0; k < j->parts[m].shards.size(); k++) held.push_back({j->parts[m].shards[k].index, m, k});
    std::sort(held.begin(), held.end(), [](const Held &a, const Held &b) { return a.index < b.index; });
    std::vector<std::vector<unsigned long long>> base_of(held.size(), std::vector<unsigned long long>(nq, 0));
    WatchEmitArgs ea{};
    ea.cap_each = K;
    for (size_t h = 0; h < held.size(); h++)
        for (size_t q = 0; q < nq; q++) {
            base_of[h][q] = ea.total[q];
            ea.total[q] += run.mem[held[h].m]->totals[held[h].k * nq + q];
        }
    for (size_t q = 0; q < nq; q++) totals[q] = ea.total[q];
    // the kept ranks of query q among [lo, hi)
    auto kept_in = [&](size_t q, unsigned long long lo, unsigned long long hi) {
        const watch::Keep keep = watch::keep_of(ea.total[q], K);
        return hi > lo && (lo < keep.first_end || hi > keep.last_begin);
    };

    // ---- emit: only the shards with a kept rank
    double emit_shards = 0;
    for (size_t h = 0; K && h < held.size(); h++) {
        const size_t m = held[h].m, k = held[h].k;
        WatchMember &wm = *run.mem[m];
        bool any = false;
        for (size_t q = 0; q < nq; q++) any = any || kept_in(q, base_of[h][q], base_of[h][q] + wm.totals[k * nq + q]);
        if (!any) continue;
        if (int rc = turn_to(p, m)) return rc;
        const Lane c = lane0(p, m);
        Engine &e = c.eng;
        if (!wm.emitted) {
            HIP_TRY(c.err, e.pool.alloc_bytes(&wm.hits.ptr, 2 * nq * K * sizeof(dvt_watch_hit)));
            HIP_TRY(c.err, hipEventRecord(wm.ev[3], e.stream));
            wm.emitted = true;
        }
        const ShardJob &s = j->parts[m].shards[k];
        args.statics = d_statics[m]; args.offs = d_statics[m] + n; args.shard = s.index;
        std::copy(base_of[h].begin(), base_of[h].end(), ea.base);
        HIP_TRY(c.err, launch_watch_emit(e.stream, s.d_recs, s.n_recs, args, ea, wm.d_counts + wm.span0[k] * nq, wm.d_offs + wm.span0[k] * nq, wm.hits.ptr));
        emit_shards++;
    }
    double ms[3] = {0, 0, 0};
    for (size_t m = 0; m < G; m++) {
        WatchMember &wm = *run.mem[m];
        if (!wm.ev[0]) continue;
        if (int rc = turn_to(p, m)) return rc;
        const Lane c = lane0(p, m);
        Engine &e = c.eng;
        float t = 0;
        if (wm.emitted) {
            HIP_TRY(c.err, hipEventRecord(wm.ev[4], e.stream));
            wm.h_hits.resize(2 * nq * K);
            if (!e.download(wm.h_hits.data(), wm.hits.ptr, wm.h_hits.size() * sizeof(dvt_watch_hit))) return engine_fail(c.err, e);
            if (hipEventElapsedTime(&t, wm.ev[3], wm.ev[4]) == hipSuccess) ms[2] += t;
        }
        if (hipEventElapsedTime(&t, wm.ev[0], wm.ev[1]) == hipSuccess) ms[0] += t;
        if (hipEventElapsedTime(&t, wm.ev[1], wm.ev[2]) == hipSuccess) ms[1] += t;
    }
    if (turn_to(p, 0)) return DVT_ERR_DEVICE;
    // every kept rank from the array of the member whose shard holds it
    for (size_t h = 0; K && h < held.size(); h++) {
        const WatchMember &wm = *run.mem[held[h].m];
        if (!wm.emitted) continue;
        for (size_t q = 0; q < nq; q++) {
            const watch::Keep keep = watch::keep_of(ea.total[q], K);
            const unsigned long long lo = base_of[h][q], hi = lo + wm.totals[held[h].k * nq + q];
            for (unsigned long long r = lo; r < std::min(hi, keep.first_end); r++) hits[2 * q * K + r] = wm.h_hits[2 * q * K + r];
            for (unsigned long long r = std::max(lo, keep.last_begin); r < hi; r++) hits[(2 * q + 1) * K + (r - keep.last_begin)] = wm.h_hits[(2 * q + 1) * K + (r - keep.last_begin)];
        }
    }
    for (int i = 0; i < 3; i++) p->watch_ms[i] = ms[i];
    p->watch_ms[3] = emit_shards;
    dvt_watch_summary out{};
    out.cycles = cycles;
    out.n_queries = (uint32_t)nq; out.cap_each = K;
    out.shards_searched = (uint32_t)held.size(); out.shards_total = (uint32_t)j->n_total;
    out.text_base = pk->prog.text_base; out.n_instr = (uint32_t)n; out.span = watch::SPAN;
    out.ms = (float)ms_since(t0);
    *summary = out;
    return DVT_OK;
}

// ------------------------------------------------------------------ snapshots (dvt_rv32_job_snapshot)
// Reduce per member on lane 0's stream with buffers from lane 0's pool (one launch per shard it holds) into the member's winner
// tables; the backtrace from the call-tree pass in summary mode over the records before the position and the merge of the call
// tree; the host merges the members' winners with max / min and asks the member that holds each winner's shard for the record
// at that position (gather), the call records of the returned frames among them; snap::emit() makes the cells.
namespace {
struct SnapMember {
    StageBuf base, items, sides;
    unsigned long long *d_tables = nullptr;
    const uint32_t *d_statics = nullptr;
    std::vector<SnapFetch> fetch;
    std::vector<snap::Side> got;
    hipEvent_t ev[4] = {};                // reduce [0, 1], gather [2, 3]
    bool gathered = false;
    explicit SnapMember(DevPool &pool) : base{pool}, items{pool}, sides{pool} {}
    ~SnapMember() {
        for (hipEvent_t x : ev)
            if (x) (void)hipEventDestroy(x);
    }
};
// the members' buffers go back to their pools under their own device's turn
struct SnapRun {
    dvt_prover *p;
    std::vector<std::unique_ptr<SnapMember>> mem;
    ~SnapRun() {
        for (size_t m = 0; m < mem.size(); m++) {
            (void)turn_to(p, m);
            mem[m].reset();
        }
        (void)turn_to(p, 0);
    }
};
}  // namespace

static int job_snapshot(dvt_prover *p, const dvt_pk *pk, dvt_job *j, uint32_t shard, uint32_t row, const snap::Ranges &rg, dvt_snap_cell regs[32],
                        dvt_snap_cell *words, dvt_snap_frame *frames, size_t cap_frames, dvt_snap_summary *summary) {
    if (int rc = same_members(p, pk, j)) return rc;
    if (j->first != 0 || j->stride != 1 || j->held() != j->n_total)
        return fail(p, DVT_ERR_UNSUPPORTED, "the job holds %zu of the %zu shards of its execution (first %zu, stride %zu): the state across a gap is unknown",
                    j->held(), j->n_total, j->first, j->stride);
    const auto t0 = Clock::now();
    const rv32::Program &prog = pk->prog;
    const size_t n = prog.instrs.size() - 1, G = n_members(p), W = rg.n_words;
    const unsigned long long P = watch::position(shard, row);
    SnapRun run{p, {}};   // (declared first: however the call ends, member 0's device is current again)
    // ---- the shards in execution order: their sizes, the records before P, the record at P
    std::vector<uint64_t> shard_n(j->n_total);
    uint64_t cycles = 0, position = 0;
    size_t any_m = 0;
    for (size_t pos = 0; pos < j->n_total; pos++) {
        const ShardJob *s = j->at(pos, &any_m);
        if (!s) return fail(p, DVT_ERR_UNSUPPORTED, "the job does not hold shard %zu", pos);
        if (s->n_recs > 0xffffffffull) return fail(p, DVT_ERR_INPUT, "shard %zu has %zu records", pos, s->n_recs);
        shard_n[pos] = s->n_recs;
        cycles += s->n_recs;
        position += s->index < shard ? s->n_recs : s->index == shard ? std::min<uint64_t>(s->n_recs, row) : 0;
    }
    uint32_t at_shard = 1, at_row = 0, idx_at = prof::NO_SUCC, pc = j->n_total ? 0 : prog.entry;
    snap::locate(shard_n, position, &at_shard, &at_row);
    if (position < cycles) {   // the record at P: its idx is the successor of the last record before P, and names the pc
        size_t m = 0;
        const ShardJob *s = j->at(at_shard - 1, &m);
        if (!s || at_row >= s->n_recs) return fail(p, DVT_ERR_DEVICE, "position %llu lies in no shard", (unsigned long long)position);
        if (int rc = turn_to(p, m)) return rc;
        if (!member(p, m).eng.download(&idx_at, &s->d_recs[at_row].idx, 4)) return engine_fail(p->err, member(p, m).eng);
        if (idx_at >= n) return fail(p, DVT_ERR_INPUT, "the cycle record at shard %u, row %u names an instruction outside the text", at_shard, at_row);
        pc = prog.text_base + 4 * idx_at;
    } else if (j->n_total)
        pc = j->at(j->n_total - 1, &any_m)->next_pc;

    std::vector<uint32_t> statics(2 * n);   // the static words, then the offsets
    for (size_t i = 0; i < n; i++) {
        statics[i] = watch::instr_static(prog.instrs[i]);
        statics[n + i] = prog.instrs[i].off;
    }
    SnapArgs args{};
    args.rg = rg;
    args.sh = watch::shapes();
    args.n_instr = (uint32_t)n; args.text_base = prog.text_base; args.P = P;
    const size_t table_words = 1 + 32 + 2 * W;   // 64-bit: bad records, regs, before | after; then the static words

    // ---- reduce
    for (size_t m = 0; m < G; m++) {
        if (int rc = turn_to(p, m)) return rc;
        const Lane c = lane0(p, m);
        Engine &e = c.eng;
        run.mem.emplace_back(new SnapMember(e.pool));
        SnapMember &sm = *run.mem.back();
        JobPart &part = j->parts[m];
        if (part.shards.empty()) continue;
        for (auto &x : sm.ev) HIP_TRY(c.err, hipEventCreate(&x));
        HIP_TRY(c.err, e.pool.alloc_bytes(&sm.base.ptr, table_words * 8 + statics.size() * 4));
        sm.d_tables = static_cast<unsigned long long *>(sm.base.ptr);
        uint32_t *d_stat = reinterpret_cast<uint32_t *>(sm.d_tables + table_words);
        sm.d_statics = d_stat;
        const SnapTables tb{sm.d_tables + 33, sm.d_tables + 33 + W, sm.d_tables + 1, sm.d_tables};
        HIP_TRY(c.err, hipMemsetAsync(sm.d_tables, 0, (33 + W) * 8, e.stream));
        if (W) HIP_TRY(c.err, hipMemsetAsync(tb.after, 0xff, W * 8, e.stream));
        HIP_TRY(c.err, hipMemcpyAsync(d_stat, statics.data(), statics.size() * 4, hipMemcpyHostToDevice, e.stream));
        args.statics = d_stat; args.offs = d_stat + n;
        HIP_TRY(c.err, hipEventRecord(sm.ev[0], e.stream));
        for (auto &s : part.shards) {
            args.shard = s.index;
            HIP_TRY(c.err, launch_snapshot_reduce(e.stream, s.d_recs, s.n_recs, args, tb));
        }
        HIP_TRY(c.err, hipEventRecord(sm.ev[1], e.stream));
    }

    // ---- the backtrace: the call-tree pass in summary mode over the records before P, and the call tree's merge
    const uint32_t entry = prof::index_of_pc(prog, prog.entry);
    if (entry == prof::NO_SUCC) return fail(p, DVT_ERR_INPUT, "the entry 0x%08x is no instruction of the text", prog.entry);
    const std::vector<uint32_t> classes = calltree::instr_classes(prog);
    CalltreeRun ct{p, {}};
    auto prefix = [&](const ShardJob &s, size_t *take, uint32_t *succ) {
        *take = s.index < shard ? s.n_recs : s.index == shard ? std::min<size_t>(s.n_recs, row) : 0;
        *succ = *take < s.n_recs ? idx_at : prof::index_of_pc(prog, s.next_pc);
    };
    if (int rc = calltree_summaries(p, j, classes, 0, true, prefix, &ct)) return rc;
    std::vector<calltree::Frame> stack;
    uint64_t unmatched = 0, before_shard = 0;
    if (position) stack.push_back(calltree::Frame{entry, 0});
    for (size_t pos = 0; pos < j->n_total && position; pos++) {
        size_t m = 0;
        const ShardJob *s = j->at(pos, &m);
        CalltreeMember &cm = *ct.mem[m];
        const size_t k = (size_t)(s - j->parts[m].shards.data());
        const size_t n_spans = (cm.n_of[k] + CALLTREE_SPAN - 1) / CALLTREE_SPAN;
        for (size_t i = 0; i < n_spans; i++) {
            const size_t span = cm.span0[k] + i;
            unmatched += calltree_merge_span(stack, cm.summaries[span], cm.h_calls.data() + cm.calls_at[span], before_shard + i * CALLTREE_SPAN);
        }
        before_shard += s->n_recs;
    }

    // ---- the members' winners, merged
    std::vector<unsigned long long> win(table_words, 0), one(table_words);
    std::fill(win.begin() + 33 + W, win.end(), ~0ull);
    for (size_t m = 0; m < G; m++) {
        SnapMember &sm = *run.mem[m];
        if (!sm.d_tables) continue;
        if (int rc = turn_to(p, m)) return rc;
        Engine &e = lane0(p, m).eng;
        if (!e.download(one.data(), sm.d_tables, table_words * 8)) return engine_fail(p->err, e);
        win[0] += one[0];
        for (size_t i = 1; i < 33 + W; i++) win[i] = std::max(win[i], one[i]);
        for (size_t i = 33 + W; i < table_words; i++) win[i] = std::min(win[i], one[i]);
    }
    if (turn_to(p, 0)) return DVT_ERR_DEVICE;
    if (win[0]) return fail(p, DVT_ERR_INPUT, "%llu cycle records name an instruction outside the text or an address outside guest memory", win[0]);

    // ---- gather: every winner from the member that holds its shard; the call records of the frames that are returned
    struct Want { size_t m, at; uint32_t what, index; };
    std::vector<Want> wants;
    auto want = [&](unsigned long long where, uint32_t addr, uint32_t what, uint32_t index) {
        const uint32_t sh = (uint32_t)(where >> 32), rw = (uint32_t)where;
        size_t m = 0;
        const ShardJob *s = sh ? j->at(sh - 1, &m) : nullptr;
        if (!s || rw >= s->n_recs) return false;
        wants.push_back({m, run.mem[m]->fetch.size(), what, index});
        run.mem[m]->fetch.push_back(SnapFetch{s->d_recs, (uint32_t)s->n_recs, sh, rw, addr, what, 0});
        return true;
    };
    bool ok = true;
    for (uint32_t k = 1; k < 32; k++)
        if (win[1 + k]) ok = ok && want(win[1 + k], k, snap::WHAT_REG, k);
    for (uint32_t r = 0; r < rg.n; r++)
        for (uint32_t addr = rg.lo[r]; addr < rg.hi[r]; addr += 4) {
            const uint32_t slot = rg.at[r] + (addr - rg.lo[r]) / 4;
            if (win[33 + slot]) ok = ok && want(win[33 + slot], addr, snap::WHAT_BEFORE, slot);
            if (win[33 + W + slot] != ~0ull) ok = ok && want(win[33 + W + slot], addr, snap::WHAT_AFTER, slot);
        }
    const size_t depth = stack.size(), nf = std::min(depth, cap_frames);
    for (size_t f = 0; f < nf; f++) {
        const uint64_t open = stack[depth - 1 - f].open;
        if (!open) continue;   // (the root)
        uint32_t sh = 1, rw = 0;
        snap::locate(shard_n, open - 1, &sh, &rw);
        ok = ok && want(watch::position(sh, rw), 0, snap::WHAT_FRAME, (uint32_t)(depth - 1 - f));
    }
    if (!ok) return fail(p, DVT_ERR_DEVICE, "a winner of the reduce pass lies in no shard of the job");
    for (size_t m = 0; m < G; m++) {
        SnapMember &sm = *run.mem[m];
        if (sm.fetch.empty()) continue;
        if (int rc = turn_to(p, m)) return rc;
        const Lane c = lane0(p, m);
        Engine &e = c.eng;
        HIP_TRY(c.err, e.pool.alloc_bytes(&sm.items.ptr, sm.fetch.size() * sizeof(SnapFetch)));
        HIP_TRY(c.err, e.pool.alloc_bytes(&sm.sides.ptr, sm.fetch.size() * sizeof(snap::Side)));
        HIP_TRY(c.err, hipMemcpyAsync(sm.items.ptr, sm.fetch.data(), sm.fetch.size() * sizeof(SnapFetch), hipMemcpyHostToDevice, e.stream));
        args.statics = sm.d_statics; args.offs = sm.d_statics + n; args.shard = 0;
        HIP_TRY(c.err, hipEventRecord(sm.ev[2], e.stream));
        HIP_TRY(c.err, launch_snapshot_gather(e.stream, static_cast<const SnapFetch *>(sm.items.ptr), (uint32_t)sm.fetch.size(), args, sm.sides.ptr));
        HIP_TRY(c.err, hipEventRecord(sm.ev[3], e.stream));
        sm.gathered = true;
        sm.got.resize(sm.fetch.size());
        if (!e.download(sm.got.data(), sm.sides.ptr, sm.got.size() * sizeof(snap::Side))) return engine_fail(c.err, e);
    }
    double ms[3] = {0, 0, 0};
    for (size_t m = 0; m < G; m++) {
        SnapMember &sm = *run.mem[m];
        CalltreeMember &cm = *ct.mem[m];
        if (!sm.ev[0] && !cm.ev[0]) continue;
        if (int rc = turn_to(p, m)) return rc;
        float t = 0;
        if (sm.ev[0] && hipEventElapsedTime(&t, sm.ev[0], sm.ev[1]) == hipSuccess) ms[0] += t;
        if (sm.gathered && hipEventElapsedTime(&t, sm.ev[2], sm.ev[3]) == hipSuccess) ms[1] += t;
        if (cm.ev[0] && hipEventElapsedTime(&t, cm.ev[0], cm.ev[1]) == hipSuccess) ms[2] += t;
        if (cm.timed_calls && hipEventElapsedTime(&t, cm.ev[2], cm.ev[3]) == hipSuccess) ms[2] += t;
    }
    if (turn_to(p, 0)) return DVT_ERR_DEVICE;

    snap::Side reg[32] = {};
    std::vector<snap::Side> before(W, snap::Side{}), after(W, snap::Side{});
    std::vector<snap::CallRec> calls(depth);
    for (const Want &w : wants) {
        const snap::Side &s = run.mem[w.m]->got[w.at];
        if (s.kind == snap::SIDE_BAD || s.kind == snap::SIDE_NONE)
            return fail(p, DVT_ERR_DEVICE, "the record at shard %u, row %u is not the access the reduce pass saw", s.shard, s.row);
        if (w.what == snap::WHAT_REG) reg[w.index] = s;
        else if (w.what == snap::WHAT_BEFORE) before[w.index] = s;
        else if (w.what == snap::WHAT_AFTER) after[w.index] = s;
        else calls[w.index] = snap::CallRec{s.pc, s.value};
    }
    for (int i = 0; i < 3; i++) p->snap_ms[i] = ms[i];
    const snap::Parts parts{reg, before.data(), after.data(), &stack, &calls, &shard_n, position, cycles, unmatched, pc};
    snap::emit(prog, rg, parts, ms_since(t0), regs, words, frames, cap_frames, summary);
    return DVT_OK;
}

// The host-only reports (no GPU is touched): the guest in trace mode, where an instruction without a chip is recorded instead
// of trapping, 2^log_shard (2^21) cycles per shard and one shard's records in memory at a time.  begin(prog) once the ELF is loaded;
// shard(prog, recs, n, last_succ) per shard in execution order; end(prog, ms) after the last, and a text it returns fails the
// call with DVT_ERR_UNSUPPORTED.  Return codes, *report and *err_text as dvt_execute gives them; end runs for whatever retired,
// also when the guest fails.
template <class Begin, class Shard, class End>
static int execute_traced(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint64_t max_cycles, dvt_report *report,
                          char **err_text, Begin begin, Shard shard, End end, uint32_t log_shard = 21) {
    const auto t0 = Clock::now();
    rv32::Program prog;
    std::string err;
    if (!rv32::load_elf(elf, elf_len, &prog, &err)) {
        if (err_text) *err_text = strdup(("ELF: " + err).c_str());
        return DVT_ERR_INPUT;
    }
    const uint32_t LOG_SHARD = log_shard;
    std::vector<std::vector<uint8_t>> inputs(nbuf);
    for (size_t i = 0; i < nbuf; i++)
        if (stdin_bufs[i].len) inputs[i].assign(stdin_bufs[i].data, stdin_bufs[i].data + stdin_bufs[i].len);
    rv32::Vm vm(prog, &inputs, LOG_SHARD);
    vm.trace_unprovable = true;
    const std::unique_ptr<rv32::CycleRec[]> recs(new rv32::CycleRec[(size_t)1 << LOG_SHARD]);   // (pages a short run never touches cost nothing)
    rv32::ShardOut so;
    so.recs = recs.get();
    begin(prog);
    for (;;) {
        vm.run_shard(true, &so, max_cycles ? max_cycles : ~0ull);
        if constexpr (std::is_invocable_v<Shard, const rv32::Program &, const rv32::CycleRec *, size_t, uint32_t, uint32_t>)
            shard(prog, so.recs, so.n_recs, prof::index_of_pc(prog, so.next_pc), so.next_pc);   // (a report that wants the pc itself)
        else
            shard(prog, so.recs, so.n_recs, prof::index_of_pc(prog, so.next_pc));
        if (vm.halted || !vm.error.empty() || !vm.next_shard()) break;
    }
    if (report) {
        report->cycles = vm.cycles;
        report->exit_code = vm.halted ? vm.exit_code : -1;
        report->halted = vm.halted;
        report->unprovable = vm.unsupported;
    }
    if (const char *why = end(prog, ms_since(t0))) {
        if (err_text) *err_text = strdup(why);
        return DVT_ERR_UNSUPPORTED;
    }
    if (!vm.error.empty()) {
        if (err_text) *err_text = strdup(vm.error.c_str());
        return DVT_ERR_GUEST;
    }
    if (vm.exit_code != 0) {
        if (err_text) *err_text = strdup("guest halted with a non-zero exit code");
        return DVT_ERR_GUEST;
    }
    return DVT_OK;
}

extern "C" {

// ---- the execution report (profile.h)
int dvt_rv32_job_profile(dvt_prover *p, const dvt_pk *pk, dvt_job *job, uint32_t log_edge_slots, uint64_t *pc_count, size_t cap_pc,
                         dvt_profile_edge *edges, size_t cap_edges, dvt_profile_syscall *sys, size_t cap_sys, dvt_profile_opcode *ops,
                         size_t cap_ops, dvt_profile_summary *summary) {
    const prof::Out out{pc_count, cap_pc, edges, cap_edges, sys, cap_sys, ops, cap_ops, summary};
    if (!p || !pk || !job || !summary || out.null_array()) return fail(p, DVT_ERR_INPUT, "null argument");
    if (int rc = rv32_key(p, pk)) return rc;
    if (log_edge_slots && (log_edge_slots < prof::MIN_LOG_SLOTS || log_edge_slots > prof::MAX_LOG_SLOTS))
        return fail(p, DVT_ERR_INPUT, "log_edge_slots %u (0 or %u..%u)", log_edge_slots, prof::MIN_LOG_SLOTS, prof::MAX_LOG_SLOTS);
    Guard g(p); if (g.rc) return g.rc;
    return job_profile(p, pk, job, log_edge_slots, out);
}

// host-only: the same rule (prof::tally_records) over execute_traced's shards
int dvt_execute_profile(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint64_t max_cycles, uint64_t *pc_count,
                        size_t cap_pc, dvt_profile_edge *edges, size_t cap_edges, dvt_profile_syscall *sys, size_t cap_sys,
                        dvt_profile_opcode *ops, size_t cap_ops, dvt_profile_summary *summary, dvt_report *report, char **err_text) {
    if (err_text) *err_text = nullptr;
    const prof::Out out{pc_count, cap_pc, edges, cap_edges, sys, cap_sys, ops, cap_ops, summary};
    if (!elf || (nbuf && !stdin_bufs) || !summary || out.null_array()) return DVT_ERR_INPUT;
    std::unique_ptr<prof::Tally> t;
    return execute_traced(
        elf, elf_len, stdin_bufs, nbuf, max_cycles, report, err_text, [&](const rv32::Program &prog) { t.reset(new prof::Tally(prog)); },
        [&](const rv32::Program &prog, const rv32::CycleRec *recs, size_t n, uint32_t last_succ) { prof::tally_records(prog, recs, n, last_succ, t.get()); },
        [&](const rv32::Program &prog, double ms) { return prof::emit(prog, *t, t->shards, ms, out) ? nullptr : "more than 64 distinct syscall ids"; });
}

// ---- the call-tree report (calltree.h)
int dvt_rv32_job_calltree(dvt_prover *p, const dvt_pk *pk, dvt_job *job, uint32_t log_arc_slots, dvt_calltree_arc *arcs, size_t cap_arcs,
                          dvt_calltree_func *funcs, size_t cap_funcs, dvt_calltree_summary *summary) {
    const calltree::Out out{arcs, cap_arcs, funcs, cap_funcs, summary};
    if (!p || !pk || !job || !summary || out.null_array()) return fail(p, DVT_ERR_INPUT, "null argument");
    if (int rc = rv32_key(p, pk)) return rc;
    if (log_arc_slots && (log_arc_slots < prof::MIN_LOG_SLOTS || log_arc_slots > prof::MAX_LOG_SLOTS))
        return fail(p, DVT_ERR_INPUT, "log_arc_slots %u (0 or %u..%u)", log_arc_slots, prof::MIN_LOG_SLOTS, prof::MAX_LOG_SLOTS);
    Guard g(p); if (g.rc) return g.rc;
    return job_calltree(p, pk, job, log_arc_slots, out);
}

int dvt_rv32_job_calltree_times(dvt_prover *p, double out[3]) {
    if (!p || !out) return DVT_ERR_INPUT;
    std::lock_guard<std::mutex> lk(p->mu);
    for (int i = 0; i < 3; i++) out[i] = p->calltree_ms[i];
    return DVT_OK;
}

// host-only: the same rule (calltree::walk_records) over execute_traced's shards
int dvt_execute_calltree(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint64_t max_cycles, dvt_calltree_arc *arcs,
                         size_t cap_arcs, dvt_calltree_func *funcs, size_t cap_funcs, dvt_calltree_summary *summary, dvt_report *report,
                         char **err_text) {
    if (err_text) *err_text = nullptr;
    const calltree::Out out{arcs, cap_arcs, funcs, cap_funcs, summary};
    if (!elf || (nbuf && !stdin_bufs) || !summary || out.null_array()) return DVT_ERR_INPUT;
    std::unique_ptr<calltree::State> st;
    uint32_t shards = 0;
    return execute_traced(
        elf, elf_len, stdin_bufs, nbuf, max_cycles, report, err_text, [&](const rv32::Program &prog) { st.reset(new calltree::State(prog)); },
        [&](const rv32::Program &prog, const rv32::CycleRec *recs, size_t n, uint32_t last_succ) {
            calltree::walk_records(prog, recs, n, last_succ, st->cycles, st.get());
            shards++;
        },
        [&](const rv32::Program &prog, double ms) -> const char * {
            st->finish();
            calltree::emit(prog, *st, shards, ms, out);
            return nullptr;
        });
}

// ---- the memory report (memreport.h)
int dvt_rv32_job_memory(dvt_prover *p, const dvt_pk *pk, dvt_job *job, uint64_t *first_touch, size_t cap_instr, dvt_memory_page *pages,
                        size_t cap_pages, dvt_memory_summary *summary) {
    const memrep::Out out{first_touch, cap_instr, pages, cap_pages, summary};
    if (!p || !pk || !job || !summary || out.null_array()) return fail(p, DVT_ERR_INPUT, "null argument");
    if (int rc = rv32_key(p, pk)) return rc;
    Guard g(p); if (g.rc) return g.rc;
    return job_memory(p, pk, job, out);
}

// host-only: the same rule (memrep::tally_records) over execute_traced's shards
int dvt_execute_memory(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint64_t max_cycles, uint64_t *first_touch,
                       size_t cap_instr, dvt_memory_page *pages, size_t cap_pages, dvt_memory_summary *summary, dvt_report *report,
                       char **err_text) {
    if (err_text) *err_text = nullptr;
    const memrep::Out out{first_touch, cap_instr, pages, cap_pages, summary};
    if (!elf || (nbuf && !stdin_bufs) || !summary || out.null_array()) return DVT_ERR_INPUT;
    std::unique_ptr<memrep::Tally> t;
    const std::vector<memrep::PreShape> shapes = memrep::pre_shapes();
    return execute_traced(
        elf, elf_len, stdin_bufs, nbuf, max_cycles, report, err_text, [&](const rv32::Program &prog) { t.reset(new memrep::Tally(prog)); },
        [&](const rv32::Program &prog, const rv32::CycleRec *recs, size_t n, uint32_t) { memrep::tally_records(prog, shapes, recs, n, t.get()); },
        [&](const rv32::Program &prog, double ms) -> const char * {
            memrep::emit(prog, *t, t->shards, true, ms, out);
            return nullptr;
        });
}

// ---- watchpoints (watch.h)
int dvt_rv32_job_watch(dvt_prover *p, const dvt_pk *pk, dvt_job *job, const dvt_watch_query *queries, size_t n_queries, size_t cap_each,
                       dvt_watch_hit *hits, uint64_t *totals, dvt_watch_summary *summary) {
    if (!p || !pk || !job || !summary) return fail(p, DVT_ERR_INPUT, "null argument");
    std::string text;
    if (const char *why = watch::input_error(queries, n_queries, cap_each, hits, totals, &text)) return fail(p, DVT_ERR_INPUT, "%s", why);
    if (int rc = rv32_key(p, pk)) return rc;
    Guard g(p); if (g.rc) return g.rc;
    return job_watch(p, pk, job, queries, n_queries, (uint32_t)cap_each, hits, totals, summary);
}

int dvt_rv32_job_watch_times(dvt_prover *p, double out[4]) {
    if (!p || !out) return DVT_ERR_INPUT;
    std::lock_guard<std::mutex> lk(p->mu);
    for (int i = 0; i < 4; i++) out[i] = p->watch_ms[i];
    return DVT_OK;
}

// host-only: the same rule (watch::scan_records) over execute_traced's shards
int dvt_execute_watch(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint64_t max_cycles, uint32_t log_shard_size,
                      const dvt_watch_query *queries, size_t n_queries, size_t cap_each, dvt_watch_hit *hits, uint64_t *totals,
                      dvt_watch_summary *summary, dvt_report *report, char **err_text) {
    if (err_text) *err_text = nullptr;
    if (!elf || (nbuf && !stdin_bufs) || !summary) return DVT_ERR_INPUT;
    std::string text;
    if (log_shard_size && (log_shard_size < 4 || log_shard_size > 22)) text = "log_shard_size must be 0 or 4..22";
    if (!text.empty() || watch::input_error(queries, n_queries, cap_each, hits, totals, &text)) {
        if (err_text) *err_text = strdup(text.c_str());
        return DVT_ERR_INPUT;
    }
    std::unique_ptr<watch::Search> s;
    return execute_traced(
        elf, elf_len, stdin_bufs, nbuf, max_cycles, report, err_text,
        [&](const rv32::Program &prog) { s.reset(new watch::Search(prog, queries, n_queries, (uint32_t)cap_each)); },
        [&](const rv32::Program &prog, const rv32::CycleRec *recs, size_t n, uint32_t) { watch::scan_records(prog, recs, n, s->shards + 1, s.get()); },
        [&](const rv32::Program &prog, double ms) -> const char * {
            watch::emit(prog, *s, s->shards, ms, hits, totals, summary);
            return s->bad ? "cycle records name an instruction outside the text or an address outside guest memory" : nullptr;
        },
        log_shard_size ? log_shard_size : 21);
}

// ---- snapshots (snapshot.h)
int dvt_rv32_job_snapshot(dvt_prover *p, const dvt_pk *pk, dvt_job *job, uint32_t shard, uint32_t row, const dvt_snap_range *ranges, size_t n_ranges,
                          dvt_snap_cell regs[32], dvt_snap_cell *words, size_t cap_words, dvt_snap_frame *frames, size_t cap_frames,
                          dvt_snap_summary *summary) {
    if (!p || !pk || !job || !summary) return fail(p, DVT_ERR_INPUT, "null argument");
    std::string text;
    snap::Ranges rg;
    if (const char *why = snap::input_error(ranges, n_ranges, regs, words, cap_words, frames, cap_frames, &rg, &text)) return fail(p, DVT_ERR_INPUT, "%s", why);
    if (int rc = rv32_key(p, pk)) return rc;
    Guard g(p); if (g.rc) return g.rc;
    return job_snapshot(p, pk, job, shard, row, rg, regs, words, frames, cap_frames, summary);
}

int dvt_rv32_job_snapshot_times(dvt_prover *p, double out[3]) {
    if (!p || !out) return DVT_ERR_INPUT;
    std::lock_guard<std::mutex> lk(p->mu);
    for (int i = 0; i < 3; i++) out[i] = p->snap_ms[i];
    return DVT_OK;
}

// host-only: the same rule (snap::Taker) over execute_traced's shards
int dvt_execute_snapshot(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint64_t max_cycles, uint32_t log_shard_size,
                         uint32_t shard, uint32_t row, const dvt_snap_range *ranges, size_t n_ranges, dvt_snap_cell regs[32], dvt_snap_cell *words,
                         size_t cap_words, dvt_snap_frame *frames, size_t cap_frames, dvt_snap_summary *summary, dvt_report *report,
                         char **err_text) {
    if (err_text) *err_text = nullptr;
    if (!elf || (nbuf && !stdin_bufs) || !summary) return DVT_ERR_INPUT;
    std::string text;
    snap::Ranges rg;
    if (log_shard_size && (log_shard_size < 4 || log_shard_size > 22)) text = "log_shard_size must be 0 or 4..22";
    if (!text.empty() || snap::input_error(ranges, n_ranges, regs, words, cap_words, frames, cap_frames, &rg, &text)) {
        if (err_text) *err_text = strdup(text.c_str());
        return DVT_ERR_INPUT;
    }
    std::unique_ptr<snap::Taker> t;
    return execute_traced(
        elf, elf_len, stdin_bufs, nbuf, max_cycles, report, err_text, [&](const rv32::Program &prog) { t.reset(new snap::Taker(prog, rg, shard, row)); },
        [&](const rv32::Program &prog, const rv32::CycleRec *recs, size_t n, uint32_t, uint32_t next_pc) {
            t->scan(prog, recs, n, (uint32_t)t->shard_n.size() + 1, next_pc);
        },
        [&](const rv32::Program &prog, double ms) -> const char * {
            t->emit(prog, ms, regs, words, frames, cap_frames, summary);
            return t->bad ? "cycle records name an instruction outside the text or an address outside guest memory" : nullptr;
        },
        log_shard_size ? log_shard_size : 21);
}

// ---- the trace-row checks of one chip (check.cuh)
int dvt_stage_check_constraints(dvt_prover *p, const char *machine, uint32_t chip, const uint32_t *d_main, const uint32_t *d_prep,
                                uint32_t log_n, const uint32_t *pub, const uint32_t xi[4], uint32_t *counts, dvt_check_result *out) {
    if (!p) return DVT_ERR_INPUT;
    if (!xi || !out) return fail(p, DVT_ERR_INPUT, "null argument");
    ChipStageArgs a;
    CheckChallenges ch{Fp4::zero(), Fp4::zero(), Fp4::zero()};
    if (!ext_from_canonical(xi, &ch.xi)) return fail(p, DVT_ERR_INPUT, "xi not canonical");
    if (int rc = stage_table(p, machine, chip, d_main, d_prep, log_n, pub, &a)) return rc;
    Guard g(p); if (g.rc) return g.rc;
    std::vector<CheckTableOut> res;
    if (int rc = check_tables(lane0(p), a.m, {a.t}, a.pub, ch, true, false, &res)) return rc;
    if (counts) memcpy(counts, res[0].counts.data(), res[0].counts.size() * 4);
    *out = res[0].r;
    return DVT_OK;
}

int dvt_stage_bus_sums(dvt_prover *p, const char *machine, uint32_t chip, const uint32_t *d_main, const uint32_t *d_prep, uint32_t log_n,
                       const uint32_t *pub, const uint32_t perm_alpha[4], const uint32_t beta[4], uint32_t out[DVT_CHECK_BUSES][4]) {
    if (!p) return DVT_ERR_INPUT;
    if (!out) return fail(p, DVT_ERR_INPUT, "null argument");
    ChipStageArgs a;
    if (int rc = stage_table(p, machine, chip, d_main, d_prep, log_n, pub, &a, perm_alpha, beta)) return rc;
    const CheckChallenges ch{Fp4::zero(), a.perm_alpha, a.beta};
    Guard g(p); if (g.rc) return g.rc;
    std::vector<CheckTableOut> res;
    if (int rc = check_tables(lane0(p), a.m, {a.t}, a.pub, ch, false, true, &res)) return rc;
    for (uint32_t b = 0; b < DVT_CHECK_BUSES; b++)
        for (int k = 0; k < 4; k++) out[b][k] = res[0].bus[b].c[k].canonical();
    return DVT_OK;
}

// ---- the bus ledger of chip tables (ledger.cuh), on lane 0 of member 0
static int ledger_stage_rows(dvt_prover *p, dvt_bus_ledger *l, uint32_t chip, const uint32_t *d_main, const uint32_t *d_prep, uint32_t log_n,
                             const uint32_t *pub, uint32_t tag, bool collect) {
    if (!p) return DVT_ERR_INPUT;
    if (!l) return fail(p, DVT_ERR_INPUT, "null ledger");
    if (l->closed != collect) return fail(p, DVT_ERR_INPUT, collect ? "collect before close" : "add after close");
    ChipStageArgs a;
    if (int rc = stage_table(p, l->m->name, chip, d_main, d_prep, log_n, pub, &a)) return rc;
    if (tag >= (1u << 16)) return fail(p, DVT_ERR_INPUT, "tag %u >= 2^16", tag);
    if (collect && !l->n_dirty) return DVT_OK;
    Guard g(p); if (g.rc) return g.rc;
    if (int rc = ledger_rows(lane0(p), l->dev, a.t, chip, a.pub, tag, collect)) return rc;
    HIP_TRY(p, hipStreamSynchronize(eng0(p).stream));
    return DVT_OK;
}

int dvt_stage_bus_ledger_new(dvt_prover *p, const char *machine, uint32_t log_buckets, uint32_t cap_slots, uint64_t seed, dvt_bus_ledger **ledger) {
    if (!p) return DVT_ERR_INPUT;
    if (!ledger) return fail(p, DVT_ERR_INPUT, "null argument");
    *ledger = nullptr;
    const MachineDesc *m = machine_by_name(machine);
    if (!m) return fail(p, DVT_ERR_INPUT, "unknown machine '%s'", machine ? machine : "(null)");
    Guard g(p); if (g.rc) return g.rc;
    std::unique_ptr<dvt_bus_ledger> l(new dvt_bus_ledger());
    l->m = m;
    if (int rc = ledger_init(lane0(p), &l->dev, log_buckets, cap_slots, seed)) return rc;
    HIP_TRY(p, hipStreamSynchronize(eng0(p).stream));
    *ledger = l.release();
    return DVT_OK;
}

int dvt_stage_bus_ledger_add(dvt_prover *p, dvt_bus_ledger *ledger, uint32_t chip, const uint32_t *d_main, const uint32_t *d_prep,
                             uint32_t log_n, const uint32_t *pub, uint32_t tag) {
    return ledger_stage_rows(p, ledger, chip, d_main, d_prep, log_n, pub, tag, false);
}

int dvt_stage_bus_ledger_collect(dvt_prover *p, dvt_bus_ledger *ledger, uint32_t chip, const uint32_t *d_main, const uint32_t *d_prep,
                                 uint32_t log_n, const uint32_t *pub, uint32_t tag) {
    return ledger_stage_rows(p, ledger, chip, d_main, d_prep, log_n, pub, tag, true);
}

int dvt_stage_bus_ledger_add_tuple(dvt_prover *p, dvt_bus_ledger *ledger, uint32_t bus, const uint32_t *values, uint32_t arity, int32_t sign,
                                   uint32_t mult, uint32_t tag) {
    if (!p) return DVT_ERR_INPUT;
    if (!ledger || (arity && !values)) return fail(p, DVT_ERR_INPUT, "null argument");
    if (ledger->closed && !ledger->n_dirty) return DVT_OK;
    Guard g(p); if (g.rc) return g.rc;
    if (int rc = ledger_tuple(lane0(p), ledger->dev, bus, values, arity, sign, mult, tag, ledger->closed)) return rc;
    HIP_TRY(p, hipStreamSynchronize(eng0(p).stream));
    return DVT_OK;
}

int dvt_stage_bus_ledger_close(dvt_prover *p, dvt_bus_ledger *ledger, uint32_t *n_dirty) {
    if (!p) return DVT_ERR_INPUT;
    if (!ledger || !n_dirty) return fail(p, DVT_ERR_INPUT, "null argument");
    if (ledger->closed) return fail(p, DVT_ERR_INPUT, "the ledger is closed already");
    Guard g(p); if (g.rc) return g.rc;
    if (int rc = ledger_close(lane0(p), ledger->dev, &ledger->n_dirty)) return rc;
    ledger->closed = true;
    *n_dirty = ledger->n_dirty;
    return DVT_OK;
}

int dvt_stage_bus_ledger_result(dvt_prover *p, dvt_bus_ledger *ledger, dvt_bus_tuple *out, size_t cap, size_t *n_tuples, uint32_t *truncated) {
    if (!p) return DVT_ERR_INPUT;
    if (!ledger || !n_tuples || !truncated || (cap && !out)) return fail(p, DVT_ERR_INPUT, "null argument");
    if (!ledger->closed) return fail(p, DVT_ERR_INPUT, "result before close");
    Guard g(p); if (g.rc) return g.rc;
    std::vector<dvt_bus_tuple> all;
    bool overflow = false;
    if (int rc = ledger_records(lane0(p), ledger->dev, &all, &overflow)) return rc;
    ledger_finish(&all);
    ledger_copy_out(all, overflow, out, cap, n_tuples, truncated);
    return DVT_OK;
}

int dvt_stage_bus_ledger_free(dvt_prover *p, dvt_bus_ledger *ledger) {
    if (!p) return DVT_ERR_INPUT;
    if (!ledger) return fail(p, DVT_ERR_INPUT, "null ledger");
    Guard g(p); if (g.rc) return g.rc;
    (void)hipStreamSynchronize(eng0(p).stream);
    ledger_release(&ledger->dev);
    delete ledger;
    return DVT_OK;
}

// ---- the forgery hunt of one chip table (hunt.cuh), on lane 0 of member 0
static int hunt_stage(dvt_prover *p, const char *machine, uint32_t chip, const uint32_t *d_main, const uint32_t *d_prep, uint32_t log_n,
                      const uint32_t *pub, const HuntRequest &rq) {
    if (!p) return DVT_ERR_INPUT;
    ChipStageArgs a;
    if (int rc = stage_table(p, machine, chip, d_main, d_prep, log_n, pub, &a)) return rc;
    HuntPlan plan;
    if (int rc = hunt_plan(p->err, *a.t.d, log_n, rq, &plan)) return rc;
    Guard g(p); if (g.rc) return g.rc;
    return hunt_table(lane0(p), a.m, a.t, a.pub, rq, plan);
}

int dvt_stage_hunt_cells(dvt_prover *p, const char *machine, uint32_t chip, const uint32_t *d_main, const uint32_t *d_prep,
                         uint32_t log_n, const uint32_t *pub, uint64_t seed, const uint32_t *deltas, uint32_t n_deltas,
                         uint32_t row_first, uint32_t row_count, uint64_t max_evals, uint32_t *free_counts, uint8_t *free_map) {
    HuntRequest rq = hunt_request(seed, deltas, n_deltas, row_first, row_count, max_evals);
    hunt_want_cells(&rq, free_counts, free_map);
    return hunt_stage(p, machine, chip, d_main, d_prep, log_n, pub, rq);
}

int dvt_stage_hunt_pairs(dvt_prover *p, const char *machine, uint32_t chip, const uint32_t *d_main, const uint32_t *d_prep,
                         uint32_t log_n, const uint32_t *pub, uint64_t seed, const uint32_t *deltas, uint32_t n_deltas,
                         const uint32_t *cols, uint32_t n_cols, uint32_t adjacent, uint32_t row_first, uint32_t row_count,
                         uint64_t max_evals, dvt_escape *out, size_t cap, uint64_t *n_reported, uint64_t *n_tried) {
    HuntRequest rq = hunt_request(seed, deltas, n_deltas, row_first, row_count, max_evals);
    hunt_want_pairs(&rq, cols, n_cols, adjacent, out, cap, n_reported, n_tried);
    return hunt_stage(p, machine, chip, d_main, d_prep, log_n, pub, rq);
}

// ---- the join hunt over windows of several chip tables (hunt_join.cuh), on lane 0 of member 0
int dvt_stage_hunt_join_new(dvt_prover *p, const char *machine, uint64_t seed, const uint32_t *deltas, uint32_t n_deltas, size_t cap_records,
                            size_t cap_absorbed, uint32_t log_slots, dvt_hunt_join **join) {
    if (!p) return DVT_ERR_INPUT;
    if (!join) return fail(p, DVT_ERR_INPUT, "null argument");
    *join = nullptr;
    const MachineDesc *m = machine_by_name(machine);
    if (!m) return fail(p, DVT_ERR_INPUT, "unknown machine '%s'", machine ? machine : "(null)");
    Guard g(p); if (g.rc) return g.rc;
    std::unique_ptr<dvt_hunt_join> j(new dvt_hunt_join());
    if (int rc = join_init(lane0(p), &j->dev, m, seed, deltas, n_deltas, cap_records, cap_absorbed, log_slots)) {
        join_release(&j->dev);
        return rc;
    }
    HIP_TRY(p, hipStreamSynchronize(eng0(p).stream));
    *join = j.release();
    return DVT_OK;
}

int dvt_stage_hunt_join_supply(dvt_prover *p, dvt_hunt_join *join, uint32_t chip, const uint32_t *d_main, const uint32_t *d_prep, uint32_t log_n,
                               const uint32_t *pub) {
    if (!p) return DVT_ERR_INPUT;
    if (!join) return fail(p, DVT_ERR_INPUT, "null join");
    ChipStageArgs a;
    if (int rc = stage_table(p, join->dev.m->name, chip, d_main, d_prep, log_n, pub, &a)) return rc;
    Guard g(p); if (g.rc) return g.rc;
    return join_supply(p->err, join->dev, a.t, a.pub);
}

int dvt_stage_hunt_join_add(dvt_prover *p, dvt_hunt_join *join, uint32_t tag, uint32_t chip, const uint32_t *d_main, const uint32_t *d_prep,
                            uint32_t log_n, const uint32_t *pub, uint32_t row_first, uint32_t row_count, const uint32_t *cols, uint32_t n_cols,
                            uint64_t max_evals) {
    if (!p) return DVT_ERR_INPUT;
    if (!join) return fail(p, DVT_ERR_INPUT, "null join");
    ChipStageArgs a;
    if (int rc = stage_table(p, join->dev.m->name, chip, d_main, d_prep, log_n, pub, &a)) return rc;
    std::vector<uint32_t> cl;
    if (int rc = join_check_add(p->err, join->dev, tag, chip, *a.t.d, log_n, row_first, row_count, cols, n_cols, max_evals, &cl)) return rc;
    Guard g(p); if (g.rc) return g.rc;
    return join_add(lane0(p), join->dev, tag, chip, a.t, a.pub, row_first, row_count, cl);
}

int dvt_stage_hunt_join_match(dvt_prover *p, dvt_hunt_join *join, dvt_join_summary *summary) {
    if (!p) return DVT_ERR_INPUT;
    if (!join || !summary) return fail(p, DVT_ERR_INPUT, "null argument");
    Guard g(p); if (g.rc) return g.rc;
    if (int rc = join_match(lane0(p), join->dev)) return rc;
    *summary = join->dev.summary;
    return DVT_OK;
}

int dvt_stage_hunt_join_result(dvt_prover *p, dvt_hunt_join *join, dvt_join_cell *cells, size_t cap_cells, size_t *n_cells, dvt_join_cell *absorbed,
                               size_t cap_absorbed, size_t *n_absorbed) {
    if (!p) return DVT_ERR_INPUT;
    if (!join || !n_cells || !n_absorbed || (cap_cells && !cells) || (cap_absorbed && !absorbed)) return fail(p, DVT_ERR_INPUT, "null argument");
    Guard g(p); if (g.rc) return g.rc;
    if (!join->dev.matched) return fail(p, DVT_ERR_INPUT, "result before match");
    const JoinDev &j = join->dev;
    std::copy_n(j.cells.begin(), std::min(cap_cells, j.cells.size()), cells);
    std::copy_n(j.absorbed.begin(), std::min(cap_absorbed, j.absorbed.size()), absorbed);
    *n_cells = j.cells.size();
    *n_absorbed = j.absorbed.size();
    return DVT_OK;
}

int dvt_stage_hunt_join_free(dvt_prover *p, dvt_hunt_join *join) {
    if (!p) return DVT_ERR_INPUT;
    if (!join) return fail(p, DVT_ERR_INPUT, "null join");
    Guard g(p); if (g.rc) return g.rc;
    (void)hipStreamSynchronize(eng0(p).stream);
    join_release(&join->dev);
    delete join;
    return DVT_OK;
}

uint64_t dvt_debug_ledger_key(uint64_t seed, uint32_t bus, uint32_t arity, const uint32_t *values) {
    return values || !arity ? ledger_key(seed, bus, arity, values) : 0;
}

int dvt_rv32_job_bus_tuples(dvt_prover *p, const dvt_pk *pk, dvt_job *job, dvt_bus_tuple *out, size_t cap, size_t *n_tuples, uint32_t *truncated) {
    if (!p) return DVT_ERR_INPUT;
    if (!pk || !job || !n_tuples || !truncated || (cap && !out)) return fail(p, DVT_ERR_INPUT, "null argument");
    if (int rc = rv32_key(p, pk)) return rc;
    Guard g(p); if (g.rc) return g.rc;
    return job_bus_tuples(p, pk, job, out, cap, n_tuples, truncated);
}

int dvt_rv32_check_job(dvt_prover *p, const dvt_pk *pk, dvt_job *job, dvt_check_finding *findings, size_t cap, dvt_check_summary *summary) {
    if (!p || !pk || !job || !summary || (cap && !findings)) return fail(p, DVT_ERR_INPUT, "null argument");
    if (int rc = rv32_key(p, pk)) return rc;
    Guard g(p); if (g.rc) return g.rc;
    return job_check(p, pk, job, findings, cap, summary);
}

int dvt_rv32_job_shard_chip_shape(const dvt_job *job, size_t shard, uint32_t chip, uint32_t *main_w, uint32_t *log_n) {
    size_t m = 0;
    const ShardJob *s = job ? const_cast<dvt_job *>(job)->at(shard, &m) : nullptr;
    if (!s || chip >= (uint32_t)rv32::N_CHIPS || !s->present[chip] || !main_w || !log_n) return DVT_ERR_INPUT;
    *main_w = (uint32_t)machine_rv32()->chips[chip].main_w;
    *log_n = s->log_n[chip];
    return DVT_OK;
}

// The forgery hunt (hunt.cuh) of one chip table of a shard, on lane 0 of the member that holds it.
int dvt_rv32_hunt_shard(dvt_prover *p, const dvt_pk *pk, dvt_job *job, size_t shard, uint32_t chip, uint64_t seed, const uint32_t *deltas,
                        uint32_t n_deltas, uint32_t pairs, const uint32_t *cols, uint32_t n_cols, uint32_t adjacent, uint32_t row_first,
                        uint32_t row_count, uint64_t max_evals, uint32_t *free_counts, uint8_t *free_map, dvt_escape *out, size_t cap,
                        uint64_t *n_reported, uint64_t *n_tried) {
    if (!p || !pk || !job) return fail(p, DVT_ERR_INPUT, "null argument");
    if (int rc = rv32_key(p, pk)) return rc;
    if (pairs > 1) return fail(p, DVT_ERR_INPUT, "pairs %u", pairs);
    if (int rc = same_members(p, pk, job)) return rc;
    const MachineDesc *m = machine_rv32();
    if (chip >= (uint32_t)m->n_chips) return fail(p, DVT_ERR_INPUT, "chip %u out of range (%d chips)", chip, m->n_chips);
    size_t mi = 0;
    ShardJob *s = job->at(shard, &mi);
    if (!s) return fail(p, DVT_ERR_INPUT, "shard %zu is not held by this job", shard);
    if (!s->present[chip]) return fail(p, DVT_ERR_INPUT, "shard %zu has no table of chip %s", shard, m->chips[chip].name);
    HuntRequest rq = hunt_request(seed, deltas, n_deltas, row_first, row_count, max_evals);
    if (pairs) hunt_want_pairs(&rq, cols, n_cols, adjacent, out, cap, n_reported, n_tried);
    else hunt_want_cells(&rq, free_counts, free_map);
    HuntPlan plan;
    if (int rc = hunt_plan(p->err, m->chips[chip], s->log_n[chip], rq, &plan)) return rc;
    Guard g(p); if (g.rc) return g.rc;
    if (int rc = turn_to(p, mi)) return rc;
    const Lane c = lane0(p, mi);
    ShardView v;
    if (int rc = shard_view(c, member_key(pk, mi), job, *s, shard, &v)) return rc;
    const CheckTable *t = v.table(chip);
    if (!t) return fail(p, DVT_ERR_INPUT, "shard %zu has no table of chip %s", shard, m->chips[chip].name);
    return hunt_table(c, m, *t, v.pub_mont, rq, plan);
}

// The join hunt (hunt_join.cuh) over windows of the job's tables, on lane 0 of the one member that holds their shards.
// Shard after shard: the next shard's K0 may write the working buffers the launches of the last one read, and every
// join_add synchronises.
int dvt_rv32_hunt_join_job(dvt_prover *p, const dvt_pk *pk, dvt_job *job, const dvt_join_window *windows, size_t n_windows,
                           const uint32_t *supply_chips, uint32_t n_supply, uint64_t seed, const uint32_t *deltas, uint32_t n_deltas,
                           const uint32_t *cols, const uint32_t *cols_count, uint64_t max_evals, size_t cap_records, size_t cap_absorbed,
                           uint32_t log_slots, dvt_join_summary *summary, dvt_join_cell *cells, size_t cap_cells, size_t *n_cells,
                           dvt_join_cell *absorbed, size_t cap_absorbed_out, size_t *n_absorbed) {
    if (!p || !pk || !job) return fail(p, DVT_ERR_INPUT, "null argument");
    if (!windows || !n_windows || (n_supply && !supply_chips) || !summary || !n_cells || !n_absorbed || (cap_cells && !cells) ||
        (cap_absorbed_out && !absorbed) || (cols_count && !cols))
        return fail(p, DVT_ERR_INPUT, "null argument");
    if (int rc = rv32_key(p, pk)) return rc;
    if (int rc = same_members(p, pk, job)) return rc;
    if (int rc = join_check_new(p->err, n_deltas, deltas, cap_records, cap_absorbed, log_slots)) return rc;
    const MachineDesc *m = machine_rv32();
    size_t mi = 0;
    std::vector<uint32_t> order;   // the shards in the order of their first window
    for (size_t w = 0; w < n_windows; w++) {
        size_t at = 0;
        ShardJob *s = job->at(windows[w].shard, &at);
        if (!s) return fail(p, DVT_ERR_INPUT, "shard %u is not held by this job", windows[w].shard);
        if (windows[w].chip >= (uint32_t)m->n_chips) return fail(p, DVT_ERR_INPUT, "chip %u out of range (%d chips)", windows[w].chip, m->n_chips);
        if (!s->present[windows[w].chip]) return fail(p, DVT_ERR_INPUT, "shard %u has no table of chip %s", windows[w].shard, m->chips[windows[w].chip].name);
        if (w && at != mi)
            return fail(p, DVT_ERR_UNSUPPORTED, "windows on shards of members %zu and %zu: a join runs on one device", mi, at);
        mi = at;
        if (std::find(order.begin(), order.end(), windows[w].shard) == order.end()) order.push_back(windows[w].shard);
    }
    for (uint32_t k = 0; k < n_supply; k++)
        if (supply_chips[k] >= (uint32_t)m->n_chips) return fail(p, DVT_ERR_INPUT, "supply chip %u out of range", supply_chips[k]);
    Guard g(p); if (g.rc) return g.rc;
    if (int rc = turn_to(p, mi)) return rc;
    const Lane c = lane0(p, mi);
    struct Held {   // the join's buffers go back however the call ends
        JoinDev dev;
        hipStream_t st;
        ~Held() { (void)hipStreamSynchronize(st); join_release(&dev); }
    } held{{}, c.eng.stream};
    JoinDev &j = held.dev;
    if (int rc = join_init(c, &j, m, seed, deltas, n_deltas, cap_records, cap_absorbed, log_slots)) return rc;
    for (size_t o = 0; o < order.size(); o++) {
        ShardView v;
        if (int rc = shard_view(c, member_key(pk, mi), job, *job->parts[mi].at(order[o]), order[o], &v)) return rc;
        auto table_of = [&](uint32_t chip) {   // (nullptr: p->err says which)
            const CheckTable *t = v.table(chip);
            if (!t) fail(p, DVT_ERR_INPUT, "shard %u has no table of chip %s", order[o], m->chips[chip].name);
            return t;
        };
        for (uint32_t k = 0; o == 0 && k < n_supply; k++) {
            const CheckTable *t = table_of(supply_chips[k]);
            if (!t) return DVT_ERR_INPUT;
            if (int rc = join_supply(p->err, j, *t, v.pub_mont)) return rc;
        }
        size_t col_at = 0;
        for (size_t w = 0; w < n_windows; w++) {
            const uint32_t nc = cols_count ? cols_count[w] : 0;
            const uint32_t *cl = nc ? cols + col_at : nullptr;
            col_at += nc;
            if (windows[w].shard != order[o]) continue;
            const CheckTable *t = table_of(windows[w].chip);
            if (!t) return DVT_ERR_INPUT;
            const uint64_t n = (uint64_t)1 << t->log_n;
            const uint32_t first = windows[w].row_first;
            const uint32_t count = windows[w].row_count ? windows[w].row_count : (uint32_t)(first < n ? n - first : 0);
            std::vector<uint32_t> use;
            if (int rc = join_check_add(p->err, j, order[o], windows[w].chip, *t->d, t->log_n, first, count, cl, nc, max_evals, &use)) return rc;
            if (int rc = join_add(c, j, order[o], windows[w].chip, *t, v.pub_mont, first, count, use)) return rc;
        }
        HIP_TRY(p, hipStreamSynchronize(c.eng.stream));
    }
    if (int rc = join_match(c, j)) return rc;
    std::copy_n(j.cells.begin(), std::min(cap_cells, j.cells.size()), cells);
    std::copy_n(j.absorbed.begin(), std::min(cap_absorbed_out, j.absorbed.size()), absorbed);
    *n_cells = j.cells.size();
    *n_absorbed = j.absorbed.size();
    *summary = j.summary;
    return DVT_OK;
}

}  // extern "C"
