// The inspectors of trace rows of the C ABI (include/dvt_prover.h): row checks, bus ledger, forgery hunt, join hunt.  Each has
// stage entry points (dvt_stage_*) on a table the caller uploaded (stage_table) and job entry points (dvt_rv32_*) on the
// tables of a prepared job's held shards (shard_view).  (What reads a job's cycle records instead: capi_report.hip.)
#include <algorithm>

#include "capi_job.h"
#include "ledger_key.h"
#include "sha256.h"

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
    if (int rc = for_members(p, [&](size_t m, const Lane &c) {
            JobPart &part = j->parts[m];
            int rc = DVT_OK;
            for (size_t k = 0; k < part.shards.size() && !rc; k++)
                rc = shard_check(c, member_key(pk, m), j, part.shards[k], part.first + k * part.stride, ch, &all, bus);
            return rc;
        }))
        return rc;
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
    if (int rc = for_members(p, [&](size_t m, const Lane &c) {
            JobPart &part = j->parts[m];
            for (size_t k = 0; k < part.shards.size(); k++)
                if (int rc = shard_ledger(c, member_key(pk, m), j, part.shards[k], part.first + k * part.stride, ledgers[m], mode)) return rc;
            return DVT_OK;
        }))
        return rc;
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
    if (int rc = for_members(p, [&](size_t m, const Lane &c) { return ledger_init(c, &ledgers[m], LOG_BUCKETS, CAP_SLOTS, seed); })) return rc;
    if (int rc = job_ledger_pass(p, pk, j, ledgers, 0)) return rc;
    uint32_t n_dirty = 0;
    if (ledgers.size() == 1) {
        if (int rc = ledger_close(lane0(p), ledgers[0], &n_dirty)) return rc;
    } else {   // the members' tallies added mod p on the host; the one bitmap back to every member
        std::vector<uint64_t> sum, one;
        if (int rc = for_members(p, [&](size_t m, const Lane &c) {
                const int rc = ledger_tallies(c, ledgers[m], m ? &one : &sum);
                for (size_t i = 0; !rc && m && i < sum.size(); i++) sum[i] = (sum[i] + one[i]) % P;
                return rc;
            }))
            return rc;
        std::vector<uint32_t> bitmap;
        n_dirty = ledger_dirty_of(sum, &bitmap);
        if (n_dirty)
            if (int rc = for_members(p, [&](size_t m, const Lane &c) { return ledger_set_dirty(c, ledgers[m], bitmap); })) return rc;
    }
    all->clear();
    *overflow = false;
    if (!n_dirty) return DVT_OK;
    if (int rc = job_ledger_pass(p, pk, j, ledgers, 1)) return rc;
    if (int rc = for_members(p, [&](size_t m, const Lane &c) { return ledger_records(c, ledgers[m], all, overflow); })) return rc;
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

extern "C" {

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
