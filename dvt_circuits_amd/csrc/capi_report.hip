// The record reports of the C ABI (include/dvt_prover.h): what reads the cycle records a prepared job holds in HBM instead of its
// trace rows.  The execution report (profile.h), the call-tree report (calltree.h) and the memory report (memreport.h) count
// over them; the watchpoint search (watch.h) returns the ones that match; the snapshot (snapshot.h) reduces them to the state of
// the machine at one position; the origin search (origin.h) follows one value back through them and the uses search (uses.h)
// forward; the divergence report (diverge.h) holds the records of two jobs side by side.  Each has a job entry point
// (dvt_rv32_job_*), which runs on lane 0 of every member that holds shards, and a host-only one (dvt_execute_*) with the same
// rule over the executor's records (execute_traced).
#include <algorithm>
#include <type_traits>

#include "calltree.h"
#include "capi_job.h"
#include "diverge.h"
#include "memreport.h"
#include "origin.h"
#include "profile.h"
#include "snapshot.h"
#include "uses.h"
#include "watch.h"

using namespace dvt;

// ------------------------------------------------------------------ what the reports share
namespace {
// One M(pool of lane 0) per member of the handle.  The members' buffers go back to their pools under their own device's turn,
// member 0's device is current afterwards: declared first in a function, that holds however the call ends.
template <class M>
struct MemberRun {
    dvt_prover *p;
    std::vector<std::unique_ptr<M>> mem;
    explicit MemberRun(dvt_prover *p) : p(p) {
        for (size_t m = 0; m < n_members(p); m++) mem.emplace_back(new M(member(p, m).eng.pool));
    }
    ~MemberRun() {
        for (size_t m = 0; m < mem.size(); m++) {
            (void)turn_to(p, m);
            mem[m].reset();
        }
        (void)turn_to(p, 0);
    }
    M &operator[](size_t m) { return *mem[m]; }
};

// A pair of events on a stream, made at first use, destroyed with the span (under the device's turn: the span belongs to a
// member of a MemberRun).  ms(), once the stream was synchronised: the time between them, 0 when the pair was never closed.
// begin_at_end_of(prev): the span begins where prev, which outlives it, ended; no event of its own is recorded for that.
struct EventSpan {
    hipEvent_t ev[2] = {};
    bool closed = false, borrowed = false;
    EventSpan() = default;
    EventSpan(const EventSpan &) = delete;
    ~EventSpan() {
        for (int i = borrowed; i < 2; i++)
            if (ev[i]) (void)hipEventDestroy(ev[i]);
    }
    void begin_at_end_of(const EventSpan &prev) { ev[0] = prev.ev[1]; borrowed = true; }
    hipError_t mark(int i, hipStream_t s) {
        if (!ev[i])
            if (hipError_t e = hipEventCreate(&ev[i])) return e;
        return hipEventRecord(ev[i], s);
    }
    hipError_t begin(hipStream_t s) { return mark(0, s); }
    hipError_t end(hipStream_t s) {
        const hipError_t e = mark(1, s);
        closed = e == hipSuccess;
        return e;
    }
    double ms() const {
        float t = 0;
        return closed && hipEventElapsedTime(&t, ev[0], ev[1]) == hipSuccess ? t : 0;
    }
};

// the shards a job holds, in execution order, whichever member holds them: shard k of member m is at position pos
struct Held {
    size_t pos, m, k;
    ShardJob *s;
};
std::vector<Held> held_in_order(dvt_job *j) {
    std::vector<Held> out;
    for (size_t pos = 0; pos < j->n_total; pos++) {
        size_t m = 0;
        if (ShardJob *s = j->at(pos, &m)) out.push_back({pos, m, (size_t)(s - j->parts[m].shards.data()), s});
    }
    return out;
}

// the refusal of a report that follows `what` from the first record on: held_in_order(j)[pos] is then the shard at pos
int whole_execution(dvt_prover *p, dvt_job *j, const char *what) {
    if (j->first != 0 || j->stride != 1 || j->held() != j->n_total)
        return fail(p, DVT_ERR_UNSUPPORTED, "the job holds %zu of the %zu shards of its execution (first %zu, stride %zu): the %s across a gap is unknown",
                    j->held(), j->n_total, j->first, j->stride, what);
    size_t m = 0;
    for (size_t pos = 0; pos < j->n_total; pos++)
        if (!j->at(pos, &m)) return fail(p, DVT_ERR_UNSUPPORTED, "the job does not hold shard %zu", pos);
    return DVT_OK;
}

// the slot table of a report that was given no size: four slots per instruction, within the bounds
uint32_t default_log_slots(size_t n_instr) {
    uint32_t log_slots = prof::DEFAULT_MIN_LOG_SLOTS;
    while (log_slots < prof::MAX_LOG_SLOTS && ((size_t)1 << log_slots) < 4 * n_instr) log_slots++;
    return log_slots;
}

// records the executor never writes (after their count, on the device paths), and a tally with too many syscall ids
constexpr const char *BAD_INSTR = "cycle records name an instruction outside the text";
constexpr const char *BAD_RECORD = "cycle records name an instruction outside the text or an address outside guest memory";
std::string sys_overflow() { return "more than " + std::to_string(prof::MAX_SYSCALLS) + " distinct syscall ids"; }

// The shards of a whole execution (whole_execution() passed) in order, and the position P = (shard, row) among them: the number
// of records before it, as the summaries report it.
struct Placed {
    std::vector<Held> held;
    std::vector<uint64_t> shard_n;
    uint64_t cycles = 0, position = 0;
    int init(dvt_prover *p, dvt_job *j, uint32_t shard, uint32_t row) {
        held = held_in_order(j);
        shard_n.resize(held.size());
        for (const Held &h : held) {
            const ShardJob &s = *h.s;
            if (s.n_recs > 0xffffffffull) return fail(p, DVT_ERR_INPUT, "shard %zu has %zu records", h.pos, s.n_recs);
            shard_n[h.pos] = s.n_recs;
            cycles += s.n_recs;
            position += s.index < shard ? s.n_recs : s.index == shard ? std::min<uint64_t>(s.n_recs, row) : 0;
        }
        return DVT_OK;
    }
    // the shard that holds the record at position `where`, or nullptr
    const Held *holder(unsigned long long where) const {
        const uint32_t sh = (uint32_t)(where >> 32), rw = (uint32_t)where;
        return sh && sh <= held.size() && rw < held[sh - 1].s->n_recs ? &held[sh - 1] : nullptr;
    }
    // position, cycles, shard, row and shards_total of a summary
    template <class Summary>
    void place(Summary *s) const {
        s->position = position; s->cycles = cycles;
        snap::locate(shard_n, position, &s->shard, &s->row);
        s->shards_total = (uint32_t)held.size();
    }
};

// One allocation cut into typed arrays.  A layout is a function that take()s its arrays in order: run over Carve{} it returns the
// bytes to allocate (at), run over Carve{base} it hands out the pointers.
struct Carve {
    char *base = nullptr;
    size_t at = 0;
    template <class T>
    T *take(size_t count, size_t align = alignof(T)) {
        at = (at + align - 1) / align * align;
        T *out = base ? reinterpret_cast<T *>(base + at) : nullptr;
        at += count * sizeof(T);
        return out;
    }
};

// ---- what the origin search and the uses search share: both ask a level of sorted questions in chunks of one device pass, and
// both read the records their answers name from the member that holds each one's shard.
constexpr size_t PASS_Q = origin::PASS_Q;

// The questions of a level in the order a pass takes them (origin::sorts_before), cut into chunks of at most PASS_Q.
struct Chunks {
    const std::vector<origin::Question> &qs;
    std::vector<uint32_t> order;                // order[i]: the question at place i of the sorted level
    std::vector<uint32_t> target;               // [PASS_Q], of the chunk cut last
    std::vector<unsigned long long> pos;        // [PASS_Q], of the chunk cut last
    explicit Chunks(const std::vector<origin::Question> &qs) : qs(qs), order(qs.size()), target(PASS_Q), pos(PASS_Q) {
        for (size_t i = 0; i < order.size(); i++) order[i] = (uint32_t)i;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return origin::sorts_before(qs[x], qs[y]); });
    }
    // the chunk that begins at place `at`: target[], pos[], a->reg_off and a->n; returns n
    size_t cut(size_t at, PassArgs *a) {
        const size_t n = std::min(PASS_Q, order.size() - at);
        uint32_t n_regs = 0;
        for (size_t i = 0; i < n; i++) {
            const origin::Question &q = qs[order[at + i]];
            target[i] = q.target; pos[i] = q.Q;
            if (q.what == DVT_ORIGIN_REG) n_regs++;
        }
        for (uint32_t k = 0; k <= 32; k++) {   // the first register question with a register >= k (they are sorted)
            uint32_t f = 0;
            while (f < n_regs && target[f] < k) f++;
            a->reg_off[k] = f;
        }
        a->n = (uint32_t)n;
        return n;
    }
};

// What a member of either search holds for the gather (origin.hip's): the fetches of a level and the records they brought.
struct GatherMember {
    OriginFetch *d_fetch = nullptr;     // [MAX_EDGES]
    rv32::CycleRec *d_recs = nullptr;   // [MAX_EDGES]
    std::vector<OriginFetch> fetch;
    std::vector<rv32::CycleRec> got;
    EventSpan t_gather;
};
static_assert(origin::MAX_EDGES == uses::MAX_EDGES, "the gather buffers of both searches");

// The records at the positions `want` (repeats are fetched once), each from the member that holds its shard: (*out)[position].
// buffers(c, member) makes the member's device arrays; nowhere / too_many: the search's words for a position that lies in no
// shard and for more fetches than its edges.  *ms grows by the gather's time.
template <class Run, class Buffers>
int gather_records(dvt_prover *p, const Placed &pl, Run &run, const std::vector<unsigned long long> &want, Buffers buffers, const char *nowhere,
                   const char *too_many, double *ms, std::map<unsigned long long, rv32::CycleRec> *out) {
    std::map<unsigned long long, std::pair<size_t, size_t>> where;   // position -> (member, index among its fetches)
    for (size_t m = 0; m < n_members(p); m++) run[m].fetch.clear();
    for (const unsigned long long pos : want) {
        if (where.count(pos)) continue;
        const Held *h = pl.holder(pos);
        if (!h) return fail(p, DVT_ERR_DEVICE, "%s", nowhere);
        where[pos] = {h->m, run[h->m].fetch.size()};
        run[h->m].fetch.push_back(OriginFetch{h->s->d_recs, (uint32_t)h->s->n_recs, (uint32_t)pos});
    }
    if (int rc = for_members(p, [&](size_t m, const Lane &c) {
            Engine &e = c.eng;
            auto &gm = run[m];
            if (gm.fetch.empty()) return DVT_OK;
            if (gm.fetch.size() > origin::MAX_EDGES) return fail(c.err, DVT_ERR_DEVICE, "%s", too_many);
            if (int rc = buffers(c, gm)) return rc;
            HIP_TRY(c.err, hipMemcpyAsync(gm.d_fetch, gm.fetch.data(), gm.fetch.size() * sizeof(OriginFetch), hipMemcpyHostToDevice, e.stream));
            HIP_TRY(c.err, gm.t_gather.begin(e.stream));
            HIP_TRY(c.err, launch_origin_gather(e.stream, gm.d_fetch, (uint32_t)gm.fetch.size(), gm.d_recs));
            HIP_TRY(c.err, gm.t_gather.end(e.stream));
            gm.got.resize(gm.fetch.size());
            if (!e.download(gm.got.data(), gm.d_recs, gm.got.size() * sizeof(rv32::CycleRec))) return engine_fail(c.err, e);
            *ms += gm.t_gather.ms();
            return DVT_OK;
        }))
        return rc;
    out->clear();
    for (const auto &w : where) (*out)[w.first] = run[w.second.first].got[w.second.second];
    return DVT_OK;
}

// How either search over a job ends.  rc: of Search::run; rc_answer: why an answer failed; ms[n_ms]: the device times, copied to
// out_ms with the rest of the call's time, which is the host's, behind them.
template <class Search, class Summary>
int finish_search(dvt_prover *p, int rc, int rc_answer, uint64_t bad, const Search &search, uint32_t passes, const Placed &pl, Clock::time_point t0,
                  const double *ms, int n_ms, double *out_ms, Summary *summary) {
    if (rc == 1) return rc_answer;
    if (bad) return fail(p, DVT_ERR_INPUT, "%llu %s", (unsigned long long)bad, BAD_RECORD);
    if (rc) return fail(p, DVT_ERR_DEVICE, "%s", search.why.c_str());
    Summary s = search.s;
    s.passes = passes;
    pl.place(&s);
    const double total = ms_since(t0);
    s.ms = (float)total;
    double rest = total;
    for (int i = 0; i < n_ms; i++) { out_ms[i] = ms[i]; rest -= ms[i]; }
    out_ms[n_ms] = std::max(0.0, rest);
    *summary = s;
    return DVT_OK;
}
}  // namespace

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
    if (counters[PROFILE_BAD_RECORDS]) return fail(c.err, DVT_ERR_INPUT, "%llu %s", counters[PROFILE_BAD_RECORDS], BAD_INSTR);
    if (counters[PROFILE_SYS_OVERFLOW]) return fail(c.err, DVT_ERR_UNSUPPORTED, "%s", sys_overflow().c_str());
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
    const uint32_t log_slots = log_edge_slots ? log_edge_slots : default_log_slots(classes.size());
    prof::Tally t(pk->prog);
    if (int rc = for_members(p, [&](size_t m, const Lane &c) { return member_profile(c, pk, j->parts[m], log_slots, classes, &t); })) return rc;
    if (!prof::emit(pk->prog, t, (uint32_t)j->n_total, ms_since(t0), out)) return fail(p, DVT_ERR_UNSUPPORTED, "%s", sys_overflow().c_str());
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
    EventSpan t_summaries, t_calls;                   // of a timed run: the summaries, the unmatched calls
    explicit CalltreeMember(DevPool &pool) : base{pool}, calls{pool}, frames{pool} {}
};
using CalltreeRun = MemberRun<CalltreeMember>;
}  // namespace

// Summary mode over a prefix of every held shard, for the call tree (all records) and the snapshot's backtrace (the records
// before its position): prefix(shard, &n, &succ) names the first n records the pass takes and the successor of the last of
// them.  {u, c} of every span; then summary mode again, writing the unmatched calls of the shards that have any at the offsets
// the host made of the c's.  S = 2^log_slots arc slots are laid out for emit mode (log_slots 0: none).  timed: stream events
// around both runs.
template <class Prefix>
static int calltree_summaries(dvt_prover *p, dvt_job *j, const std::vector<uint32_t> &classes, uint32_t log_slots, bool timed, Prefix prefix, CalltreeRun &run) {
    const size_t n = classes.size(), S = log_slots ? (size_t)1 << log_slots : 0;
    // ---- summary mode: {u, c} of every span
    if (int rc = for_members(p, [&](size_t m, const Lane &c) {
            Engine &e = c.eng;
            CalltreeMember &cm = run[m];
            for (auto &s : j->parts[m].shards) {
                size_t take = 0;
                uint32_t succ = prof::NO_SUCC;
                prefix(s, &take, &succ);
                cm.n_of.push_back(std::min(take, s.n_recs));
                cm.succ_of.push_back(succ);
                cm.span0.push_back(cm.spans);
                cm.spans += (cm.n_of.back() + CALLTREE_SPAN - 1) / CALLTREE_SPAN;
            }
            if (!cm.spans) return DVT_OK;
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
            if (timed) HIP_TRY(c.err, cm.t_summaries.begin(e.stream));
            for (size_t k = 0; k < cm.span0.size(); k++)
                HIP_TRY(c.err, launch_calltree_summary(e.stream, j->parts[m].shards[k].d_recs, cm.n_of[k], cm.succ_of[k], cm.span0[k], tb));
            if (timed) HIP_TRY(c.err, cm.t_summaries.end(e.stream));
            cm.summaries.resize(cm.spans);
            if (!e.download(cm.summaries.data(), tb.summaries, cm.spans * sizeof(CalltreeSpanSummary))) return engine_fail(c.err, e);
            cm.calls_at.resize(cm.spans);
            for (size_t i = 0; i < cm.spans; i++) {
                if (cm.summaries[i].u > CALLTREE_SPAN || cm.summaries[i].c > CALLTREE_SPAN) return fail(p, DVT_ERR_DEVICE, "span summary out of range");
                cm.calls_at[i] = cm.total_calls;
                cm.total_calls += cm.summaries[i].c;
            }
            return DVT_OK;
        }))
        return rc;
    // ---- summary mode again: the unmatched calls of the shards that have any, at those offsets
    return for_members(p, [&](size_t m, const Lane &c) {
        Engine &e = c.eng;
        CalltreeMember &cm = run[m];
        if (!cm.total_calls) return DVT_OK;
        HIP_TRY(c.err, e.pool.alloc_bytes(&cm.calls.ptr, cm.total_calls * sizeof(CalltreeCall)));
        CalltreeTables tb = cm.tb;
        tb.calls_at = cm.d_calls_at;
        tb.calls = static_cast<CalltreeCall *>(cm.calls.ptr);
        HIP_TRY(c.err, hipMemcpyAsync(cm.d_calls_at, cm.calls_at.data(), cm.spans * 8, hipMemcpyHostToDevice, e.stream));
        if (timed) HIP_TRY(c.err, cm.t_calls.begin(e.stream));
        for (size_t k = 0; k < cm.span0.size(); k++) {
            const size_t end = k + 1 < cm.span0.size() ? cm.span0[k + 1] : cm.spans;
            size_t n_calls = 0;
            for (size_t i = cm.span0[k]; i < end; i++) n_calls += cm.summaries[i].c;
            if (n_calls) HIP_TRY(c.err, launch_calltree_summary(e.stream, j->parts[m].shards[k].d_recs, cm.n_of[k], cm.succ_of[k], cm.span0[k], tb));
        }
        if (timed) HIP_TRY(c.err, cm.t_calls.end(e.stream));
        cm.h_calls.resize(cm.total_calls);
        if (!e.download(cm.h_calls.data(), tb.calls, cm.total_calls * sizeof(CalltreeCall))) return engine_fail(c.err, e);
        return DVT_OK;
    });
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
    if (int rc = whole_execution(p, j, "call stack")) return rc;
    const auto t0 = Clock::now();
    calltree::State st(pk->prog);
    const uint32_t log_slots = log_arc_slots ? log_arc_slots : default_log_slots(st.classes.size());
    const size_t S = (size_t)1 << log_slots;
    const uint32_t entry = prof::index_of_pc(pk->prog, pk->prog.entry);
    if (entry == prof::NO_SUCC) return fail(p, DVT_ERR_INPUT, "the entry 0x%08x is no instruction of the text", pk->prog.entry);
    auto succ_of = [&](const ShardJob &s) { return prof::index_of_pc(pk->prog, s.next_pc); };
    CalltreeRun run(p);
    if (int rc = calltree_summaries(p, j, st.classes, log_slots, false, [&](const ShardJob &s, size_t *take, uint32_t *succ) { *take = s.n_recs; *succ = succ_of(s); }, run))
        return rc;
    const double ms_summary = ms_since(t0);

    // ---- the merge: the spans in execution order, over all shards in job order, whichever member holds them
    const auto t1 = Clock::now();
    std::vector<uint64_t> base_of(j->n_total);   // global position of the shard's first record
    uint64_t cycles = 0;
    st.stack.push_back(calltree::Frame{entry, 0});
    for (const Held &h : held_in_order(j)) {
        CalltreeMember &cm = run[h.m];
        base_of[h.pos] = cycles;
        const size_t n_spans = (h.s->n_recs + CALLTREE_SPAN - 1) / CALLTREE_SPAN;
        if (cm.span_in.empty()) cm.span_in.resize(cm.spans);
        for (size_t i = 0; i < n_spans; i++) {
            const size_t span = cm.span0[h.k] + i;
            const CalltreeSpanSummary sum = cm.summaries[span];
            const size_t depth = st.stack.size(), n_in = std::min<size_t>((size_t)sum.u + 1, depth);
            cm.span_in[span] = CalltreeSpanIn{cm.h_frames.size(), (uint32_t)n_in, (uint32_t)std::min<size_t>(depth, 0xffffffffu)};
            for (size_t f = 0; f < n_in; f++) cm.h_frames.push_back(CalltreeFrame{st.stack[depth - 1 - f].open, st.stack[depth - 1 - f].fn, 0});
            (void)calltree_merge_span(st.stack, sum, cm.h_calls.data() + cm.calls_at[span], cycles + i * CALLTREE_SPAN);
        }
        cycles += h.s->n_recs;
    }
    const double ms_merge = ms_since(t1);

    // ---- emit mode
    const auto t2 = Clock::now();
    unsigned long long bad = 0;
    if (int rc = for_members(p, [&](size_t m, const Lane &c) {
            Engine &e = c.eng;
            CalltreeMember &cm = run[m];
            if (!cm.spans) return DVT_OK;
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
            return DVT_OK;
        }))
        return rc;
    if (bad) return fail(p, DVT_ERR_INPUT, "%llu %s", bad, BAD_INSTR);
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
// ORed into *t.  The buffers go back to the pool at scope exit.  table: memrep::device_table, n_pre shapes at its end.
static int member_memory(const Lane &c, JobPart &part, const std::vector<uint32_t> &table, size_t n, uint32_t n_pre, memrep::Tally *t) {
    if (part.shards.empty()) return DVT_OK;
    Engine &e = c.eng;
    // 64-bit words: first_touch, counters, the page arrays; then sp[2], the dense count and a pad; then the table
    const size_t zero_words = n + MEMORY_COUNTERS + (size_t)MEMORY_PAGE_ARRAYS * memrep::N_PAGES;
    size_t n_recs = 0;
    for (auto &s : part.shards) n_recs += s.n_recs;
    const uint32_t cap = (uint32_t)std::min<size_t>(memrep::N_PAGES, 4 * n_recs);   // (a record touches at most four pages)
    StageBuf buf{e.pool}, bitmap{e.pool}, dense{e.pool};
    HIP_TRY(c.err, e.pool.alloc_bytes(&buf.ptr, zero_words * 8 + 16 + table.size() * 4));
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
    HIP_TRY(c.err, hipMemcpyAsync(d32 + 4, table.data(), table.size() * 4, hipMemcpyHostToDevice, e.stream));
    for (auto &s : part.shards) HIP_TRY(c.err, launch_memory_records(e.stream, s.d_recs, s.n_recs, tb));
    HIP_TRY(c.err, launch_memory_gather(e.stream, tb, static_cast<MemoryDensePage *>(dense.ptr), cap, d32 + 2));
    std::vector<unsigned long long> h(n + MEMORY_COUNTERS + 2);   // first_touch, counters | sp, the dense count, the pad
    if (!e.download(h.data(), d, (n + MEMORY_COUNTERS) * 8) || !e.download(h.data() + n + MEMORY_COUNTERS, d32, 16)) return engine_fail(c.err, e);
    const unsigned long long *counters = h.data() + n;
    uint32_t tail[4];
    memcpy(tail, h.data() + n + MEMORY_COUNTERS, sizeof tail);
    if (counters[MEMORY_BAD_RECORDS]) return fail(c.err, DVT_ERR_INPUT, "%llu %s", counters[MEMORY_BAD_RECORDS], BAD_RECORD);
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
    const std::vector<uint32_t> table = memrep::device_table(pk->prog, shapes);
    memrep::Tally t(pk->prog);
    if (int rc = for_members(p, [&](size_t m, const Lane &c) { return member_memory(c, j->parts[m], table, n, (uint32_t)shapes.size(), &t); })) return rc;
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
    StageBuf base, hits;                  // hits: from the member's first emit launch on
    std::vector<size_t> span0;            // of the member's k-th shard
    size_t spans = 0;
    uint32_t *d_counts = nullptr, *d_offs = nullptr, *d_totals = nullptr;
    const uint32_t *d_statics = nullptr;
    std::vector<uint32_t> totals;         // [shard k][query]
    std::vector<dvt_watch_hit> h_hits;
    EventSpan t_count, t_scan, t_emit;
    explicit WatchMember(DevPool &pool) : base{pool}, hits{pool} {}
};
}  // namespace

static int job_watch(dvt_prover *p, const dvt_pk *pk, dvt_job *j, const dvt_watch_query *queries, size_t nq, uint32_t K, dvt_watch_hit *hits,
                     uint64_t *totals, dvt_watch_summary *summary) {
    if (int rc = same_members(p, pk, j)) return rc;
    const auto t0 = Clock::now();
    const watch::Statics statics(pk->prog);
    const size_t n = statics.n();
    WatchArgs args{};
    std::copy_n(queries, nq, args.q);
    args.sh = watch::shapes();
    args.n_instr = (uint32_t)n; args.text_base = pk->prog.text_base; args.n_queries = (uint32_t)nq;
    MemberRun<WatchMember> run(p);
    uint64_t cycles = 0;
    unsigned long long bad = 0;

    // ---- count and scan
    if (int rc = for_members(p, [&](size_t m, const Lane &c) {
            Engine &e = c.eng;
            WatchMember &wm = run[m];
            JobPart &part = j->parts[m];
            for (auto &s : part.shards) {
                wm.span0.push_back(wm.spans);
                wm.spans += (s.n_recs + watch::SPAN - 1) / watch::SPAN;
                cycles += s.n_recs;
            }
            if (part.shards.empty()) return DVT_OK;
            // the bad-record counter (64 bits), then u32: span counts, span offsets, shard totals, the static words
            const size_t span_words = std::max<size_t>(wm.spans, 1) * nq, total_words = part.shards.size() * nq;
            HIP_TRY(c.err, e.pool.alloc_bytes(&wm.base.ptr, 8 + (2 * span_words + total_words) * 4 + statics.bytes()));
            unsigned long long *d_bad = static_cast<unsigned long long *>(wm.base.ptr);
            wm.d_counts = reinterpret_cast<uint32_t *>(d_bad + 1);
            wm.d_offs = wm.d_counts + span_words;
            wm.d_totals = wm.d_offs + span_words;
            uint32_t *d_stat = wm.d_totals + total_words;
            wm.d_statics = d_stat;
            args.statics = d_stat; args.offs = d_stat + n;
            HIP_TRY(c.err, hipMemsetAsync(wm.base.ptr, 0, 8 + (2 * span_words + total_words) * 4, e.stream));
            HIP_TRY(c.err, hipMemcpyAsync(d_stat, statics.words.data(), statics.bytes(), hipMemcpyHostToDevice, e.stream));
            HIP_TRY(c.err, wm.t_count.begin(e.stream));
            for (size_t k = 0; k < part.shards.size(); k++) {
                const ShardJob &s = part.shards[k];
                args.shard = s.index;
                HIP_TRY(c.err, launch_watch_count(e.stream, s.d_recs, s.n_recs, args, wm.d_counts + wm.span0[k] * nq, d_bad));
            }
            HIP_TRY(c.err, wm.t_count.end(e.stream));
            wm.t_scan.begin_at_end_of(wm.t_count);
            for (size_t k = 0; k < part.shards.size(); k++) {
                const size_t n_spans = (part.shards[k].n_recs + watch::SPAN - 1) / watch::SPAN;
                HIP_TRY(c.err, launch_watch_scan(e.stream, wm.d_counts + wm.span0[k] * nq, wm.d_offs + wm.span0[k] * nq, (uint32_t)n_spans, (uint32_t)nq,
                                                 wm.d_totals + k * nq));
            }
            HIP_TRY(c.err, wm.t_scan.end(e.stream));
            wm.totals.resize(total_words);
            unsigned long long h_bad = 0;
            if (!e.download(wm.totals.data(), wm.d_totals, total_words * 4) || !e.download(&h_bad, d_bad, 8)) return engine_fail(c.err, e);
            bad += h_bad;
            return DVT_OK;
        }))
        return rc;
    if (bad) return fail(p, DVT_ERR_INPUT, "%llu %s", bad, BAD_RECORD);

    // ---- the ranks: the held shards in execution order, whichever member holds them
    const std::vector<Held> held = held_in_order(j);
    std::vector<std::vector<unsigned long long>> base_of(held.size(), std::vector<unsigned long long>(nq, 0));
    WatchEmitArgs ea{};
    ea.cap_each = K;
    for (size_t h = 0; h < held.size(); h++)
        for (size_t q = 0; q < nq; q++) {
            base_of[h][q] = ea.total[q];
            ea.total[q] += run[held[h].m].totals[held[h].k * nq + q];
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
        WatchMember &wm = run[m];
        bool any = false;
        for (size_t q = 0; q < nq; q++) any = any || kept_in(q, base_of[h][q], base_of[h][q] + wm.totals[k * nq + q]);
        if (!any) continue;
        if (int rc = turn_to(p, m)) return rc;
        const Lane c = lane0(p, m);
        Engine &e = c.eng;
        if (!wm.hits.ptr) {
            HIP_TRY(c.err, e.pool.alloc_bytes(&wm.hits.ptr, 2 * nq * K * sizeof(dvt_watch_hit)));
            HIP_TRY(c.err, wm.t_emit.begin(e.stream));
        }
        const ShardJob &s = *held[h].s;
        args.statics = wm.d_statics; args.offs = wm.d_statics + n; args.shard = s.index;
        std::copy(base_of[h].begin(), base_of[h].end(), ea.base);
        HIP_TRY(c.err, launch_watch_emit(e.stream, s.d_recs, s.n_recs, args, ea, wm.d_counts + wm.span0[k] * nq, wm.d_offs + wm.span0[k] * nq, wm.hits.ptr));
        emit_shards++;
    }
    double ms[3] = {0, 0, 0};
    if (int rc = for_members(p, [&](size_t m, const Lane &c) {
            WatchMember &wm = run[m];
            if (wm.hits.ptr) {
                HIP_TRY(c.err, wm.t_emit.end(c.eng.stream));
                wm.h_hits.resize(2 * nq * K);
                if (!c.eng.download(wm.h_hits.data(), wm.hits.ptr, wm.h_hits.size() * sizeof(dvt_watch_hit))) return engine_fail(c.err, c.eng);
            }
            ms[0] += wm.t_count.ms(); ms[1] += wm.t_scan.ms(); ms[2] += wm.t_emit.ms();
            return DVT_OK;
        }))
        return rc;
    // every kept rank from the array of the member whose shard holds it
    for (size_t h = 0; K && h < held.size(); h++) {
        const WatchMember &wm = run[held[h].m];
        if (wm.h_hits.empty()) continue;
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
    EventSpan t_reduce, t_gather;
    explicit SnapMember(DevPool &pool) : base{pool}, items{pool}, sides{pool} {}
};
}  // namespace

static int job_snapshot(dvt_prover *p, const dvt_pk *pk, dvt_job *j, uint32_t shard, uint32_t row, const snap::Ranges &rg, dvt_snap_cell regs[32],
                        dvt_snap_cell *words, dvt_snap_frame *frames, size_t cap_frames, dvt_snap_summary *summary) {
    if (int rc = same_members(p, pk, j)) return rc;
    if (int rc = whole_execution(p, j, "state")) return rc;
    const auto t0 = Clock::now();
    const rv32::Program &prog = pk->prog;
    const size_t W = rg.n_words;
    const unsigned long long P = watch::position(shard, row);
    MemberRun<SnapMember> run(p);   // (declared first: however the call ends, member 0's device is current again)
    // ---- the shards in execution order: their sizes, the records before P, the record at P
    Placed pl;
    if (int rc = pl.init(p, j, shard, row)) return rc;
    const std::vector<Held> &held = pl.held;
    const std::vector<uint64_t> &shard_n = pl.shard_n;
    const uint64_t cycles = pl.cycles, position = pl.position;
    const watch::Statics statics(prog);
    const size_t n = statics.n();
    uint32_t at_shard = 1, at_row = 0, idx_at = prof::NO_SUCC, pc = held.empty() ? prog.entry : held.back().s->next_pc;
    snap::locate(shard_n, position, &at_shard, &at_row);
    if (position < cycles) {   // the record at P: its idx is the successor of the last record before P, and names the pc
        if (at_shard > held.size() || at_row >= held[at_shard - 1].s->n_recs) return fail(p, DVT_ERR_DEVICE, "position %llu lies in no shard", (unsigned long long)position);
        const Held &h = held[at_shard - 1];
        if (int rc = turn_to(p, h.m)) return rc;
        if (!member(p, h.m).eng.download(&idx_at, &h.s->d_recs[at_row].idx, 4)) return engine_fail(p->err, member(p, h.m).eng);
        if (idx_at >= n) return fail(p, DVT_ERR_INPUT, "the cycle record at shard %u, row %u names an instruction outside the text", at_shard, at_row);
        pc = prog.text_base + 4 * idx_at;
    }

    SnapArgs args{};
    args.rg = rg;
    args.sh = watch::shapes();
    args.n_instr = (uint32_t)n; args.text_base = prog.text_base; args.P = P;
    const size_t table_words = 1 + 32 + 2 * W;   // 64-bit: bad records, regs, before | after; then the static words

    // ---- reduce (launches only: the backtrace's downloads below wait while every member's reduce runs)
    if (int rc = for_members(p, [&](size_t m, const Lane &c) {
            Engine &e = c.eng;
            SnapMember &sm = run[m];
            JobPart &part = j->parts[m];
            if (part.shards.empty()) return DVT_OK;
            HIP_TRY(c.err, e.pool.alloc_bytes(&sm.base.ptr, table_words * 8 + statics.bytes()));
            sm.d_tables = static_cast<unsigned long long *>(sm.base.ptr);
            uint32_t *d_stat = reinterpret_cast<uint32_t *>(sm.d_tables + table_words);
            sm.d_statics = d_stat;
            const SnapTables tb{sm.d_tables + 33, sm.d_tables + 33 + W, sm.d_tables + 1, sm.d_tables};
            HIP_TRY(c.err, hipMemsetAsync(sm.d_tables, 0, (33 + W) * 8, e.stream));
            if (W) HIP_TRY(c.err, hipMemsetAsync(tb.after, 0xff, W * 8, e.stream));
            HIP_TRY(c.err, hipMemcpyAsync(d_stat, statics.words.data(), statics.bytes(), hipMemcpyHostToDevice, e.stream));
            args.statics = d_stat; args.offs = d_stat + n;
            HIP_TRY(c.err, sm.t_reduce.begin(e.stream));
            for (auto &s : part.shards) {
                args.shard = s.index;
                HIP_TRY(c.err, launch_snapshot_reduce(e.stream, s.d_recs, s.n_recs, args, tb));
            }
            HIP_TRY(c.err, sm.t_reduce.end(e.stream));
            return DVT_OK;
        }))
        return rc;

    // ---- the backtrace: the call-tree pass in summary mode over the records before P, and the call tree's merge
    const uint32_t entry = prof::index_of_pc(prog, prog.entry);
    if (entry == prof::NO_SUCC) return fail(p, DVT_ERR_INPUT, "the entry 0x%08x is no instruction of the text", prog.entry);
    const std::vector<uint32_t> classes = calltree::instr_classes(prog);
    CalltreeRun ct(p);
    auto prefix = [&](const ShardJob &s, size_t *take, uint32_t *succ) {
        *take = s.index < shard ? s.n_recs : s.index == shard ? std::min<size_t>(s.n_recs, row) : 0;
        *succ = *take < s.n_recs ? idx_at : prof::index_of_pc(prog, s.next_pc);
    };
    if (int rc = calltree_summaries(p, j, classes, 0, true, prefix, ct)) return rc;
    std::vector<calltree::Frame> stack;
    uint64_t unmatched = 0, before_shard = 0;
    if (position) stack.push_back(calltree::Frame{entry, 0});
    for (size_t pos = 0; pos < held.size() && position; pos++) {
        const Held &h = held[pos];
        CalltreeMember &cm = ct[h.m];
        const size_t n_spans = (cm.n_of[h.k] + CALLTREE_SPAN - 1) / CALLTREE_SPAN;
        for (size_t i = 0; i < n_spans; i++) {
            const size_t span = cm.span0[h.k] + i;
            unmatched += calltree_merge_span(stack, cm.summaries[span], cm.h_calls.data() + cm.calls_at[span], before_shard + i * CALLTREE_SPAN);
        }
        before_shard += h.s->n_recs;
    }

    // ---- the members' winners, merged
    std::vector<unsigned long long> win(table_words, 0), one(table_words);
    std::fill(win.begin() + 33 + W, win.end(), ~0ull);
    if (int rc = for_members(p, [&](size_t m, const Lane &c) {
            if (!run[m].d_tables) return DVT_OK;
            if (!c.eng.download(one.data(), run[m].d_tables, table_words * 8)) return engine_fail(c.err, c.eng);
            win[0] += one[0];
            for (size_t i = 1; i < 33 + W; i++) win[i] = std::max(win[i], one[i]);
            for (size_t i = 33 + W; i < table_words; i++) win[i] = std::min(win[i], one[i]);
            return DVT_OK;
        }))
        return rc;
    if (win[0]) return fail(p, DVT_ERR_INPUT, "%llu %s", win[0], BAD_RECORD);

    // ---- gather: every winner from the member that holds its shard; the call records of the frames that are returned
    struct Want { size_t m, at; uint32_t what, index; };
    std::vector<Want> wants;
    auto want = [&](unsigned long long where, uint32_t addr, uint32_t what, uint32_t index) {
        const Held *h = pl.holder(where);
        if (!h) return false;
        wants.push_back({h->m, run[h->m].fetch.size(), what, index});
        run[h->m].fetch.push_back(SnapFetch{h->s->d_recs, (uint32_t)h->s->n_recs, (uint32_t)(where >> 32), (uint32_t)where, addr, what, 0});
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
    double ms[3] = {0, 0, 0};
    if (int rc = for_members(p, [&](size_t m, const Lane &c) {
            Engine &e = c.eng;
            SnapMember &sm = run[m];
            if (!sm.fetch.empty()) {
                HIP_TRY(c.err, e.pool.alloc_bytes(&sm.items.ptr, sm.fetch.size() * sizeof(SnapFetch)));
                HIP_TRY(c.err, e.pool.alloc_bytes(&sm.sides.ptr, sm.fetch.size() * sizeof(snap::Side)));
                HIP_TRY(c.err, hipMemcpyAsync(sm.items.ptr, sm.fetch.data(), sm.fetch.size() * sizeof(SnapFetch), hipMemcpyHostToDevice, e.stream));
                args.statics = sm.d_statics; args.offs = sm.d_statics + n; args.shard = 0;
                HIP_TRY(c.err, sm.t_gather.begin(e.stream));
                HIP_TRY(c.err, launch_snapshot_gather(e.stream, static_cast<const SnapFetch *>(sm.items.ptr), (uint32_t)sm.fetch.size(), args, sm.sides.ptr));
                HIP_TRY(c.err, sm.t_gather.end(e.stream));
                sm.got.resize(sm.fetch.size());
                if (!e.download(sm.got.data(), sm.sides.ptr, sm.got.size() * sizeof(snap::Side))) return engine_fail(c.err, e);
            }
            ms[0] += sm.t_reduce.ms(); ms[1] += sm.t_gather.ms(); ms[2] += ct[m].t_summaries.ms() + ct[m].t_calls.ms();
            return DVT_OK;
        }))
        return rc;

    snap::Side reg[32] = {};
    std::vector<snap::Side> before(W, snap::Side{}), after(W, snap::Side{});
    std::vector<snap::CallRec> calls(depth);
    for (const Want &w : wants) {
        const snap::Side &s = run[w.m].got[w.at];
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

// ------------------------------------------------------------------ origins (dvt_rv32_job_origin)
// origin::Search runs the rule on the host and asks its questions level by level.  A level is answered in chunks of
// DVT_ORIGIN_PASS_QUESTIONS sorted questions: every member that holds shards before the chunk's largest position runs the reduce
// pass over them on lane 0's stream (one launch per such shard, over its records before that position) into its own winners;
// the host merges the members' winners with max and asks the member that holds each winner's shard for the record (gather, one
// fetch per distinct position of the level).
namespace {
struct OriginMember : GatherMember {
    StageBuf base;
    unsigned long long *d_win = nullptr, *d_qpos = nullptr;   // [PASS_Q] winners and behind them the bad records [1]; [PASS_Q]
    uint32_t *d_qtarget = nullptr;                             // [PASS_Q]
    uint32_t *d_statics = nullptr;
    EventSpan t_reduce;
    explicit OriginMember(DevPool &pool) : base{pool} {}
};
}  // namespace

static int job_origin(dvt_prover *p, const dvt_pk *pk, dvt_job *j, uint32_t shard, uint32_t row, uint32_t what, uint32_t target, uint32_t flags,
                      uint32_t max_depth, dvt_origin_node *nodes, size_t cap_nodes, dvt_origin_edge *edges, size_t cap_edges, dvt_origin_summary *summary) {
    if (int rc = same_members(p, pk, j)) return rc;
    if (int rc = whole_execution(p, j, "origin of a value")) return rc;
    const auto t0 = Clock::now();
    const rv32::Program &prog = pk->prog;
    constexpr size_t PQ = PASS_Q;
    MemberRun<OriginMember> run(p);   // (declared first: however the call ends, member 0's device is current again)
    Placed pl;
    if (int rc = pl.init(p, j, shard, row)) return rc;
    const watch::Statics statics(prog);
    const watch::Shapes shapes = watch::shapes();
    const size_t n = statics.n();
    auto layout = [&](OriginMember &om, Carve c) {
        om.d_win = c.take<unsigned long long>(PQ + 1);
        om.d_qpos = c.take<unsigned long long>(PQ);
        om.d_recs = c.take<rv32::CycleRec>(origin::MAX_EDGES, 16);
        om.d_fetch = c.take<OriginFetch>(origin::MAX_EDGES);
        om.d_qtarget = c.take<uint32_t>(PQ);
        om.d_statics = c.take<uint32_t>(statics.words.size());
        return c.at;
    };
    auto buffers = [&](const Lane &c, OriginMember &om) {
        if (om.base.ptr) return DVT_OK;
        HIP_TRY(c.err, c.eng.pool.alloc_bytes(&om.base.ptr, layout(om, Carve{})));   // (over no base: the size; the pointers follow)
        layout(om, Carve{static_cast<char *>(om.base.ptr)});
        HIP_TRY(c.err, hipMemcpyAsync(om.d_statics, statics.words.data(), statics.bytes(), hipMemcpyHostToDevice, c.eng.stream));
        return DVT_OK;
    };

    double ms[2] = {0, 0};
    uint64_t bad = 0;
    uint32_t passes = 0;
    int rc_answer = DVT_OK;
    auto answer = [&](const std::vector<origin::Question> &qs, std::vector<origin::Found> *found) {
        Chunks chunks(qs);
        const std::vector<uint32_t> &order = chunks.order;
        std::vector<unsigned long long> win(qs.size(), 0), one(PQ + 1);
        // ---- reduce: one pass per chunk of the sorted questions
        for (size_t at = 0; at < order.size(); at += PQ) {
            OriginArgs args{};
            args.sh = shapes;
            args.n_instr = (uint32_t)n; args.text_base = prog.text_base;
            const size_t n_q = chunks.cut(at, &args);
            args.max_q = *std::max_element(chunks.pos.begin(), chunks.pos.begin() + n_q);
            const uint32_t q_shard = (uint32_t)(args.max_q >> 32), q_row = (uint32_t)args.max_q;
            auto take = [&](const ShardJob &s) { return s.index < q_shard ? s.n_recs : s.index == q_shard ? std::min<size_t>(s.n_recs, q_row) : 0; };
            passes++;
            rc_answer = for_members(p, [&](size_t m, const Lane &c) {
                Engine &e = c.eng;
                OriginMember &om = run[m];
                JobPart &part = j->parts[m];
                bool any = false;
                for (auto &s : part.shards) any = any || take(s);
                if (!any) return DVT_OK;
                if (int rc = buffers(c, om)) return rc;
                HIP_TRY(c.err, hipMemsetAsync(om.d_win, 0, (PQ + 1) * 8, e.stream));
                HIP_TRY(c.err, hipMemcpyAsync(om.d_qpos, chunks.pos.data(), n_q * 8, hipMemcpyHostToDevice, e.stream));
                HIP_TRY(c.err, hipMemcpyAsync(om.d_qtarget, chunks.target.data(), n_q * 4, hipMemcpyHostToDevice, e.stream));
                OriginArgs a = args;
                a.statics = om.d_statics; a.offs = om.d_statics + n; a.target = om.d_qtarget; a.pos = om.d_qpos;
                HIP_TRY(c.err, om.t_reduce.begin(e.stream));
                for (auto &s : part.shards) {
                    a.shard = s.index;
                    HIP_TRY(c.err, launch_origin_reduce(e.stream, s.d_recs, take(s), a, om.d_win, om.d_win + PQ));
                }
                HIP_TRY(c.err, om.t_reduce.end(e.stream));
                if (!e.download(one.data(), om.d_win, (PQ + 1) * 8)) return engine_fail(c.err, e);
                ms[0] += om.t_reduce.ms();
                bad += one[PQ];
                for (size_t i = 0; i < n_q; i++) win[order[at + i]] = std::max(win[order[at + i]], one[i]);
                return DVT_OK;
            });
            if (rc_answer) return false;
        }
        if (bad) return true;   // (the call fails below: no record is read again)
        // ---- gather: every distinct winner from the member that holds its shard
        std::vector<unsigned long long> want;
        for (const unsigned long long w : win)
            if (w) want.push_back(w);
        std::map<unsigned long long, rv32::CycleRec> recs;
        rc_answer = gather_records(p, pl, run, want, buffers, "a winner of the reduce pass lies in no shard of the job", "more winners than questions", &ms[1], &recs);
        if (rc_answer) return false;
        for (size_t i = 0; i < qs.size(); i++)
            if (win[i]) (*found)[i] = origin::Found{win[i], recs[win[i]]};
        return true;
    };

    origin::Search search(prog, statics, shapes, watch::position(shard, row), what, target, flags, max_depth, nodes, cap_nodes, edges, cap_edges);
    const int rc = search.run(answer);
    return finish_search(p, rc, rc_answer, bad, search, passes, pl, t0, ms, 2, p->origin_ms, summary);
}

// ------------------------------------------------------------------ uses (dvt_rv32_job_uses)
// uses::Search runs the rule on the host and asks its definitions level by level.  A level is answered in chunks of
// DVT_USES_PASS_DEFS sorted definitions.  Per chunk every member that holds records at or after the chunk's smallest F runs the
// next pass over them on lane 0's stream into its own winners, and the host merges them with min.  With the windows [F, N] known,
// every member that holds records in [min F, max N] counts the uses per span, scans the spans in execution order and emits its
// own first `fan` uses and its total per definition; the host sums the totals and keeps the fan smallest positions of the union.
// The consumers' records come from the member that holds each one's shard (origin.hip's gather, one fetch per distinct position
// of the level).
namespace {
struct UsesMember : GatherMember {
    StageBuf base;
    unsigned long long *d_win = nullptr, *d_from = nullptr, *d_next = nullptr;   // [PASS_DEFS] each; behind d_win the bad records [1]
    unsigned long long *d_carry = nullptr;   // [PASS_DEFS] and behind them out_pos [PASS_DEFS * MAX_FAN]
    UsesItem *d_items = nullptr;             // [PASS_DEFS * MAX_FAN]
    uint32_t *d_target = nullptr, *d_out_role = nullptr, *d_n_items = nullptr, *d_table = nullptr;
    uint32_t *d_statics = nullptr, *d_ostat = nullptr;
    size_t table_rows = 0;                   // the spans of the shards the member holds
    std::vector<const Held *> shards;        // in execution order
    EventSpan t_next, t_count, t_emit;
    explicit UsesMember(DevPool &pool) : base{pool} {}
};
}  // namespace

static int job_uses(dvt_prover *p, const dvt_pk *pk, dvt_job *j, uint32_t shard, uint32_t row, uint32_t what, uint32_t target, uint32_t flags,
                    uint32_t max_depth, uint32_t fan, dvt_uses_node *nodes, size_t cap_nodes, dvt_uses_def *defs, size_t cap_defs, dvt_uses_edge *edges,
                    size_t cap_edges, dvt_uses_summary *summary) {
    if (int rc = same_members(p, pk, j)) return rc;
    if (int rc = whole_execution(p, j, "uses of a value")) return rc;
    const auto t0 = Clock::now();
    const rv32::Program &prog = pk->prog;
    constexpr size_t PD = PASS_Q, SPAN = uses::SPAN, MAX_ITEMS = PD * uses::MAX_FAN;
    MemberRun<UsesMember> run(p);   // (declared first: however the call ends, member 0's device is current again)
    Placed pl;
    if (int rc = pl.init(p, j, shard, row)) return rc;
    for (const Held &h : pl.held) {
        run[h.m].shards.push_back(&h);
        run[h.m].table_rows += (h.s->n_recs + SPAN - 1) / SPAN;
    }
    const watch::Statics statics(prog);
    const flow::Statics ostat(prog);
    const watch::Shapes shapes = watch::shapes();
    const size_t n = statics.n();
    auto layout = [&](UsesMember &um, Carve c) {
        um.d_win = c.take<unsigned long long>(PD + 1);
        um.d_from = c.take<unsigned long long>(PD);
        um.d_next = c.take<unsigned long long>(PD);
        um.d_carry = c.take<unsigned long long>(PD + MAX_ITEMS);
        um.d_recs = c.take<rv32::CycleRec>(uses::MAX_EDGES, 16);
        um.d_fetch = c.take<OriginFetch>(uses::MAX_EDGES);
        um.d_items = c.take<UsesItem>(MAX_ITEMS);
        um.d_target = c.take<uint32_t>(PD);
        um.d_out_role = c.take<uint32_t>(MAX_ITEMS);
        um.d_n_items = c.take<uint32_t>(4);
        um.d_statics = c.take<uint32_t>(statics.words.size());
        um.d_ostat = c.take<uint32_t>(n);
        um.d_table = c.take<uint32_t>(um.table_rows * PD);
        return c.at;
    };
    auto buffers = [&](const Lane &c, UsesMember &um) {
        if (um.base.ptr) return DVT_OK;
        HIP_TRY(c.err, c.eng.pool.alloc_bytes(&um.base.ptr, layout(um, Carve{})));   // (over no base: the size; the pointers follow)
        layout(um, Carve{static_cast<char *>(um.base.ptr)});
        HIP_TRY(c.err, hipMemcpyAsync(um.d_statics, statics.words.data(), statics.bytes(), hipMemcpyHostToDevice, c.eng.stream));
        HIP_TRY(c.err, hipMemcpyAsync(um.d_ostat, ostat.words.data(), n * 4, hipMemcpyHostToDevice, c.eng.stream));
        return DVT_OK;
    };
    // the spans of shard s that hold a position in [lo, hi]: {first, count}
    auto spans_in = [&](const ShardJob &s, unsigned long long lo, unsigned long long hi) {
        if (!s.n_recs) return std::pair<uint32_t, uint32_t>{0, 0};
        const unsigned long long first_pos = watch::position(s.index, 0), last_pos = watch::position(s.index, (uint32_t)(s.n_recs - 1));
        if (hi < first_pos || lo > last_pos) return std::pair<uint32_t, uint32_t>{0, 0};
        const uint32_t r0 = lo > first_pos ? (uint32_t)lo : 0, r1 = hi < last_pos ? (uint32_t)hi : (uint32_t)(s.n_recs - 1);
        return std::pair<uint32_t, uint32_t>{(uint32_t)(r0 / SPAN), (uint32_t)(r1 / SPAN - r0 / SPAN + 1)};
    };

    double ms[4] = {0, 0, 0, 0};
    uint64_t bad = 0;
    uint32_t passes = 0;
    int rc_answer = DVT_OK;
    auto answer = [&](const std::vector<uses::Def> &qs, std::vector<uses::Found> *found) {
        Chunks chunks(qs);
        const std::vector<uint32_t> &order = chunks.order, &d_target = chunks.target;
        const std::vector<unsigned long long> &d_from = chunks.pos;
        std::vector<unsigned long long> one(PD + 1), d_next(PD), carry(PD + MAX_ITEMS);
        std::vector<uint32_t> out_role(MAX_ITEMS);
        struct Kept { unsigned long long pos; uint32_t role; };
        std::vector<std::vector<Kept>> kept(qs.size());
        for (size_t at = 0; at < order.size(); at += PD) {
            UsesArgs args{};
            args.sh = shapes;
            args.n_instr = (uint32_t)n; args.text_base = prog.text_base; args.flags = flags; args.fan = fan;
            const size_t n_d = chunks.cut(at, &args);
            args.min_from = *std::min_element(d_from.begin(), d_from.begin() + n_d);
            std::fill(d_next.begin(), d_next.begin() + n_d, uses::NO_POS);
            passes++;
            // ---- next: the first writer at or after F, per member, merged with min
            rc_answer = for_members(p, [&](size_t m, const Lane &c) {
                Engine &e = c.eng;
                UsesMember &um = run[m];
                bool any = false;
                for (const Held *h : um.shards) any = any || spans_in(*h->s, args.min_from, uses::NO_POS).second;
                if (!any) return DVT_OK;
                if (int rc = buffers(c, um)) return rc;
                HIP_TRY(c.err, hipMemsetAsync(um.d_win, 0xff, PD * 8, e.stream));
                HIP_TRY(c.err, hipMemsetAsync(um.d_win + PD, 0, 8, e.stream));
                HIP_TRY(c.err, hipMemcpyAsync(um.d_from, d_from.data(), n_d * 8, hipMemcpyHostToDevice, e.stream));
                HIP_TRY(c.err, hipMemcpyAsync(um.d_target, d_target.data(), n_d * 4, hipMemcpyHostToDevice, e.stream));
                UsesArgs a = args;
                a.statics = um.d_statics; a.offs = um.d_statics + n; a.ostat = um.d_ostat; a.target = um.d_target; a.pos = um.d_from; a.d_next = um.d_next;
                HIP_TRY(c.err, um.t_next.begin(e.stream));
                for (const Held *h : um.shards) {
                    const auto sp = spans_in(*h->s, args.min_from, uses::NO_POS);
                    a.shard = h->s->index;
                    HIP_TRY(c.err, launch_uses_next(e.stream, h->s->d_recs, h->s->n_recs, sp.first, sp.second, a, um.d_win, um.d_win + PD));
                }
                HIP_TRY(c.err, um.t_next.end(e.stream));
                if (!e.download(one.data(), um.d_win, (PD + 1) * 8)) return engine_fail(c.err, e);
                ms[0] += um.t_next.ms();
                bad += one[PD];
                for (size_t i = 0; i < n_d; i++) d_next[i] = std::min(d_next[i], one[i]);
                return DVT_OK;
            });
            if (rc_answer) return false;
            if (bad) return true;   // (the call fails below: no record is read again)
            args.max_next = 0;
            for (size_t i = 0; i < n_d; i++) {
                (*found)[order[at + i]].next = d_next[i];
                args.max_next = std::max(args.max_next, d_next[i]);
            }
            // ---- count, scan, emit: every member's own totals and first `fan` uses
            rc_answer = for_members(p, [&](size_t m, const Lane &c) {
                Engine &e = c.eng;
                UsesMember &um = run[m];
                bool any = false;
                for (const Held *h : um.shards) any = any || spans_in(*h->s, args.min_from, args.max_next).second;
                if (!any) return DVT_OK;
                if (int rc = buffers(c, um)) return rc;
                HIP_TRY(c.err, hipMemcpyAsync(um.d_from, d_from.data(), n_d * 8, hipMemcpyHostToDevice, e.stream));
                HIP_TRY(c.err, hipMemcpyAsync(um.d_target, d_target.data(), n_d * 4, hipMemcpyHostToDevice, e.stream));
                HIP_TRY(c.err, hipMemcpyAsync(um.d_next, d_next.data(), n_d * 8, hipMemcpyHostToDevice, e.stream));
                HIP_TRY(c.err, hipMemsetAsync(um.d_carry, 0, PD * 8, e.stream));
                HIP_TRY(c.err, hipMemsetAsync(um.d_n_items, 0, 16, e.stream));
                UsesArgs a = args;
                a.statics = um.d_statics; a.offs = um.d_statics + n; a.ostat = um.d_ostat; a.target = um.d_target; a.pos = um.d_from; a.d_next = um.d_next;
                HIP_TRY(c.err, um.t_count.begin(e.stream));
                size_t table_row = 0;
                for (const Held *h : um.shards) {
                    const auto sp = spans_in(*h->s, args.min_from, args.max_next);
                    a.shard = h->s->index;
                    HIP_TRY(c.err, launch_uses_count(e.stream, h->s->d_recs, h->s->n_recs, sp.first, sp.second, a, um.d_table, table_row, um.table_rows));
                    table_row += sp.second;
                }
                table_row = 0;
                for (const Held *h : um.shards) {
                    const auto sp = spans_in(*h->s, args.min_from, args.max_next);
                    HIP_TRY(c.err, launch_uses_scan(e.stream, um.d_table, table_row, sp.second, um.table_rows, h->s->d_recs, h->s->n_recs, h->s->index, sp.first,
                                                    (uint32_t)n_d, fan, um.d_carry, um.d_items, um.d_n_items, (uint32_t)(n_d * fan)));
                    table_row += sp.second;
                }
                HIP_TRY(c.err, um.t_count.end(e.stream));
                um.t_emit.begin_at_end_of(um.t_count);
                HIP_TRY(c.err, launch_uses_emit(e.stream, um.d_items, um.d_n_items, (uint32_t)(n_d * fan), a, um.d_carry + PD, um.d_out_role));
                HIP_TRY(c.err, um.t_emit.end(e.stream));
                if (!e.download(out_role.data(), um.d_out_role, n_d * fan * 4)) return engine_fail(c.err, e);
                if (!e.download(carry.data(), um.d_carry, (PD + n_d * fan) * 8)) return engine_fail(c.err, e);   // (carry | out_pos, adjacent)
                const unsigned long long *out_pos = carry.data() + PD;
                ms[1] += um.t_count.ms();
                ms[2] += um.t_emit.ms();
                for (size_t i = 0; i < n_d; i++) {
                    const size_t qi = order[at + i];
                    (*found)[qi].n_uses += carry[i];
                    for (size_t r = 0; r < std::min<unsigned long long>(fan, carry[i]); r++) kept[qi].push_back(Kept{out_pos[i * fan + r], out_role[i * fan + r]});
                }
                return DVT_OK;
            });
            if (rc_answer) return false;
        }
        // ---- the fan smallest of the members' kept uses; gather: every distinct consumer from the member that holds its shard
        std::vector<unsigned long long> want;
        for (size_t i = 0; i < qs.size(); i++) {
            std::stable_sort(kept[i].begin(), kept[i].end(), [](const Kept &x, const Kept &y) { return x.pos != y.pos ? x.pos < y.pos : x.role < y.role; });
            if (kept[i].size() > fan) kept[i].resize(fan);
            for (const Kept &k : kept[i]) want.push_back(k.pos);
        }
        std::map<unsigned long long, rv32::CycleRec> recs;
        rc_answer = gather_records(p, pl, run, want, buffers, "a use of the emit pass lies in no shard of the job", "more kept uses than edges", &ms[3], &recs);
        if (rc_answer) return false;
        for (size_t i = 0; i < qs.size(); i++)
            for (const Kept &k : kept[i]) (*found)[i].uses.push_back(uses::Use{k.pos, k.role, recs[k.pos]});
        return true;
    };

    uses::Search search(prog, statics, shapes, watch::position(shard, row), what, target, flags, max_depth, fan, nodes, cap_nodes, defs, cap_defs, edges,
                        cap_edges);
    const int rc = search.run(answer);
    return finish_search(p, rc, rc_answer, bad, search, passes, pl, t0, ms, 4, p->uses_ms, summary);
}

// ------------------------------------------------------------------ divergence (dvt_rv32_job_diverge)
// The host cuts the pairs [0, N) into segments in which each side stays inside one shard (at most shardsA + shardsB of them; with
// equal starts one per shard) and numbers their spans in pair order.  A segment is classified on lane 0's stream of the member
// that holds both of its shards.  Segments are launched in batches of at most DVT_DIVERGE_BATCH_PAIRS pairs; after a batch the
// host reads the stop flag and, once a stop is found, launches no later batch.  With several members the span records of the
// others are relayed to member 0, which merges; the merged counts and rank bases go back for the emit, and every member's kept
// pairs are picked from its own arrays.  Pairs stop - 1 and stop and the rejoin windows come out by origin.hip's gather.
namespace {
struct DivergeMember {
    StageBuf base;
    DivergeSpan *d_spans = nullptr;
    DivergeSpanRegs *d_span_regs = nullptr;
    unsigned long long *d_rank = nullptr, *d_stop = nullptr;
    DivergeMerged *d_merged = nullptr;
    dvt_diverge_pair *d_first = nullptr, *d_last = nullptr;
    OriginFetch *d_items = nullptr;
    rv32::CycleRec *d_recs = nullptr;
    const uint32_t *d_statics = nullptr;
    EventSpan t_classify, t_merge, t_emit, t_gather;
    explicit DivergeMember(DevPool &pool) : base{pool} {}
};
struct DivergeSegment {
    unsigned long long k0;
    uint32_t n, span0, n_spans;
    size_t m;
    const rv32::CycleRec *rec_a, *rec_b;
    dvt_diverge_pos at_a, at_b;
};
}  // namespace

static int job_diverge(dvt_prover *p, const dvt_pk *pk, dvt_job *ja, dvt_job *jb, dvt_diverge_pos start_a, dvt_diverge_pos start_b, uint64_t max_pairs,
                       uint32_t flags, uint32_t window, uint32_t K, dvt_diverge_pair *first, dvt_diverge_pair *last, dvt_diverge_reg regs[32],
                       dvt_diverge_summary *summary) {
    if (int rc = same_members(p, pk, ja)) return rc;
    if (int rc = same_members(p, pk, jb)) return rc;
    if (int rc = whole_execution(p, ja, "divergence of two executions")) return rc;
    if (int rc = whole_execution(p, jb, "divergence of two executions")) return rc;
    const auto t0 = Clock::now();
    const rv32::Program &prog = pk->prog;
    MemberRun<DivergeMember> run(p);   // (declared first: however the call ends, member 0's device is current again)
    const std::vector<Held> held[2] = {held_in_order(ja), held_in_order(jb)};
    diverge::Stream st[2];
    for (int x = 0; x < 2; x++)
        for (const Held &h : held[x]) {
            if (h.s->n_recs > 0xffffffffull) return fail(p, DVT_ERR_INPUT, "shard %zu has %zu records", h.pos, h.s->n_recs);
            st[x].shard_n.push_back(h.s->n_recs);
        }
    const uint64_t g[2] = {st[0].global_of(start_a), st[1].global_of(start_b)};
    uint64_t N = std::min(st[0].len() - g[0], st[1].len() - g[1]);
    if (max_pairs) N = std::min<uint64_t>(N, max_pairs);

    // ---- the segments
    std::vector<DivergeSegment> segs;
    uint64_t n_spans = 0;
    {
        dvt_diverge_pos at[2] = {st[0].locate(g[0]), st[1].locate(g[1])};
        for (uint64_t k = 0; k < N;) {
            for (int x = 0; x < 2; x++)
                while (at[x].shard <= st[x].shard_n.size() && at[x].row >= st[x].shard_n[at[x].shard - 1]) { at[x].shard++; at[x].row = 0; }
            const Held &ha = held[0][at[0].shard - 1], &hb = held[1][at[1].shard - 1];
            const uint64_t n = std::min({N - k, st[0].shard_n[at[0].shard - 1] - at[0].row, st[1].shard_n[at[1].shard - 1] - at[1].row});
            if (ha.m != hb.m)
                return fail(p, DVT_ERR_UNSUPPORTED, "segment %zu (pairs %llu..%llu): shard %u of A is held by member %zu, shard %u of B by member %zu", segs.size(),
                            (unsigned long long)k, (unsigned long long)(k + n), at[0].shard, ha.m, at[1].shard, hb.m);
            const uint32_t spans = (uint32_t)((n + diverge::SPAN - 1) / diverge::SPAN);
            segs.push_back(DivergeSegment{k, (uint32_t)n, (uint32_t)n_spans, spans, ha.m, ha.s->d_recs + at[0].row, hb.s->d_recs + at[1].row, at[0], at[1]});
            n_spans += spans;
            k += n;
            at[0].row += (uint32_t)n; at[1].row += (uint32_t)n;
        }
    }
    if (n_spans > 0x7fffffffull) return fail(p, DVT_ERR_UNSUPPORTED, "%llu spans", (unsigned long long)n_spans);
    const uint32_t win = window ? window : diverge::DEFAULT_WINDOW;
    const size_t cap_items = 2 * ((size_t)diverge::MAX_WINDOW + 2);
    const watch::Statics statics(prog);
    const watch::Shapes shapes = watch::shapes();
    const size_t n_instr = statics.n(), cap_spans = std::max<size_t>(n_spans, 1);
    // a member's buffer: merged | stop flag | rank bases | fetched records | fetch items | kept pairs | span records | span registers | statics
    const size_t bytes = sizeof(DivergeMerged) + 16 + cap_spans * 8 + 8 + cap_items * (sizeof(rv32::CycleRec) + sizeof(OriginFetch)) +
                         2 * diverge::MAX_KEEP * sizeof(dvt_diverge_pair) + cap_spans * (sizeof(DivergeSpan) + sizeof(DivergeSpanRegs)) + statics.bytes();
    auto buffers = [&](const Lane &c, DivergeMember &dm) {
        if (dm.base.ptr) return DVT_OK;
        Engine &e = c.eng;
        HIP_TRY(c.err, e.pool.alloc_bytes(&dm.base.ptr, bytes));
        dm.d_merged = static_cast<DivergeMerged *>(dm.base.ptr);
        dm.d_stop = reinterpret_cast<unsigned long long *>(dm.d_merged + 1);
        dm.d_rank = dm.d_stop + 2;                                                 // (what lies behind stays 16-byte aligned)
        dm.d_recs = reinterpret_cast<rv32::CycleRec *>(dm.d_rank + cap_spans + (cap_spans & 1));
        dm.d_items = reinterpret_cast<OriginFetch *>(dm.d_recs + cap_items);
        dm.d_first = reinterpret_cast<dvt_diverge_pair *>(dm.d_items + cap_items);
        dm.d_last = dm.d_first + diverge::MAX_KEEP;
        dm.d_spans = reinterpret_cast<DivergeSpan *>(dm.d_last + diverge::MAX_KEEP);
        dm.d_span_regs = reinterpret_cast<DivergeSpanRegs *>(dm.d_spans + cap_spans);
        uint32_t *d_stat = reinterpret_cast<uint32_t *>(dm.d_span_regs + cap_spans);
        dm.d_statics = d_stat;
        HIP_TRY(c.err, hipMemsetAsync(dm.d_stop, 0xff, 8, e.stream));
        HIP_TRY(c.err, hipMemsetAsync(dm.d_first, 0xff, 2 * diverge::MAX_KEEP * sizeof(dvt_diverge_pair), e.stream));
        HIP_TRY(c.err, hipMemcpyAsync(d_stat, statics.words.data(), statics.bytes(), hipMemcpyHostToDevice, e.stream));
        return DVT_OK;
    };
    auto args_of = [&](const DivergeSegment &sg, const DivergeMember &dm) {
        DivergeArgs a{};
        a.sh = shapes;
        a.statics = dm.d_statics; a.offs = dm.d_statics + n_instr;
        a.rec_a = sg.rec_a; a.rec_b = sg.rec_b;
        a.k0 = sg.k0;
        a.n_instr = (uint32_t)n_instr; a.text_base = prog.text_base; a.n_pairs = sg.n; a.span0 = sg.span0;
        a.shard_a = sg.at_a.shard; a.row_a = sg.at_a.row; a.shard_b = sg.at_b.shard; a.row_b = sg.at_b.row;
        return a;
    };

    // ---- classify, batch by batch
    double ms[3] = {0, 0, 0};
    unsigned long long stop_flag = diverge::NONE;
    uint64_t launched_pairs = 0;
    size_t done = 0;   // segments launched
    while (done < segs.size() && stop_flag == diverge::NONE) {
        size_t end = done;
        uint64_t batch = 0;
        while (end < segs.size() && (end == done || batch + segs[end].n <= diverge::BATCH_PAIRS)) batch += segs[end++].n;
        if (int rc = for_members(p, [&](size_t m, const Lane &c) {
                Engine &e = c.eng;
                DivergeMember &dm = run[m];
                bool any = false;
                for (size_t i = done; i < end; i++) any = any || segs[i].m == m;
                if (!any) return DVT_OK;
                if (int rc = buffers(c, dm)) return rc;
                HIP_TRY(c.err, dm.t_classify.begin(e.stream));
                for (size_t i = done; i < end; i++)
                    if (segs[i].m == m) HIP_TRY(c.err, launch_diverge_classify(e.stream, args_of(segs[i], dm), dm.d_spans, dm.d_span_regs, (uint32_t)cap_spans, dm.d_stop));
                HIP_TRY(c.err, dm.t_classify.end(e.stream));
                unsigned long long flag = diverge::NONE;
                if (!e.download(&flag, dm.d_stop, 8)) return engine_fail(c.err, e);
                ms[0] += dm.t_classify.ms();
                stop_flag = std::min(stop_flag, flag);
                return DVT_OK;
            }))
            return rc;
        launched_pairs += batch;
        done = end;
    }
    const uint32_t spans_done = done ? segs[done - 1].span0 + segs[done - 1].n_spans : 0;

    // ---- the span records of the other members to member 0, which merges
    DivergeMerged merged{};
    merged.first_data = merged.last_data = diverge::NONE;
    for (uint32_t r = 0; r < 32; r++) merged.reg_first_diff[r] = merged.reg_last_diff[r] = merged.reg_last_write[r] = diverge::NONE;
    std::vector<unsigned long long> rank_base;
    if (spans_done) {
        std::vector<std::vector<uint8_t>> relay(done);   // per segment of another member: its span records, then its span registers
        if (n_members(p) > 1) {
            if (int rc = for_members(p, [&](size_t m, const Lane &c) {
                    if (!m) return DVT_OK;
                    for (size_t i = 0; i < done; i++) {
                        if (segs[i].m != m) continue;
                        const size_t a = segs[i].n_spans * sizeof(DivergeSpan), b = segs[i].n_spans * sizeof(DivergeSpanRegs);
                        relay[i].resize(a + b);
                        if (!c.eng.download(relay[i].data(), run[m].d_spans + segs[i].span0, a) || !c.eng.download(relay[i].data() + a, run[m].d_span_regs + segs[i].span0, b))
                            return engine_fail(c.err, c.eng);
                    }
                    return DVT_OK;
                }))
                return rc;
        }
        {
            const Lane c = lane0(p, 0);
            Engine &e = c.eng;
            DivergeMember &dm = run[0];
            if (int rc = buffers(c, dm)) return rc;
            for (size_t i = 0; i < done; i++) {
                if (relay[i].empty()) continue;
                const size_t a = segs[i].n_spans * sizeof(DivergeSpan), b = segs[i].n_spans * sizeof(DivergeSpanRegs);
                HIP_TRY(c.err, hipMemcpyAsync(dm.d_spans + segs[i].span0, relay[i].data(), a, hipMemcpyHostToDevice, e.stream));
                HIP_TRY(c.err, hipMemcpyAsync(dm.d_span_regs + segs[i].span0, relay[i].data() + a, b, hipMemcpyHostToDevice, e.stream));
            }
            HIP_TRY(c.err, dm.t_merge.begin(e.stream));
            HIP_TRY(c.err, launch_diverge_merge(e.stream, dm.d_spans, dm.d_span_regs, spans_done, dm.d_rank, dm.d_merged));
            HIP_TRY(c.err, dm.t_merge.end(e.stream));
            if (!e.download(&merged, dm.d_merged, sizeof(merged))) return engine_fail(c.err, e);   // (the relayed bytes outlive the copies: this synchronises)
            ms[1] += dm.t_merge.ms();
        }
    }
    diverge::Counts cnt;
    cnt.stop = merged.stop; cnt.stopped = merged.stopped; cnt.mask = merged.mask;
    cnt.n_data = merged.n_data; cnt.first_data = merged.first_data; cnt.last_data = merged.last_data; cnt.n_load = merged.n_load; cnt.n_store = merged.n_store;
    for (uint32_t r = 1; r < 32; r++) {
        cnt.reg[r].n_diff = merged.reg_n_diff[r]; cnt.reg[r].first_diff = merged.reg_first_diff[r];
        cnt.reg[r].last_diff = merged.reg_last_diff[r]; cnt.reg[r].last_write = merged.reg_last_write[r];
    }
    if (cnt.stop > N || merged.n_used > spans_done) return fail(p, DVT_ERR_DEVICE, "the merge pass stops past the pairs of the call");

    // ---- emit: every member over its segments that count
    if (K && cnt.n_data) {
        std::vector<DivergeSpan> h_spans;
        if (n_members(p) > 1) {   // the other members take the merged counts, the rank bases and the span records from member 0
            const Lane c = lane0(p, 0);
            rank_base.resize(spans_done);
            h_spans.resize(spans_done);
            if (!c.eng.download(rank_base.data(), run[0].d_rank, spans_done * 8) || !c.eng.download(h_spans.data(), run[0].d_spans, spans_done * sizeof(DivergeSpan)))
                return engine_fail(c.err, c.eng);
        }
        std::vector<dvt_diverge_pair> got(2 * diverge::MAX_KEEP);
        const watch::Keep keep = watch::keep_of(cnt.n_data, K);
        if (int rc = for_members(p, [&](size_t m, const Lane &c) {
                Engine &e = c.eng;
                DivergeMember &dm = run[m];
                bool any = false;
                for (size_t i = 0; i < done; i++) any = any || (segs[i].m == m && segs[i].span0 < merged.n_used);
                if (!any) return DVT_OK;
                if (m) {
                    HIP_TRY(c.err, hipMemcpyAsync(dm.d_merged, &merged, sizeof(merged), hipMemcpyHostToDevice, e.stream));
                    HIP_TRY(c.err, hipMemcpyAsync(dm.d_rank, rank_base.data(), spans_done * 8, hipMemcpyHostToDevice, e.stream));
                    HIP_TRY(c.err, hipMemcpyAsync(dm.d_spans, h_spans.data(), spans_done * sizeof(DivergeSpan), hipMemcpyHostToDevice, e.stream));
                }
                HIP_TRY(c.err, dm.t_emit.begin(e.stream));
                for (size_t i = 0; i < done; i++)
                    if (segs[i].m == m && segs[i].span0 < merged.n_used)
                        HIP_TRY(c.err, launch_diverge_emit(e.stream, args_of(segs[i], dm), dm.d_spans, dm.d_rank, dm.d_merged, (uint32_t)cap_spans, K, dm.d_first, dm.d_last));
                HIP_TRY(c.err, dm.t_emit.end(e.stream));
                if (!e.download(got.data(), dm.d_first, got.size() * sizeof(dvt_diverge_pair))) return engine_fail(c.err, e);
                ms[2] += dm.t_emit.ms();
                for (size_t r = 0; r < keep.first_end && r < K; r++)   // (a slot no span of this member owns is all ones)
                    if (got[r].k != diverge::NONE) first[r] = got[r];
                for (size_t r = 0; r < keep.first_end && r < K; r++)
                    if (got[diverge::MAX_KEEP + r].k != diverge::NONE) last[r] = got[diverge::MAX_KEEP + r];
                return DVT_OK;
            }))
            return rc;
    }

    // ---- gather: pairs stop - 1 and stop, and the rejoin windows when the runs split
    const bool want_rejoin = (flags & DVT_DIVERGE_REJOIN) && cnt.stopped == 1;
    std::vector<rv32::CycleRec> near[2];   // side x: the records from global number lo[x] on
    uint64_t lo[2];
    {
        struct Want { int x; size_t i; };
        std::vector<std::vector<OriginFetch>> items(n_members(p));
        std::vector<std::vector<Want>> wants(n_members(p));
        for (int x = 0; x < 2; x++) {
            lo[x] = g[x] + cnt.stop - (cnt.stop ? 1 : 0);
            const uint64_t hi = std::min<uint64_t>(st[x].len(), g[x] + cnt.stop + (want_rejoin ? win : 1));
            near[x].resize(hi > lo[x] ? hi - lo[x] : 0);
            for (uint64_t q = lo[x]; q < hi; q++) {
                const dvt_diverge_pos at = st[x].locate(q);
                const Held &h = held[x][at.shard - 1];
                items[h.m].push_back(OriginFetch{h.s->d_recs, (uint32_t)h.s->n_recs, at.row});
                wants[h.m].push_back(Want{x, (size_t)(q - lo[x])});
            }
        }
        std::vector<rv32::CycleRec> got;
        if (int rc = for_members(p, [&](size_t m, const Lane &c) {
                Engine &e = c.eng;
                DivergeMember &dm = run[m];
                if (items[m].empty()) return DVT_OK;
                if (items[m].size() > cap_items) return fail(c.err, DVT_ERR_DEVICE, "more records to gather than the windows hold");
                if (int rc = buffers(c, dm)) return rc;
                HIP_TRY(c.err, hipMemcpyAsync(dm.d_items, items[m].data(), items[m].size() * sizeof(OriginFetch), hipMemcpyHostToDevice, e.stream));
                HIP_TRY(c.err, dm.t_gather.begin(e.stream));
                HIP_TRY(c.err, launch_origin_gather(e.stream, dm.d_items, (uint32_t)items[m].size(), dm.d_recs));
                HIP_TRY(c.err, dm.t_gather.end(e.stream));
                got.resize(items[m].size());
                if (!e.download(got.data(), dm.d_recs, got.size() * sizeof(rv32::CycleRec))) return engine_fail(c.err, e);
                ms[2] += dm.t_gather.ms();
                for (size_t i = 0; i < got.size(); i++) near[wants[m][i].x][wants[m][i].i] = got[i];
                return DVT_OK;
            }))
            return rc;
    }
    auto rec = [&](int x, uint64_t q) -> const rv32::CycleRec * { return q >= lo[x] && q - lo[x] < near[x].size() ? &near[x][q - lo[x]] : nullptr; };
    diverge::finish(prog, statics, shapes, st[0], st[1], g[0], g[1], flags, window, K, cnt, rec,
                    [&](int x, uint64_t q, uint64_t n, std::vector<rv32::CycleRec> *out) {
                        for (uint64_t i = 0; i < n; i++)
                            if (const rv32::CycleRec *r = rec(x, q + i)) out->push_back(*r);
                    },
                    regs, summary);
    summary->launched_pairs = launched_pairs;
    const double total = ms_since(t0);
    summary->ms = (float)total;
    for (int i = 0; i < 3; i++) p->diverge_ms[i] = ms[i];
    p->diverge_ms[3] = std::max(0.0, total - ms[0] - ms[1] - ms[2]);
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

// the body of the three dvt_rv32_job_*_times
template <size_t N>
static int times_of(dvt_prover *p, double (dvt_prover::*ms)[N], double *out) {
    if (!p || !out) return DVT_ERR_INPUT;
    std::lock_guard<std::mutex> lk(p->mu);
    std::copy_n(p->*ms, N, out);
    return DVT_OK;
}

// the input check of the host-only entry points that take a shard size and the arrays of a report: why != nullptr or a
// log_shard_size out of range fails the call with *text in *err_text
static bool execute_input_error(uint32_t log_shard_size, const char *why, std::string *text, char **err_text) {
    if (log_shard_size && (log_shard_size < 4 || log_shard_size > 22)) *text = "log_shard_size must be 0 or 4..22";
    else if (!why) return false;
    if (err_text) *err_text = strdup(text->c_str());
    return true;
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
    const std::string overflow = sys_overflow();
    return execute_traced(
        elf, elf_len, stdin_bufs, nbuf, max_cycles, report, err_text, [&](const rv32::Program &prog) { t.reset(new prof::Tally(prog)); },
        [&](const rv32::Program &prog, const rv32::CycleRec *recs, size_t n, uint32_t last_succ) { prof::tally_records(prog, recs, n, last_succ, t.get()); },
        [&](const rv32::Program &prog, double ms) { return prof::emit(prog, *t, t->shards, ms, out) ? nullptr : overflow.c_str(); });
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

int dvt_rv32_job_calltree_times(dvt_prover *p, double out[3]) { return times_of(p, &dvt_prover::calltree_ms, out); }

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

int dvt_rv32_job_watch_times(dvt_prover *p, double out[4]) { return times_of(p, &dvt_prover::watch_ms, out); }

// host-only: the same rule (watch::scan_records) over execute_traced's shards
int dvt_execute_watch(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint64_t max_cycles, uint32_t log_shard_size,
                      const dvt_watch_query *queries, size_t n_queries, size_t cap_each, dvt_watch_hit *hits, uint64_t *totals,
                      dvt_watch_summary *summary, dvt_report *report, char **err_text) {
    if (err_text) *err_text = nullptr;
    if (!elf || (nbuf && !stdin_bufs) || !summary) return DVT_ERR_INPUT;
    std::string text;
    if (execute_input_error(log_shard_size, watch::input_error(queries, n_queries, cap_each, hits, totals, &text), &text, err_text)) return DVT_ERR_INPUT;
    std::unique_ptr<watch::Search> s;
    return execute_traced(
        elf, elf_len, stdin_bufs, nbuf, max_cycles, report, err_text,
        [&](const rv32::Program &prog) { s.reset(new watch::Search(prog, queries, n_queries, (uint32_t)cap_each)); },
        [&](const rv32::Program &prog, const rv32::CycleRec *recs, size_t n, uint32_t) { watch::scan_records(prog, recs, n, s->shards + 1, s.get()); },
        [&](const rv32::Program &prog, double ms) -> const char * {
            watch::emit(prog, *s, s->shards, ms, hits, totals, summary);
            return s->bad ? BAD_RECORD : nullptr;
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

int dvt_rv32_job_snapshot_times(dvt_prover *p, double out[3]) { return times_of(p, &dvt_prover::snap_ms, out); }

// host-only: the same rule (snap::Taker) over execute_traced's shards
int dvt_execute_snapshot(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint64_t max_cycles, uint32_t log_shard_size,
                         uint32_t shard, uint32_t row, const dvt_snap_range *ranges, size_t n_ranges, dvt_snap_cell regs[32], dvt_snap_cell *words,
                         size_t cap_words, dvt_snap_frame *frames, size_t cap_frames, dvt_snap_summary *summary, dvt_report *report,
                         char **err_text) {
    if (err_text) *err_text = nullptr;
    if (!elf || (nbuf && !stdin_bufs) || !summary) return DVT_ERR_INPUT;
    std::string text;
    snap::Ranges rg;
    if (execute_input_error(log_shard_size, snap::input_error(ranges, n_ranges, regs, words, cap_words, frames, cap_frames, &rg, &text), &text, err_text))
        return DVT_ERR_INPUT;
    std::unique_ptr<snap::Taker> t;
    return execute_traced(
        elf, elf_len, stdin_bufs, nbuf, max_cycles, report, err_text, [&](const rv32::Program &prog) { t.reset(new snap::Taker(prog, rg, shard, row)); },
        [&](const rv32::Program &prog, const rv32::CycleRec *recs, size_t n, uint32_t, uint32_t next_pc) {
            t->scan(prog, recs, n, (uint32_t)t->shard_n.size() + 1, next_pc);
        },
        [&](const rv32::Program &prog, double ms) -> const char * {
            t->emit(prog, ms, regs, words, frames, cap_frames, summary);
            return t->bad ? BAD_RECORD : nullptr;
        },
        log_shard_size ? log_shard_size : 21);
}

// ---- origins (origin.h)
int dvt_rv32_job_origin(dvt_prover *p, const dvt_pk *pk, dvt_job *job, uint32_t shard, uint32_t row, uint32_t what, uint32_t target, uint32_t flags,
                        uint32_t max_depth, dvt_origin_node *nodes, size_t cap_nodes, dvt_origin_edge *edges, size_t cap_edges,
                        dvt_origin_summary *summary) {
    if (!p || !pk || !job || !summary) return fail(p, DVT_ERR_INPUT, "null argument");
    std::string text;
    if (const char *why = origin::input_error(what, target, flags, max_depth, nodes, cap_nodes, edges, cap_edges, &text)) return fail(p, DVT_ERR_INPUT, "%s", why);
    if (int rc = rv32_key(p, pk)) return rc;
    Guard g(p); if (g.rc) return g.rc;
    return job_origin(p, pk, job, shard, row, what, target, flags, max_depth, nodes, cap_nodes, edges, cap_edges, summary);
}

int dvt_rv32_job_origin_times(dvt_prover *p, double out[3]) { return times_of(p, &dvt_prover::origin_ms, out); }

// host-only: the same search (origin::Search) over the records origin::Keeper keeps of execute_traced's shards
int dvt_execute_origin(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint64_t max_cycles, uint32_t log_shard_size,
                       uint32_t shard, uint32_t row, uint32_t what, uint32_t target, uint32_t flags, uint32_t max_depth, dvt_origin_node *nodes,
                       size_t cap_nodes, dvt_origin_edge *edges, size_t cap_edges, dvt_origin_summary *summary, dvt_report *report, char **err_text) {
    if (err_text) *err_text = nullptr;
    if (!elf || (nbuf && !stdin_bufs) || !summary) return DVT_ERR_INPUT;
    std::string text;
    if (execute_input_error(log_shard_size, origin::input_error(what, target, flags, max_depth, nodes, cap_nodes, edges, cap_edges, &text), &text, err_text))
        return DVT_ERR_INPUT;
    std::unique_ptr<origin::Keeper> k;
    bool bad = false;
    const int rc = execute_traced(
        elf, elf_len, stdin_bufs, nbuf, max_cycles, report, err_text, [&](const rv32::Program &prog) { k.reset(new origin::Keeper(prog, shard, row)); },
        [&](const rv32::Program &prog, const rv32::CycleRec *recs, size_t n, uint32_t) { k->scan(prog, recs, n, (uint32_t)k->shard_n.size() + 1); },
        [&](const rv32::Program &prog, double ms) -> const char * {
            if (k->too_many)
                return "more than 2^24 cycle records before the position: prepare the job and ask dvt_rv32_job_origin, which reads them on the GPU";
            if (k->bad) { bad = true; return BAD_RECORD; }
            const auto t1 = Clock::now();
            origin::Search search(prog, k->wst, k->sh, k->P, what, target, flags, max_depth, nodes, cap_nodes, edges, cap_edges);
            search.run([&](const std::vector<origin::Question> &qs, std::vector<origin::Found> *found) { return k->answer(prog, qs, found); });
            k->place(&search.s);
            search.s.ms = (float)(ms + ms_since(t1));
            *summary = search.s;
            return nullptr;
        },
        log_shard_size ? log_shard_size : 21);
    return bad && rc == DVT_ERR_UNSUPPORTED ? DVT_ERR_INPUT : rc;
}

// ---- uses (uses.h)
int dvt_rv32_job_uses(dvt_prover *p, const dvt_pk *pk, dvt_job *job, uint32_t shard, uint32_t row, uint32_t what, uint32_t target, uint32_t flags,
                      uint32_t max_depth, uint32_t fan, dvt_uses_node *nodes, size_t cap_nodes, dvt_uses_def *defs, size_t cap_defs,
                      dvt_uses_edge *edges, size_t cap_edges, dvt_uses_summary *summary) {
    if (!p || !pk || !job || !summary) return fail(p, DVT_ERR_INPUT, "null argument");
    std::string text;
    if (const char *why = uses::input_error(what, target, flags, max_depth, fan, nodes, cap_nodes, defs, cap_defs, edges, cap_edges, &text))
        return fail(p, DVT_ERR_INPUT, "%s", why);
    if (int rc = rv32_key(p, pk)) return rc;
    Guard g(p); if (g.rc) return g.rc;
    return job_uses(p, pk, job, shard, row, what, target, flags, max_depth, fan, nodes, cap_nodes, defs, cap_defs, edges, cap_edges, summary);
}

int dvt_rv32_job_uses_times(dvt_prover *p, double out[5]) { return times_of(p, &dvt_prover::uses_ms, out); }

// host-only: the same search (uses::Search) over the records uses::Keeper keeps of execute_traced's shards
int dvt_execute_uses(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint64_t max_cycles, uint32_t log_shard_size,
                     uint32_t shard, uint32_t row, uint32_t what, uint32_t target, uint32_t flags, uint32_t max_depth, uint32_t fan, dvt_uses_node *nodes,
                     size_t cap_nodes, dvt_uses_def *defs, size_t cap_defs, dvt_uses_edge *edges, size_t cap_edges, dvt_uses_summary *summary,
                     dvt_report *report, char **err_text) {
    if (err_text) *err_text = nullptr;
    if (!elf || (nbuf && !stdin_bufs) || !summary) return DVT_ERR_INPUT;
    std::string text;
    if (execute_input_error(log_shard_size, uses::input_error(what, target, flags, max_depth, fan, nodes, cap_nodes, defs, cap_defs, edges, cap_edges, &text),
                            &text, err_text))
        return DVT_ERR_INPUT;
    std::unique_ptr<uses::Keeper> k;
    bool bad = false;
    const int rc = execute_traced(
        elf, elf_len, stdin_bufs, nbuf, max_cycles, report, err_text, [&](const rv32::Program &prog) { k.reset(new uses::Keeper(prog, shard, row)); },
        [&](const rv32::Program &prog, const rv32::CycleRec *recs, size_t n, uint32_t) { k->scan(prog, recs, n, (uint32_t)k->shard_n.size() + 1); },
        [&](const rv32::Program &prog, double ms) -> const char * {
            if (k->too_many)
                return "more than 2^24 cycle records at and after the position: prepare the job and ask dvt_rv32_job_uses, which reads them on the GPU";
            if (k->bad) { bad = true; return BAD_RECORD; }
            const auto t1 = Clock::now();
            uses::Search search(prog, k->wst, k->sh, k->P, what, target, flags, max_depth, fan, nodes, cap_nodes, defs, cap_defs, edges, cap_edges);
            search.run([&](const std::vector<uses::Def> &qs, std::vector<uses::Found> *found) { return k->answer(prog, qs, found, flags, fan); });
            k->place(&search.s);
            search.s.ms = (float)(ms + ms_since(t1));
            *summary = search.s;
            return nullptr;
        },
        log_shard_size ? log_shard_size : 21);
    return bad && rc == DVT_ERR_UNSUPPORTED ? DVT_ERR_INPUT : rc;
}

// ---- divergence (diverge.h)
int dvt_rv32_job_diverge(dvt_prover *p, const dvt_pk *pk, dvt_job *job_a, dvt_job *job_b, dvt_diverge_pos start_a, dvt_diverge_pos start_b,
                         uint64_t max_pairs, uint32_t flags, uint32_t window, size_t cap_each, dvt_diverge_pair *first, dvt_diverge_pair *last,
                         dvt_diverge_reg regs[32], dvt_diverge_summary *summary) {
    if (!p || !pk || !job_a || !job_b || !summary) return fail(p, DVT_ERR_INPUT, "null argument");
    std::string text;
    if (const char *why = diverge::input_error(flags, window, cap_each, first, last, regs, &text)) return fail(p, DVT_ERR_INPUT, "%s", why);
    if (int rc = rv32_key(p, pk)) return rc;
    Guard g(p); if (g.rc) return g.rc;
    return job_diverge(p, pk, job_a, job_b, start_a, start_b, max_pairs, flags, window, (uint32_t)cap_each, first, last, regs, summary);
}

int dvt_rv32_job_diverge_times(dvt_prover *p, double out[4]) { return times_of(p, &dvt_prover::diverge_ms, out); }

// host-only: the same rule (diverge::compare) over the records diverge::Kept keeps of two runs of execute_traced
int dvt_execute_diverge(const uint8_t *elf, size_t elf_len, const uint8_t *stdin_a, size_t n_a, const uint8_t *stdin_b, size_t n_b, uint64_t max_cycles,
                        uint32_t log_shard_size, dvt_diverge_pos start_a, dvt_diverge_pos start_b, uint64_t max_pairs, uint32_t flags, uint32_t window,
                        size_t cap_each, dvt_diverge_pair *first, dvt_diverge_pair *last, dvt_diverge_reg regs[32], dvt_diverge_summary *summary,
                        dvt_report *report_a, dvt_report *report_b, char **err_text) {
    if (err_text) *err_text = nullptr;
    if (!elf || (n_a && !stdin_a) || (n_b && !stdin_b) || !summary) return DVT_ERR_INPUT;
    std::string text;
    if (execute_input_error(log_shard_size, diverge::input_error(flags, window, cap_each, first, last, regs, &text), &text, err_text)) return DVT_ERR_INPUT;
    const auto t0 = Clock::now();
    diverge::Kept kept[2];
    rv32::Program program;
    const dvt_buf bufs[2] = {{stdin_a, n_a}, {stdin_b, n_b}};
    dvt_report *reports[2] = {report_a, report_b};
    const dvt_diverge_pos starts[2] = {start_a, start_b};
    for (int x = 0; x < 2; x++) {
        char *why = nullptr;
        const int rc = execute_traced(
            elf, elf_len, &bufs[x], bufs[x].len ? 1 : 0, max_cycles, reports[x], &why, [&](const rv32::Program &prog) { if (!x) program = prog; },
            [&](const rv32::Program &, const rv32::CycleRec *recs, size_t n, uint32_t) { kept[x].scan(recs, n, starts[x]); },
            [&](const rv32::Program &, double) -> const char * { return nullptr; }, log_shard_size ? log_shard_size : 21);
        if (rc != DVT_OK && rc != DVT_ERR_GUEST) {   // (a guest that traps or exits non-zero ends its stream: no error here)
            if (err_text) *err_text = why;
            else free(why);
            return rc;
        }
        free(why);
        if (kept[x].too_many) {
            if (err_text) *err_text = strdup("more than 2^24 cycle records from a start on: prepare the jobs and ask dvt_rv32_job_diverge, which reads them on the GPU");
            return DVT_ERR_UNSUPPORTED;
        }
    }
    const uint64_t g[2] = {kept[0].st.global_of(start_a), kept[1].st.global_of(start_b)};
    diverge::compare(program, kept[0], kept[1], g[0], g[1], max_pairs, flags, window, (uint32_t)cap_each, first, last, regs, summary);
    summary->ms = (float)ms_since(t0);
    return DVT_OK;
}

}  // extern "C"
