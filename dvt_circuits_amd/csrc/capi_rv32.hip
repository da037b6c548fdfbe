// The rv32 boundary of the C ABI (include/dvt_prover.h): setup from an ELF, execute, the job (capi_job.h; the prepare pipeline and phase 1,
// the phase-2 pipeline on the prover lanes), prove, assemble, verify and the debug hooks.  (A job's inspectors: capi_inspect.hip; its reports: capi_report.hip.)
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <deque>
#include <map>

#include "capi_job.h"
#include "ntt_group.cuh"
#include "poseidon2_f64.cuh"
#include "sha256.h"

using namespace dvt;
static_assert(DVT_KEEP_NONE == KEEP_NONE && DVT_KEEP_TREE == KEEP_TREE && DVT_KEEP_FULL == KEEP_FULL, "the tiers of include/dvt_prover.h");

namespace {
std::vector<std::vector<uint8_t>> collect_stdin(const dvt_buf *bufs, size_t n) {
    std::vector<std::vector<uint8_t>> v(n);
    for (size_t i = 0; i < n; i++)
        if (bufs[i].len) v[i].assign(bufs[i].data, bufs[i].data + bufs[i].len);
    return v;
}
uint8_t *dup_bytes(const std::vector<uint8_t> &v, size_t *len) {
    uint8_t *b = (uint8_t *)malloc(v.size() + 1);
    if (b && !v.empty()) memcpy(b, v.data(), v.size());
    if (len) *len = v.size();
    return b;
}
// LogUp challenges common to all shards: transcript over the key and every shard's header
PermChallenges global_challenges(const VerifyingKey &vk, const uint32_t *headers, size_t n) {
    Challenger g;
    g.observe(vk.prep_root);
    g.observe_u32((uint32_t)n);
    for (size_t i = 0; i < n; i++) {
        const uint32_t *h = headers + i * HEADER_WORDS;
        for (uint32_t k = 0; k < 8; k++) g.observe(Fp::from_canonical(h[k]));
        g.observe_u32(N_PUB);
        for (uint32_t k = 0; k < N_PUB; k++) g.observe(Fp::from_canonical(h[8 + k] % P));
    }
    PermChallenges c;
    c.alpha = g.sample_ext();
    c.beta = g.sample_ext();
    return c;
}
// SP1's committed-value digest: word k = little-endian u32 of bytes 4k..4k+3 of SHA-256(public-value bytes)
// (an empty stream commits 42c4b0e3 141cfc98 ... = sha256("") read as LE words)
void pv_digest_words(const std::vector<uint8_t> &pv, uint32_t out[8]) {
    uint8_t dg[32];
    sha256(pv.data(), pv.size(), dg);
    for (int k = 0; k < 8; k++) out[k] = dg[4 * k] | (dg[4 * k + 1] << 8) | (dg[4 * k + 2] << 16) | ((uint32_t)dg[4 * k + 3] << 24);
}
}  // namespace

int dvt::same_members(dvt_prover *p, const dvt_pk *pk, const dvt_job *j) {
    const size_t G = n_members(p);
    if ((pk && pk->dev.size() != G) || (j && j->parts.size() != G)) return fail(p, DVT_ERR_INPUT, "proving key or job of a handle with other devices");
    return DVT_OK;
}

// (no phase-1 worker and no phase-2 pipeline runs: buffers go back to the pools only after every lane is done)
// Every buffer returns to the pool of the member and lane it came from: what a shard uploaded to lane 0's, what phase 1 kept
// (K0 output; LDEs and tree through the cache) to the pool of the lane that committed the shard, the working buffers to
// their lane's.  On a handle with fewer members than the one that made the job (include/dvt_prover.h) the other members'
// buffers cannot be reached and stay allocated.
static void job_release(dvt_prover *p, dvt_job *j) {
    if (!j) return;
    for (size_t m = std::min(j->parts.size(), n_members(p)); m-- > 0;) {
        (void)turn_to(p, m);
        Member &mem = member(p, m);
        for (auto &s : j->parts[m].shards) {
            mem.eng.pool.free(s.d_recs);
            for (auto &d : s.d_aux) mem.eng.pool.free(d);
            if (s.d_cpu || s.d_byte || s.d_prog)
                for (uint32_t *d : {s.d_cpu, s.d_byte, s.d_prog}) lane_engine(mem, s.lane).pool.free(d);
            s.cache.release();
        }
        for (int k = 0; k < MAX_LANES; k++) {
            auto &w = j->parts[m].work[k];
            if (w.d_cpu || w.d_byte || w.d_prog)
                for (uint32_t *d : {w.d_cpu, w.d_byte, w.d_prog}) lane_engine(mem, k).pool.free(d);
        }
    }
    delete j;
}

int dvt::shard_traces(const Lane &c, const DeviceKey &key, dvt_job *j, ShardJob &s, std::vector<ChipTrace> *traces, bool reuse) {
    hipStream_t st = c.eng.stream;
    JobPart::Work &w = j->parts[c.mem.index].work[c.k];
    const MachineDesc *m = machine_rv32();
    if (!s.d_cpu && (!w.d_cpu || w.log_cpu < s.log_n[RV32_CHIP_CPU])) {   // working buffers, sized for the largest shard seen
        HIP_TRY(c.err, hipStreamSynchronize(st));
        for (uint32_t **d : {&w.d_cpu, &w.d_byte, &w.d_prog}) { c.eng.pool.free(*d); *d = nullptr; }
        w.log_cpu = s.log_n[RV32_CHIP_CPU];
        HIP_TRY(c.err, c.eng.pool.alloc(&w.d_cpu, ((size_t)RV32_CPU_MAIN_W << w.log_cpu) * 4));
        HIP_TRY(c.err, c.eng.pool.alloc(&w.d_byte, j->byte_words * 4));
        HIP_TRY(c.err, c.eng.pool.alloc(&w.d_prog, j->prog_words * 4));
    }
    uint32_t *cpu = s.d_cpu ? s.d_cpu : w.d_cpu, *byte = s.d_cpu ? s.d_byte : w.d_byte, *prog = s.d_cpu ? s.d_prog : w.d_prog;
    if (!(reuse && s.d_cpu && s.traces_valid)) {
        bool ok = hipMemcpyAsync(byte, s.d_aux[RV32_CHIP_BYTE], j->byte_words * 4, hipMemcpyDeviceToDevice, st) == hipSuccess &&
                  hipMemcpyAsync(prog, s.d_aux[RV32_CHIP_PROGRAM], j->prog_words * 4, hipMemcpyDeviceToDevice, st) == hipSuccess &&
                  rv32::launch_k0_cpu_rows(st, s.d_recs, s.n_recs, s.index, s.next_pc, key.d_instrs, key.d_prog_row, cpu, s.log_n[RV32_CHIP_CPU], byte, prog) == hipSuccess &&
                  launch_to_internal(st, byte, j->byte_words) == hipSuccess && launch_to_internal(st, prog, j->prog_words) == hipSuccess;
        if (!ok) return fail(c.err, DVT_ERR_DEVICE, "trace generation (K0) failed: %s", hipGetErrorString(hipGetLastError()));
        s.traces_valid = s.d_cpu != nullptr;
    }
    traces->clear();
    for (int c = 0; c < m->n_chips; c++) {
        if (!s.present[c]) continue;
        const uint32_t *ptr = c == RV32_CHIP_CPU ? cpu : c == RV32_CHIP_BYTE ? byte : c == RV32_CHIP_PROGRAM ? prog : s.d_aux[c];
        traces->push_back({c, s.log_n[c], ptr});
    }
    return DVT_OK;
}

// Committers on one physical device (the phase-1 lanes of a member, the members of a handle that share the device) read the
// same free bytes: the first phase 1 of a shard, which asks how much is free and then allocates what it keeps, takes
// turns between them.  The turn covers the question and every allocation of the commit and ends before the commit's first
// LDE kernel is launched (commit_main_root), so the kernels of two committers overlap.  While a member commits on several
// lanes, every use of its pools is made under the turn, the feeder's uploads into lane 0's pool included: that is what
// keeps a pool single-threaded.  A shard that is committed again outside a prepare has its buffers and does not wait; nor
// does a one-lane member alone on its device.
static std::mutex &device_turn(int dev) {
    static std::mutex mu[64];
    return mu[dev & 63];
}

// What the fast pass of a prepare has found so far: the shards of the execution counted as their first cycle is reached, and
// whether the count is final.  The fast-pass thread advances it; the committers read it at the admission of a shard.
struct ShardCount {
    std::atomic<size_t> found{0};
    std::atomic<bool> final{false};
};

// the bytes a shard holds in HBM in each tier, and what its upload allocated (keep_plan.h: T, F and L - T)
static size_t shard_tree_bytes(const ShardJob &s) {
    uint32_t max_log_n = 0;
    for (int c = 0; c < rv32::N_CHIPS; c++)
        if (s.present[c]) max_log_n = std::max(max_log_n, s.log_n[c]);
    return (((size_t)2 << (max_log_n + 1)) - 1) * 32;
}
static size_t shard_k0_bytes(const dvt_job *j, const ShardJob &s) { return (((size_t)RV32_CPU_MAIN_W << s.log_n[RV32_CHIP_CPU]) + j->byte_words + j->prog_words) * 4; }
static size_t shard_lde_bytes(const ShardJob &s) {
    size_t n = 0;
    for (int c = 0; c < rv32::N_CHIPS; c++)
        if (s.present[c]) n += ((size_t)machine_rv32()->chips[c].main_w << s.log_n[c]) * 8;
    return n;
}
static size_t shard_upload_bytes(const ShardJob &s) {
    size_t n = s.n_recs * sizeof(rv32::CycleRec);
    for (int c = 0; c < rv32::N_CHIPS; c++)
        if (s.present[c] && c != RV32_CHIP_CPU) n += ((size_t)machine_rv32()->chips[c].main_w << s.log_n[c]) * 4;
    return n;
}

// phase 1 of a shard: K0 + K1..K3 of the main traces -> header.  `concurrent`: other threads of this member commit or upload
// meanwhile (the phase-1 lanes of a prepare).  `count`: the executor's shard count inside a prepare (what is still to come
// on this device enters the admission, keep_plan.h); nullptr outside one: nothing is to come and the count is known.
static int shard_commit(const Lane &c, const DeviceKey &key, dvt_job *j, ShardJob &s, bool concurrent = false, const ShardCount *count = nullptr) {
    dvt_prover *p = c.p;
    Member &mem = c.mem;
    std::vector<ChipTrace> traces;
    const bool time_stages = getenv("DVT_TIME_PREPARE") != nullptr;
    const auto t0 = Clock::now();
    auto lap = [&](const char *what) {
        if (time_stages) fprintf(stderr, "[commit] %s at %.2f ms (pool misses so far %zu)\n", what, ms_since(t0), c.eng.pool.misses);
    };
    // keep the phase-1 results in HBM while they fit (about 3 GB per 2^21-cycle shard); otherwise the tree alone
    // ("keep_phase1": 2) or nothing, and phase 2 recomputes the rest
    std::unique_lock<std::mutex> turn;
    if (concurrent || (mem.shares_device && p->keep_phase1 && !s.cache.tree)) turn = std::unique_lock<std::mutex>(device_turn(c.eng.device));
    size_t free_b = 0, total_b = 0;
    if (p->keep_phase1 && !s.cache.tree) { (void)hipMemGetInfo(&free_b, &total_b); free_b += c.eng.pool.cached_bytes; }   // (only the first commit of a shard asks)
    // the further lanes' arenas are not there yet on the first job: leave room for them (the largest arena of this member's
    // lanes is the measure of one), so that the kept caches do not take what another lane's working set then cannot get
    // (and for the lanes of the members that share this device, whose phase 1 waits for its turn meanwhile)
    size_t lane_room = 0, one_arena = mem.eng.arena.cap;
    for (auto &e : mem.more)
        if (e) one_arena = std::max(one_arena, e->arena.cap);
    auto room_of = [&](const Member &q) {
        for (int k = 0; k < p->lanes; k++) {
            if (&q == &mem && k == c.k) continue;
            const size_t have = k == 0 ? q.eng.arena.cap : q.more[k - 1] ? q.more[k - 1]->arena.cap : 0;
            if (one_arena > have) lane_room += one_arena - have;
        }
    };
    room_of(mem);
    if (turn.owns_lock())
        for (auto &q : p->members)
            if (q.get() != &mem && q->eng.device == c.eng.device) room_of(*q);
    // The tier (keep_plan.h), decided and allocated for under the turn.  The tallies of the device (shards committed in this
    // prepare, shards kept in full in this job) are shared by the members on it and written under the same turn.
    dvt_job::DeviceTally &tally = j->tally[c.eng.device & 63];
    int tier = s.cache.tier();   // (a shard that has a cache keeps its tier: no question asked, as before)
    if (p->keep_phase1 && !s.cache.tree) {
        KeepPlanIn in;
        in.mode = p->keep_phase1;
        in.free_b = free_b; in.total_b = total_b;
        in.reserve = ((size_t)24 << 30) + lane_room;
        in.tree_b = shard_tree_bytes(s);
        in.full_b = in.tree_b + shard_lde_bytes(s) + shard_k0_bytes(j, s);
        in.later_b = in.tree_b + shard_upload_bytes(s);
        if (count) {   // what the fast pass has found so far for the members on this device, less what they have committed
            in.count_known = count->final.load(std::memory_order_acquire);
            const size_t found = count->found.load(std::memory_order_acquire);
            size_t theirs = 0;
            for (auto &q : p->members) {
                if (q->eng.device != c.eng.device) continue;
                const JobPart &part = j->parts[q->index];
                if (found > part.first) theirs += (found - part.first + part.stride - 1) / part.stride;
            }
            in.remaining = theirs > tally.committed + 1 ? theirs - tally.committed - 1 : 0;
        }
        in.full_cap = p->keep_full_max;
        in.full_kept = tally.full;
        tier = keep_plan(in);
        if (tier == KEEP_FULL) tally.full++;
        if (count) tally.committed++;
    }
    if (time_stages) {
        char what[64];
        snprintf(what, sizeof what, "memory asked (tier %s)", tier == KEEP_FULL ? "FULL" : tier == KEEP_TREE ? "TREE" : "NONE");
        lap(what);
    }
    MainCache *keep = tier != KEEP_NONE ? &s.cache : nullptr;
    if (tier == KEEP_FULL && !s.d_cpu) {
        DevPool &pool = c.eng.pool;
        s.lane = c.k;
        bool ok = pool.alloc(&s.d_cpu, ((size_t)RV32_CPU_MAIN_W << s.log_n[RV32_CHIP_CPU]) * 4) == hipSuccess && pool.alloc(&s.d_byte, j->byte_words * 4) == hipSuccess &&
                  pool.alloc(&s.d_prog, j->prog_words * 4) == hipSuccess;
        if (!ok) {  // not fatal: fall back to the shared working buffers
            (void)hipGetLastError();
            for (uint32_t **d : {&s.d_cpu, &s.d_byte, &s.d_prog}) { pool.free(*d); *d = nullptr; }
        }
    }
    lap("trace buffers");
    int rc = shard_traces(c, key, j, s, &traces, false);
    if (rc) return rc;
    lap("K0 launched");
    Digest root;
    if (!c.eng.commit_main_root(key.key, traces, &root, keep, &turn, tier)) return engine_fail(c.err, c.eng);
    lap("main root");
    for (int k = 0; k < 8; k++) s.header[k] = root.d[k].canonical();
    for (uint32_t k = 0; k < N_PUB; k++) s.header[8 + k] = s.pubs[k].canonical();
    s.header_valid = true;
    s.kept = tier;
    return DVT_OK;
}

// phase 2 of a shard: K0..K9 with the common challenges -> shard proof words
// (on any lane: the shard's phase-1 buffers came from the pool of the lane that committed it and are only read here)
static int shard_prove(const Lane &c, const DeviceKey &key, dvt_job *j, ShardJob &s, const PermChallenges &gc, std::vector<uint32_t> *words) {
    std::vector<ChipTrace> traces;
    int rc = shard_traces(c, key, j, s, &traces, s.cache.valid);
    if (rc) return rc;
    ShardProof sp;
    bool ok = c.eng.prove_shard(key.key, traces, s.pubs, c.p->cfg, &sp, &gc, &s.cache);
    (void)hipStreamSynchronize(c.eng.stream);
    s.cache.valid = false;  // the buffers stay for the next commit of this shard (released with the job)
    s.traces_valid = false;
    s.header_valid = false;
    if (!ok) return engine_fail(c.err, c.eng);
    WordWriter w;
    w.w.reserve((size_t)1 << 20);  // a shard proof is about 2.4 MB at 100 queries
    write_shard_proof(w, sp);
    *words = std::move(w.w);
    return DVT_OK;
}

// ------------------------------------------------------------------ the prepare pipeline
// One sequential FAST pass of the guest finds the shard boundaries and snapshots the machine there; trace-mode
// executor threads re-run the owned shards from the snapshots into pinned buffers and build the small auxiliary
// traces; the calling thread uploads shard i+1 on the copy stream while the GPU runs phase 1 (K0 + K1..K3 of the main
// traces) of shard i.  (reference src/main.rs:461-466: prove() executes AND proves in one call.)
namespace {
struct ReadyShard {
    rv32::CycleRec *buf = nullptr;
    rv32::ShardMeta meta{};
    rv32::HostTraces aux;
    rv32::BigOpBatches big;   // the precompile calls of the shard: their chips' rows are built on the GPU
    std::string err;
    bool unsupported = false;
};
// what the fast pass found about the whole execution
struct FastPass {
    size_t n_total = 0;
    std::vector<rv32::MemInitRow> mem_rows;
    int exit_code = -1;
    bool halted = false, unsupported = false;
    uint64_t cycles = 0;
    std::string error, unsupported_what;
    std::vector<uint8_t> public_values;
    uint32_t committed[8] = {}, committed_mask = 0;
};

// The executor side of a prepare, host threads only (no HIP calls): the fast pass and the trace-mode workers.  It hands
// out the ready shard at a position and takes pinned buffers back; finish() (or the destructor) aborts and joins the threads.
struct Executor {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::pair<size_t, rv32::Snapshot>> snaps;
    bool snaps_closed = false, fast_done = false;
    std::atomic<bool> abort{false};   // (also read outside the mutex by a worker that is about to build auxiliary traces)
    std::vector<rv32::CycleRec *> free_bufs;
    std::map<size_t, ReadyShard> ready;
    FastPass fast;
    ShardCount count;   // the shards the fast pass has reached (the admission of phase 1 reads it)
    rv32::CurveLog curve_log;
    std::vector<std::thread> threads;   // the fast pass, then the workers

    // the threads run the guest over `inputs`, which must outlive the executor; they start on the pinned buffers `bufs`
    Executor(const dvt_pk *pk, const std::vector<std::vector<uint8_t>> &inputs, uint32_t log_shard, uint64_t max_cycles, size_t first,
             size_t stride, unsigned n_workers, const std::vector<rv32::CycleRec *> &bufs, bool time_stages)
        : free_bufs(bufs) {
        threads.emplace_back([=, &inputs] {
            rv32::Vm vm(pk->prog, &inputs, log_shard);
            vm.curve_log = &curve_log;
            struct Close { rv32::CurveLog &l; ~Close() { l.closed.store(true, std::memory_order_release); } } close_log{curve_log};
            size_t pos = 0;
            for (;; pos++) {
                count.found.store(pos + 1, std::memory_order_release);
                if (pos % stride == first) {
                    rv32::Snapshot snap = vm.snapshot();
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return snaps.size() < 2 * (size_t)n_workers + 2 || abort; });
                    if (abort) break;
                    snaps.emplace_back(pos, std::move(snap));
                    cv.notify_all();
                }
                vm.run_shard(false, nullptr, max_cycles);
                if (!vm.error.empty() || vm.halted || !vm.next_shard()) break;
            }
            std::vector<rv32::MemInitRow> rows;
            if (vm.halted) rows = vm.mem_rows();
            count.found.store(pos + 1, std::memory_order_release);
            count.final.store(true, std::memory_order_release);
            std::lock_guard<std::mutex> lk(mu);
            fast.n_total = pos + 1;
            fast.mem_rows = std::move(rows);
            fast.exit_code = vm.exit_code; fast.halted = vm.halted; fast.cycles = vm.cycles; fast.error = vm.error;
            fast.unsupported = vm.unsupported; fast.unsupported_what = vm.unsupported_what;
            fast.public_values = std::move(vm.public_values);
            for (int k = 0; k < 8; k++) fast.committed[k] = vm.committed[k];
            fast.committed_mask = vm.committed_mask;
            fast_done = snaps_closed = true;
            cv.notify_all();
        });
        for (unsigned w = 0; w < n_workers; w++) threads.emplace_back([=, &inputs] {
            for (;;) {
                rv32::CycleRec *buf = nullptr;
                size_t pos = 0;
                rv32::Snapshot snap;
                {
                    // a buffer first, then the OLDEST snapshot: buffers are handed out in shard order, so the shard the GPU
                    // thread waits for always has one
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return abort || ((!snaps.empty() || snaps_closed) && (!free_bufs.empty() || snaps.empty())); });
                    if (abort || snaps.empty()) return;
                    buf = free_bufs.back();
                    free_bufs.pop_back();
                    pos = snaps.front().first;
                    snap = std::move(snaps.front().second);
                    snaps.pop_front();
                    cv.notify_all();
                }
                ReadyShard r;
                r.buf = buf;
                const auto tw0 = Clock::now();
                {
                    rv32::Vm vm(pk->prog, &inputs, log_shard, snap);
                    vm.curve_log = &curve_log;
                    snap = rv32::Snapshot();
                    rv32::ShardOut so;
                    so.recs = buf;
                    vm.run_shard(true, &so, max_cycles);
                    const auto tw1 = Clock::now();
                    r.meta = rv32::ShardMeta{so.index, so.start_pc, so.next_pc, so.n_recs};
                    if (!vm.error.empty()) { r.err = vm.error; r.unsupported = vm.unsupported; }
                    else {
                        const std::vector<rv32::MemInitRow> *rows = nullptr;
                        int ec = 0;
                        if (vm.halted) {   // the last shard carries the mem_init table: final memory state of the fast pass
                            std::unique_lock<std::mutex> lk(mu);
                            cv.wait(lk, [&] { return fast_done || abort; });
                            rows = &fast.mem_rows;
                            ec = fast.exit_code;
                        }
                        std::string e;
                        const auto tw2 = Clock::now();
                        if (!abort && !rv32::build_aux_host(r.meta, so.alu, so.sha_ext, so.sha_cmp, so.big, rows, ec, pk->prep, &r.aux, &e, &r.big)) r.err = e;
                        if (time_stages) {
                            auto ms = [](Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
                            fprintf(stderr, "[prepare] shard %u: traced execution %.2f ms, wait for the fast pass %.2f ms, auxiliary traces %.2f ms\n", so.index, ms(tw0, tw1), ms(tw1, tw2),
                                    ms(tw2, Clock::now()));
                        }
                    }
                }
                std::lock_guard<std::mutex> lk(mu);
                ready[pos] = std::move(r);
                cv.notify_all();
            }
        });
    }
    ~Executor() { finish(); }

    // the ready shard at position pos; false when the execution has no shard there or the fast pass stopped on an error
    bool take(size_t pos, ReadyShard *r, double *waited) {
        std::unique_lock<std::mutex> lk(mu);
        const auto t0 = Clock::now();
        cv.wait(lk, [&] { return ready.count(pos) || (fast_done && pos >= fast.n_total) || (fast_done && !fast.error.empty()) || abort; });
        *waited += std::chrono::duration<double>(Clock::now() - t0).count();
        auto it = ready.find(pos);
        if (it == ready.end()) return false;
        *r = std::move(it->second);
        ready.erase(it);
        return true;
    }
    void give_back(rv32::CycleRec *b) {
        std::lock_guard<std::mutex> lk(mu);
        free_bufs.push_back(b);
        cv.notify_all();
    }
    // a member's phase 1 failed: the threads stop, and the other members' take() returns false for what is not ready
    void cancel() {
        std::lock_guard<std::mutex> lk(mu);
        abort = true;
        cv.notify_all();
    }
    // stops and joins the threads: what the fast pass found is final
    FastPass &finish() {
        {
            std::lock_guard<std::mutex> lk(mu);
            abort = true;   // (everything is done on the success path; on errors this stops the threads)
            cv.notify_all();
        }
        for (auto &t : threads)
            if (t.joinable()) t.join();
        return fast;
    }
};

// what a chip of a ready shard uploads: its calls / events when K0 of the chip runs on the GPU (true), else the rows the
// executor thread built (false)
bool events_of(const ReadyShard &r, int c, const void **src, size_t *bytes, size_t *count = nullptr) {
    auto is = [&](const void *data, size_t n, size_t each) {
        *src = data; *bytes = n * each;
        if (count) *count = n;
        return true;
    };
    if (!r.big.ev[c].empty()) return is(r.big.ev[c].data(), r.big.ev[c].size(), sizeof(rv32::BigOpEvent));
    if (c == RV32_CHIP_SHIFT && !r.big.shifts.empty()) return is(r.big.shifts.data(), r.big.shifts.size(), sizeof(rv32::AluEvent));
    if (c == RV32_CHIP_MULDIV && !r.big.muldivs.empty()) return is(r.big.muldivs.data(), r.big.muldivs.size(), sizeof(rv32::AluEvent));
    if (c == RV32_CHIP_SHA_EXTEND && !r.big.sha_ext.empty()) return is(r.big.sha_ext.data(), r.big.sha_ext.size(), sizeof(rv32::ShaExtEvent));
    if (c == RV32_CHIP_SHA_COMPRESS && !r.big.sha_cmp.empty()) return is(r.big.sha_cmp.data(), r.big.sha_cmp.size(), sizeof(rv32::ShaCmpEvent));
    if (c == RV32_CHIP_MEM_INIT && r.big.mem_rows && !r.big.mem_rows->empty()) return is(r.big.mem_rows->data(), r.big.mem_rows->size(), sizeof(rv32::MemInitRow));
    return false;
}
}  // namespace

// Upload of one ready shard into the shard s of the job: records on the copy stream (pinned source, overlaps the compute
// streams; `ev` is recorded after them), the small auxiliary traces and the K0 launches of the precompile chips on `aux`.
// With one phase-1 lane `aux` is the lane's compute stream.  The feeder of several phase-1 lanes passes the copy stream,
// so that the wait at the end (the staging buffer is reused by the next shard, the error words are read) is for this upload
// alone and no committing lane's stream is drained; it allocates from lane 0's pool under the device's turn (device_turn).
static int upload_shard(const Lane &lane, ReadyShard &r, ShardJob &s, hipEvent_t ev, hipStream_t aux, bool feeder) {
    Member &mem = lane.mem;
    Engine &e = lane.eng;
    const MachineDesc *m = machine_rv32();
    s.index = r.meta.index; s.n_recs = r.meta.n_recs; s.next_pc = r.meta.next_pc;
    for (int c = 0; c < m->n_chips; c++) { s.log_n[c] = r.aux.log_n[c]; s.present[c] = r.aux.present[c]; }
    uint32_t *d_calls[rv32::N_CHIPS] = {};   // per precompile chip: [error word, padding to 16 bytes, the calls]
    size_t stage_bytes = 0;
    {
        std::unique_lock<std::mutex> turn;
        if (feeder) turn = std::unique_lock<std::mutex>(device_turn(e.device));
        HIP_TRY(lane.err, e.pool.alloc(&s.d_recs, s.n_recs * sizeof(rv32::CycleRec)));
        for (int c = 0; c < m->n_chips; c++) {
            if (c == RV32_CHIP_CPU || !s.present[c]) continue;
            const void *src = nullptr;
            size_t bytes = 0;
            if (events_of(r, c, &src, &bytes)) {
                HIP_TRY(lane.err, e.pool.alloc(&s.d_aux[c], ((size_t)m->chips[c].main_w << s.log_n[c]) * 4));
                HIP_TRY(lane.err, e.pool.alloc(&d_calls[c], 16 + bytes));
            } else {
                bytes = r.aux.main[c].size() * 4;
                HIP_TRY(lane.err, e.pool.alloc(&s.d_aux[c], bytes));
            }
            stage_bytes += (bytes + 255) & ~(size_t)255;
        }
    }
    HIP_TRY(lane.err, hipMemcpyAsync(s.d_recs, r.buf, s.n_recs * sizeof(rv32::CycleRec), hipMemcpyHostToDevice, mem.copy_stream));
    HIP_TRY(lane.err, hipEventRecord(ev, mem.copy_stream));
    if (stage_bytes > mem.aux_pinned_bytes) {
        HIP_TRY(lane.err, hipStreamSynchronize(aux));
        if (mem.aux_pinned) HIP_TRY(lane.err, hipHostFree(mem.aux_pinned));
        mem.aux_pinned = nullptr; mem.aux_pinned_bytes = 0;
        HIP_TRY(lane.err, hipHostMalloc(&mem.aux_pinned, stage_bytes + stage_bytes / 4));
        mem.aux_pinned_bytes = stage_bytes + stage_bytes / 4;
    }
    size_t stage_at = 0;
    auto staged = [&](const void *src, size_t bytes) -> const void * {
        uint8_t *dst = mem.aux_pinned + stage_at;
        memcpy(dst, src, bytes);
        stage_at += (bytes + 255) & ~(size_t)255;
        return dst;
    };
    size_t n_events[rv32::N_CHIPS] = {};
    for (int c = 0; c < m->n_chips; c++) {
        if (c == RV32_CHIP_CPU || !s.present[c]) continue;
        const void *src = nullptr;
        size_t bytes = 0;
        if (events_of(r, c, &src, &bytes, &n_events[c])) {   // K0 of this chip on the GPU (after the byte counts are in): [error word, padding to 16 bytes, the events]
            const size_t words = (size_t)m->chips[c].main_w << s.log_n[c];
            HIP_TRY(lane.err, hipMemsetAsync(s.d_aux[c], 0, words * 4, aux));
            HIP_TRY(lane.err, hipMemsetAsync(d_calls[c], 0, 16, aux));
            HIP_TRY(lane.err, hipMemcpyAsync(d_calls[c] + 4, staged(src, bytes), bytes, hipMemcpyHostToDevice, aux));
            continue;
        }
        size_t words = r.aux.main[c].size();
        HIP_TRY(lane.err, hipMemcpyAsync(s.d_aux[c], staged(r.aux.main[c].data(), words * 4), words * 4, hipMemcpyHostToDevice, aux));
        // byte / program multiplicities stay plain integers until K0 has added the cpu rows' lookups
        if (c != RV32_CHIP_BYTE && c != RV32_CHIP_PROGRAM) HIP_TRY(lane.err, launch_to_internal(aux, s.d_aux[c], words));
    }
    for (int c = 0; c < m->n_chips; c++) {
        if (!d_calls[c]) continue;
        const size_t words = (size_t)m->chips[c].main_w << s.log_n[c];
        s.device_rows |= 1u << c;
        uint32_t *byte = s.d_aux[RV32_CHIP_BYTE];
        if (c == RV32_CHIP_SHIFT) {   // (these five write Montgomery words themselves)
            HIP_TRY(lane.err, rv32::launch_k0_shift_rows(aux, reinterpret_cast<const rv32::AluEvent *>(d_calls[c] + 4), n_events[c], s.d_aux[c], s.log_n[c], byte));
        } else if (c == RV32_CHIP_MEM_INIT) {
            HIP_TRY(lane.err, rv32::launch_k0_mem_init_rows(aux, reinterpret_cast<const rv32::MemInitRow *>(d_calls[c] + 4), n_events[c], s.d_aux[c], s.log_n[c], byte));
        } else if (c == RV32_CHIP_MULDIV) {
            HIP_TRY(lane.err, rv32::launch_k0_muldiv_rows(aux, reinterpret_cast<const rv32::AluEvent *>(d_calls[c] + 4), n_events[c], s.d_aux[c], s.log_n[c], byte));
        } else if (c == RV32_CHIP_SHA_EXTEND) {
            HIP_TRY(lane.err, rv32::launch_k0_sha_extend_rows(aux, reinterpret_cast<const rv32::ShaExtEvent *>(d_calls[c] + 4), n_events[c], s.index, s.d_aux[c], s.log_n[c], byte));
        } else if (c == RV32_CHIP_SHA_COMPRESS) {
            HIP_TRY(lane.err, rv32::launch_k0_sha_compress_rows(aux, reinterpret_cast<const rv32::ShaCmpEvent *>(d_calls[c] + 4), n_events[c], s.index, s.d_aux[c], s.log_n[c], byte));
        } else {
            HIP_TRY(lane.err, rv32::launch_k0_bigop_rows(aux, c, reinterpret_cast<const rv32::BigOpEvent *>(d_calls[c] + 4), (uint32_t)n_events[c], s.index,
                                                       s.d_aux[c], s.log_n[c], s.d_aux[RV32_CHIP_BYTE], d_calls[c]));
            HIP_TRY(lane.err, launch_to_internal(aux, s.d_aux[c], words));
        }
    }
    HIP_TRY(lane.err, hipStreamSynchronize(aux));   // (the staging buffer is reused by the next shard; the error words below)
    int rc = DVT_OK;
    for (int c = 0; c < m->n_chips; c++) {
        if (!d_calls[c]) continue;
        uint32_t row_err = 0;
        const hipError_t he = rc ? hipSuccess : hipMemcpy(&row_err, d_calls[c], 4, hipMemcpyDeviceToHost);
        {
            std::unique_lock<std::mutex> turn;
            if (feeder) turn = std::unique_lock<std::mutex>(device_turn(e.device));
            e.pool.free(d_calls[c]);
        }
        if (rc) continue;
        if (he != hipSuccess) rc = fail(lane.err, DVT_ERR_DEVICE, "reading the K0 error word: %s", hipGetErrorString(he));
        else if (row_err) rc = fail(lane.err, DVT_ERR_DEVICE, "K0 of chip %s: %s", m->chips[c].name, rv32::bigop_row_error_text(row_err));
    }
    if (rc) return rc;
    for (auto x : r.aux.pubs) s.pubs.push_back(Fp::from_canonical(x));
    return DVT_OK;
}

// lane k of a member (k >= 1), made when it is first needed
static int ensure_lane(Member &mem, int k, std::string &err) {
    if (mem.more[k - 1]) return DVT_OK;
    std::unique_ptr<Engine> e(new Engine());
    e->profile = false;
    e->parts_parallel_log = mem.eng.parts_parallel_log;
    const hipError_t r = e->init(mem.eng.device);
    if (r != hipSuccess) {
        e->shutdown();
        return fail(err, DVT_ERR_DEVICE, "prover lane %d: %s", k, hipGetErrorString(r));
    }
    mem.more[k - 1] = std::move(e);
    return DVT_OK;
}

// ------------------------------------------------------------------ phase 1 on several lanes ("phase1_lanes" > 1)
// The calling thread is the feeder: it takes the shards from the executor in execution order, uploads each (upload_shard on
// the copy stream) and queues it.  Up to phase1_lanes workers, one per lane and each on a thread of its own, take the next
// queued shard and run shard_commit on their lane's engine, so the LDE of one shard runs under the leaf hashing of another.
// Lane k's worker (and, for k >= 1, its engine) is started when a shard is queued and no started worker is free: a job of
// one shard starts lane 0 only.  The feeder uploads the next shard once the queue is empty, so a member has at most
// phase1_lanes shards in commit and one uploaded or in upload: that many pinned record buffers are out of the executor's
// hands (job_prepare).  A buffer goes back when the commit that read it is done.
namespace {
struct Phase1Lanes {
    struct Item { ShardJob *s; size_t pos; rv32::CycleRec *buf; };
    struct Worker {   // (workers report here, never into p->err)
        std::thread th;
        int rc = DVT_OK;
        size_t at = 0;   // the position of the shard that failed
        std::string err;
    };
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Item> queue;   // uploaded, waiting for a lane
    int idle = 0;             // started workers that wait for a shard
    bool closed = false, failed = false;
    Worker w[MAX_LANES];
    int n = 0;                // started workers (written by the feeder only)
};
}  // namespace

static void phase1_worker(const Lane &feeder, const DeviceKey &key, dvt_job *j, Executor &ex, Phase1Lanes *q, int k) {
    Phase1Lanes::Worker &me = q->w[k];
    const Lane c{feeder.p, feeder.mem, k, lane_engine(feeder.mem, k), me.err};
    const hipError_t dev = hipSetDevice(c.mem.eng.device);
    for (;;) {
        Phase1Lanes::Item it;
        {
            std::unique_lock<std::mutex> lk(q->mu);
            q->idle++;
            q->cv.wait(lk, [&] { return q->failed || q->closed || !q->queue.empty(); });
            q->idle--;
            if (q->failed || q->queue.empty()) return;
            it = q->queue.front();
            q->queue.pop_front();
            q->cv.notify_all();   // (the feeder uploads the next shard)
        }
        const int rc = dev != hipSuccess ? fail(me.err, DVT_ERR_DEVICE, "hipSetDevice: %s", hipGetErrorString(dev)) : shard_commit(c, key, j, *it.s, true, &ex.count);
        ex.give_back(it.buf);
        if (rc) {
            ex.cancel();
            std::lock_guard<std::mutex> lk(q->mu);
            me.rc = rc;
            me.at = it.pos;
            q->failed = true;   // the other lanes stop at their next shard boundary, the feeder after its upload
            q->cv.notify_all();
            return;
        }
    }
}

static int commit_on_lanes(const Lane &c, const DeviceKey &key, dvt_job *j, Executor &ex, bool time_stages, Clock::time_point t_begin) {
    Member &mem = c.mem;
    JobPart &part = j->parts[mem.index];
    Phase1Lanes q;
    std::deque<ShardJob> built;   // (the workers hold references: the part takes the shards, in execution order, at the end)
    int rc = DVT_OK;
    size_t rc_at = ~(size_t)0;
    hipEvent_t ev = nullptr;
    (void)hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    for (size_t pos = part.first;; pos += part.stride) {
        {
            std::unique_lock<std::mutex> lk(q.mu);
            q.cv.wait(lk, [&] { return q.failed || q.queue.empty(); });
            if (q.failed) break;
        }
        ReadyShard r;
        if (!ex.take(pos, &r, &part.t_exec_wait)) break;
        rc_at = pos;
        if (!r.err.empty()) {
            rc = r.unsupported ? fail(c.err, DVT_ERR_UNSUPPORTED, "no chip for an instruction of the guest (%s)", r.err.c_str())
                               : fail(c.err, DVT_ERR_GUEST, "guest trapped: %s", r.err.c_str());
            ex.give_back(r.buf);
            break;
        }
        if (time_stages) fprintf(stderr, "[prepare] %.2f ms: shard at position %zu ready\n", ms_since(t_begin), pos);
        built.emplace_back();
        rc = upload_shard(c, r, built.back(), ev, mem.copy_stream, true);
        if (time_stages) fprintf(stderr, "[prepare] %.2f ms: uploaded\n", ms_since(t_begin));
        if (rc) { ex.give_back(r.buf); break; }
        bool start;
        {
            std::lock_guard<std::mutex> lk(q.mu);
            q.queue.push_back({&built.back(), pos, r.buf});
            start = q.idle == 0 && q.n < c.p->phase1_lanes;
            q.cv.notify_all();
        }
        if (!start) continue;
        if (q.n > 0) {   // (an engine allocates, and the committers read the member's lanes: under the turn)
            std::lock_guard<std::mutex> turn(device_turn(mem.eng.device));
            rc = ensure_lane(mem, q.n, c.err);
        }
        if (rc) break;
        q.w[q.n].th = std::thread([&, k = q.n] { phase1_worker(c, key, j, ex, &q, k); });
        q.n++;
    }
    if (rc) ex.cancel();
    {
        std::lock_guard<std::mutex> lk(q.mu);
        if (rc) q.failed = true;
        q.closed = true;
        q.cv.notify_all();
    }
    for (int k = 0; k < q.n; k++) q.w[k].th.join();
    for (auto &it : q.queue) ex.give_back(it.buf);   // (left behind by a failure)
    (void)hipStreamSynchronize(mem.copy_stream);
    for (int k = 0; k < q.n; k++) (void)hipStreamSynchronize(lane_engine(mem, k).stream);
    (void)hipEventDestroy(ev);
    for (auto &s : built) part.shards.push_back(std::move(s));
    for (int k = 0; k < q.n; k++)   // the error of the lowest failed position
        if (q.w[k].rc && (!rc || q.w[k].at < rc_at)) {
            rc_at = q.w[k].at;
            rc = fail(c.err, q.w[k].rc, "%s", q.w[k].err.c_str());
        }
    if (time_stages) fprintf(stderr, "[prepare] %.2f ms: phase 1 of the last shard done (%d lanes)\n", ms_since(t_begin), q.n);
    return rc;
}

// Phase 1 of the job's shards in execution order, as the executor hands them over: the records of shard i+1 come in on the
// copy stream while the GPU runs phase 1 of shard i.  Every pinned buffer goes back to the executor.  (One phase-1 lane: one
// compute stream, the calling thread uploads and commits in turn.)
static int commit_overlapped(const Lane &c, const DeviceKey &key, dvt_job *j, Executor &ex, bool time_stages, Clock::time_point t_begin) {
    if (c.p->phase1_lanes > 1) return commit_on_lanes(c, key, j, ex, time_stages, t_begin);
    JobPart &part = j->parts[c.mem.index];
    int rc = DVT_OK;
    hipEvent_t ev = nullptr;
    (void)hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    bool have_prev = false;
    rv32::CycleRec *prev_buf = nullptr;
    for (size_t pos = part.first; rc == DVT_OK; pos += part.stride) {
        ReadyShard r;
        const bool got = ex.take(pos, &r, &part.t_exec_wait);
        if (got && !r.err.empty()) {
            rc = r.unsupported ? fail(c.err, DVT_ERR_UNSUPPORTED, "no chip for an instruction of the guest (%s)", r.err.c_str())
                               : fail(c.err, DVT_ERR_GUEST, "guest trapped: %s", r.err.c_str());
            ex.give_back(r.buf);
            break;
        }
        if (time_stages && got) fprintf(stderr, "[prepare] %.2f ms: shard at position %zu ready\n", ms_since(t_begin), pos);
        if (got) {
            part.shards.emplace_back();
            rc = upload_shard(c, r, part.shards.back(), ev, c.eng.stream, false);
        }
        if (time_stages && got) fprintf(stderr, "[prepare] %.2f ms: uploaded\n", ms_since(t_begin));
        // phase 1 of the previous shard runs while the copy engine brings this one in
        if (rc == DVT_OK && have_prev) {
            ShardJob &ps = part.shards[part.shards.size() - (got ? 2 : 1)];
            rc = shard_commit(c, key, j, ps, false, &ex.count);
            ex.give_back(prev_buf);
        }
        if (!got) { have_prev = false; break; }
        if (rc == DVT_OK) {
            // the event is re-recorded per shard: wait for this copy before the buffer can be reused / the event re-armed.
            // (the host waits, so the compute stream needs no dependency on the copy stream)
            if (hipEventSynchronize(ev) != hipSuccess) rc = fail(c.err, DVT_ERR_DEVICE, "record upload failed");
        }
        have_prev = true;
        prev_buf = r.buf;
    }
    if (rc == DVT_OK && have_prev) {
        rc = shard_commit(c, key, j, part.shards.back(), false, &ex.count);
        ex.give_back(prev_buf);
    }
    if (time_stages) fprintf(stderr, "[prepare] %.2f ms: phase 1 of the last shard done\n", ms_since(t_begin));
    (void)hipEventDestroy(ev);
    return rc;
}

// the verdict on the execution once the executor has stopped, given what phase 1 returned
static int prepare_verdict(std::string &err, const FastPass &f, int rc) {
    if (rc == DVT_ERR_GUEST && f.unsupported) return fail(err, DVT_ERR_UNSUPPORTED, "no chip for %s", f.unsupported_what.c_str());
    if (rc) return rc;
    if (!f.error.empty()) return fail(err, DVT_ERR_GUEST, "guest trapped: %s", f.error.c_str());
    if (f.unsupported) return fail(err, DVT_ERR_UNSUPPORTED, "no chip for %s", f.unsupported_what.c_str());
    if (f.exit_code != 0) return fail(err, DVT_ERR_GUEST, "guest halted with exit code %d", f.exit_code);
    uint32_t want[8];
    pv_digest_words(f.public_values, want);
    bool ok = f.committed_mask == 0xff;
    for (int k = 0; ok && k < 8; k++) ok = f.committed[k] == want[k];
    if (!ok) return fail(err, DVT_ERR_GUEST, "guest did not COMMIT the SHA-256 digest of the %zu public-value bytes it wrote to fd 3", f.public_values.size());
    return DVT_OK;
}

// Phase 1 on a handle with several members: every member runs the upload + phase-1 loop for its part of the job on a thread
// of its own (its device, copy stream, staging and lanes), all fed by the one executor.  The threads report into strings of
// their own, never into p->err; the error is that of the lowest failed position.  Every thread is joined and every member's
// streams are idle on return.
static int commit_on_members(dvt_prover *p, const dvt_pk *pk, dvt_job *j, Executor &ex, bool time_stages, Clock::time_point t_begin) {
    const size_t G = n_members(p);
    struct Run { int rc = DVT_OK; std::string err; };
    std::vector<Run> runs(G);
    std::vector<std::thread> threads;
    for (size_t m = 0; m < G; m++) threads.emplace_back([&, m] {
        Run &r = runs[m];
        Member &mem = member(p, m);
        const hipError_t e = hipSetDevice(mem.eng.device);
        r.rc = e != hipSuccess ? fail(r.err, DVT_ERR_DEVICE, "hipSetDevice(%d): %s", mem.eng.device, hipGetErrorString(e))
                               : commit_overlapped(Lane{p, mem, 0, mem.eng, r.err}, member_key(pk, m), j, ex, time_stages, t_begin);
        if (r.rc) ex.cancel();
    });
    for (auto &t : threads) t.join();
    int rc = DVT_OK;
    size_t at = ~(size_t)0;
    for (size_t m = G; m-- > 0;) {
        if (select_member(p, m) == DVT_OK) {
            (void)hipStreamSynchronize(member(p, m).copy_stream);
            (void)sync_lanes(member(p, m));
        }
        const JobPart &q = j->parts[m];
        const size_t pos = q.first + q.shards.size() * q.stride;   // about where it stopped
        if (runs[m].rc && pos <= at) { at = pos; rc = runs[m].rc; p->err = runs[m].err; }
    }
    return rc;
}

static int job_prepare(dvt_prover *p, const dvt_pk *pk, const dvt_buf *stdin_bufs, size_t nbuf, size_t first, size_t stride, dvt_job **out,
                       dvt_report *report) {
    if (stride == 0 || first >= stride) return fail(p, DVT_ERR_INPUT, "bad shard partition %zu / %zu", first, stride);
    const size_t G = n_members(p);
    if (int rc = same_members(p, pk, nullptr)) return rc;
    unsigned hw = std::thread::hardware_concurrency();
    const unsigned n_workers = p->exec_threads ? p->exec_threads : std::max(1u, std::min(6u, hw > 3 ? hw - 2 : 1u));
    // pinned staging: one buffer per worker + two in flight on the GPU side of every member (one in upload, one in commit) and
    // one more for each further lane that commits.  Any worker's buffer may go to any member, so with several members the
    // buffers are pinned for every device (portable).
    const size_t want_bufs = n_workers + (2 + (size_t)(p->phase1_lanes - 1)) * G;
    while (p->pinned.size() < want_bufs) {
        rv32::CycleRec *b = nullptr;
        HIP_TRY(p, hipHostMalloc(&b, sizeof(rv32::CycleRec) << p->log_shard, G > 1 ? hipHostMallocPortable : hipHostMallocDefault));
        p->pinned.push_back(b);
    }
    const bool time_stages = getenv("DVT_TIME_PREPARE") != nullptr;   // (stderr: where the host side of a prepare goes)
    const auto t_begin = Clock::now();
    const std::vector<std::vector<uint8_t>> inputs = collect_stdin(stdin_bufs, nbuf);
    Executor ex(pk, inputs, p->log_shard, p->max_cycles, first, stride, n_workers, p->pinned, time_stages);
    dvt_job *j = new dvt_job();
    j->first = first; j->stride = stride;
    j->byte_words = (size_t)rv32::N_BYTE_OPS * 65536;
    j->prog_words = (size_t)1 << pk->prep.log_n[RV32_CHIP_PROGRAM];
    j->parts.resize(G);
    for (size_t m = 0; m < G; m++) { j->parts[m].first = first + m * stride; j->parts[m].stride = stride * G; }
    // (one member: phase 1 runs on the calling thread)
    int rc = G == 1 ? commit_overlapped(lane0(p), member_key(pk, 0), j, ex, time_stages, t_begin) : commit_on_members(p, pk, j, ex, time_stages, t_begin);
    for (auto &q : j->parts) j->t_exec_wait = std::max(j->t_exec_wait, q.t_exec_wait);
    FastPass &f = ex.finish();
    if (time_stages) fprintf(stderr, "[prepare] %.2f ms: threads joined\n", ms_since(t_begin));
    if (report) {
        report->cycles = f.cycles;
        report->exit_code = f.halted ? f.exit_code : -1;
        report->halted = f.halted;
        report->unprovable = f.unsupported;
    }
    rc = prepare_verdict(p->err, f, rc);
    if (rc) { job_release(p, j); return rc; }
    j->exit_code = f.exit_code;
    j->cycles = f.cycles;
    j->public_values = std::move(f.public_values);
    j->n_total = f.n_total;
    *out = j;
    return DVT_OK;
}

// ------------------------------------------------------------------ the phase-2 pipeline (Phase2Pipe)
// the further lanes' engines that phase 1 has not made, on the first job that has at least two shards to prove
static int ensure_lanes(dvt_prover *p, Member &mem) {
    for (int k = 1; k < p->lanes; k++)
        if (int rc = ensure_lane(mem, k, p->err)) return rc;
    return DVT_OK;
}

static void pipe_worker(dvt_prover *p, Member *mem, Phase2Pipe *pp, PermChallenges gc, int k) {
    std::string err;
    const Lane c{p, *mem, k, lane_engine(*mem, k), err};
    const hipError_t dev = hipSetDevice(mem->eng.device);
    for (;;) {
        size_t i;
        {
            std::unique_lock<std::mutex> lk(pp->mu);
            pp->cv.wait(lk, [&] { return pp->stop || pp->failed || pp->next >= pp->slots.size() || pp->next < pp->limit; });
            if (pp->stop || pp->failed || pp->next >= pp->slots.size()) return;
            i = pp->next++;
            pp->slots[i].state = 1;
        }
        std::vector<uint32_t> words;
        err.clear();
        const int rc = dev != hipSuccess ? fail(err, DVT_ERR_DEVICE, "hipSetDevice: %s", hipGetErrorString(dev))
                                         : shard_prove(c, *pp->pk, pp->job, pp->job->parts[mem->index].shards[pp->slots[i].shard], gc, &words);
        std::lock_guard<std::mutex> lk(pp->mu);
        Phase2Pipe::Slot &s = pp->slots[i];
        s.rc = rc;
        s.err = std::move(err);
        s.words = std::move(words);
        s.state = 2;
        if (rc) pp->failed = true;   // the other lanes stop at their next shard boundary
        pp->cv.notify_all();
    }
}

// Starts the pipeline of a member over the shards of its part of the job that have a valid header, in job order from shard
// index k0 of the part (which must be one of them).  Returns DVT_OK with mem.pipe set; DVT_OK without a pipeline when there
// is nothing to run ahead (one lane, or fewer than two such shards).  `always` (a handle with several members, which run at
// the same time) starts a pipeline for a single lane or a single shard too.  Caller holds the handle's mutex and has
// selected the member; no pipeline runs on it.
static int pipe_start(dvt_prover *p, Member &mem, const DeviceKey &key, dvt_job *j, size_t k0, const PermChallenges &gc, bool always) {
    const std::vector<ShardJob> &shards = j->parts[mem.index].shards;
    if ((p->lanes < 2 && !always) || k0 >= shards.size() || !shards[k0].header_valid) return DVT_OK;
    std::vector<size_t> order;
    for (size_t k = k0; k < shards.size(); k++)
        if (shards[k].header_valid) order.push_back(k);
    if (order.size() < (always ? 1u : 2u)) return DVT_OK;
    int rc = ensure_lanes(p, mem);
    if (rc) return rc;
    HIP_TRY(p, sync_lanes(mem));   // phase 1 (on whichever lanes committed) is complete before another lane reads its buffers
    std::unique_ptr<Phase2Pipe> pp(new Phase2Pipe());
    pp->job = j;
    pp->pk = &key;
    for (int k = 0; k < 4; k++) { pp->ch[k] = gc.alpha.c[k].canonical(); pp->ch[4 + k] = gc.beta.c[k].canonical(); }
    pp->slots.resize(order.size());
    for (size_t i = 0; i < order.size(); i++) pp->slots[i].shard = order[i];
    pp->limit = (size_t)p->lanes;   // (the caller claims slot 0 next)
    const int n_workers = (int)std::min<size_t>((size_t)p->lanes, order.size());
    for (int k = 0; k < n_workers; k++) pp->workers.emplace_back(pipe_worker, p, &mem, pp.get(), gc, k);
    mem.pipe = std::move(pp);
    return DVT_OK;
}

// Waits for a slot's words.  Taking the last unclaimed slot ends the pipeline (nothing is left to run ahead).  On a failure
// the pipeline is drained and the error of the lowest failed shard is reported.
static int pipe_claim(dvt_prover *p, Member &mem, size_t slot, std::vector<uint32_t> *words) {
    Phase2Pipe &pp = *mem.pipe;
    bool ok, last;
    {
        std::unique_lock<std::mutex> lk(pp.mu);
        pp.limit = std::max(pp.limit, slot + (size_t)p->lanes);
        pp.cv.notify_all();
        pp.cv.wait(lk, [&] { return pp.slots[slot].state == 2 || (pp.failed && pp.slots[slot].state == 0); });
        Phase2Pipe::Slot &s = pp.slots[slot];
        ok = s.state == 2 && s.rc == 0;
        if (ok) {
            s.claimed = true;
            *words = std::move(s.words);
        }
        last = std::all_of(pp.slots.begin(), pp.slots.end(), [](const Phase2Pipe::Slot &x) { return x.claimed; });
    }
    if (ok) {
        if (last) (void)pipe_drain(mem);
        return DVT_OK;
    }
    std::string why;
    const int rc = pipe_drain(mem, &why);
    return fail(p, rc ? rc : DVT_ERR_DEVICE, "%s", rc ? why.c_str() : "phase-2 pipeline stopped");
}

// both phases on the handle's devices; the job must hold every shard of the execution.  Leaves no pipeline running.
// Shard i is on member i mod G; the challenges are computed once, then phase 2 runs on every member's lanes at the same time.
static int job_prove(dvt_prover *p, const dvt_pk *pk, dvt_job *j, uint8_t **proof, size_t *proof_len) {
    const size_t n = j->held(), G = n_members(p);
    if (n != j->n_total) return fail(p, DVT_ERR_INPUT, "this job holds %zu of the execution's %zu shards: prove them shard by shard", n, j->n_total);
    if (int rc = same_members(p, pk, j)) return rc;
    auto shard = [&](size_t i) -> ShardJob & { return j->parts[i % G].shards[i / G]; };
    std::vector<uint32_t> headers(n * HEADER_WORDS);
    for (size_t i = 0; i < n; i++) {
        if (!shard(i).header_valid) {
            int rc = turn_to(p, i % G);
            if (!rc) rc = shard_commit(lane0(p, i % G), member_key(pk, i % G), j, shard(i));
            if (rc) return rc;
        }
        memcpy(headers.data() + i * HEADER_WORDS, shard(i).header, sizeof(uint32_t) * HEADER_WORDS);
    }
    PermChallenges gc = global_challenges(pk->dev[0].key.vk, headers.data(), n);
    std::vector<std::vector<uint32_t>> shards(n);
    int rc = DVT_OK;
    for (size_t m = 0; m < G && !rc; m++) {
        rc = turn_to(p, m);
        if (!rc) rc = pipe_start(p, member(p, m), member_key(pk, m), j, 0, gc, G > 1);
    }
    for (size_t i = 0; i < n && !rc; i++) {   // (every shard of a member is in its pipeline when one runs: its last claim ends it)
        Member &mem = member(p, i % G);
        rc = turn_to(p, i % G);
        if (!rc) rc = mem.pipe ? pipe_claim(p, mem, i / G, &shards[i]) : shard_prove(lane0(p, i % G), member_key(pk, i % G), j, shard(i), gc, &shards[i]);
    }
    if (G > 1) pipe_drain_all(p);   // (on an error the other members still run)
    for (size_t m = G; m-- > 0;)   // member 0 last: its device stays current
        if (!turn_to(p, m)) (void)hipStreamSynchronize(member(p, m).eng.stream);
    if (rc) return rc;
    if (!proof) return DVT_OK;  // timing runs may discard the bytes
    *proof = copy_out(write_core_proof({(uint32_t)j->exit_code, j->public_values, std::move(shards)}), proof_len);
    if (!*proof) return fail(p, DVT_ERR_DEVICE, "out of host memory");
    return DVT_OK;
}

Fp4 dvt::commit_digest_term(const PermChallenges &gc, const std::vector<uint8_t> &public_values) {
    uint8_t dg[32];
    sha256(public_values.data(), public_values.size(), dg);
    Fp4 bp[13];
    bp[1] = gc.beta;
    for (int k = 2; k < 13; k++) bp[k] = bp[k - 1] * gc.beta;
    Fp4 expect = Fp4::zero();
    for (uint32_t k = 0; k < 8; k++) {
        Fp4 d = gc.alpha + Fp::from_canonical(PV_BUS) + bp[1] * Fp::from_canonical(rv32::SYS_COMMIT) + bp[5] * Fp::from_canonical(k);
        for (int b = 0; b < 4; b++) d += bp[9 + b] * Fp::from_canonical(dg[4 * k + b]);
        expect += inv(d);
    }
    return expect;
}

static std::string core_shards(const VerifyingKey &key, const CoreProof &cp, std::vector<ShardProof> &sps, PermChallenges *gc_out);

// The rv32 checks of a parsed container: shard chaining through the public values, the chip set of every shard, each
// shard's proof under the common challenges, and the COMMIT-digest balance.  "" or why the proof is rejected.
// With dev != nullptr the query part of the shards runs on the device: the host part of every shard in order up to the first
// that fails it, then the first failure in the host's order (the queries of an earlier shard come before that host failure).
static std::string verify_core(const VerifyingKey &key, const CoreProof &cp, const StarkConfig &cfg, DeviceQueries *dev = nullptr) {
    const auto t0 = Clock::now();
    const size_t nshards = cp.shards.size();
    std::vector<ShardProof> sps;
    PermChallenges gc;
    {
        const std::string why = core_shards(key, cp, sps, &gc);
        if (!why.empty()) return why;
    }
    Fp4 total = Fp4::zero();
    if (dev) {
        std::string host_why;
        size_t added = 0;
        for (; added < nshards && !dev->rc; added++) {
            Fp4 t;
            ShardQueryCtx ctx;
            host_why = verify_shard_host(key, sps[added], cfg, &gc, &t, &ctx);
            if (!host_why.empty()) break;
            total += t;
            dev->add(ctx, cp.shards[added].data(), cp.shards[added].size());
        }
        dev->finish(std::chrono::duration<double, std::milli>(Clock::now() - t0).count());
        if (dev->rc) return "";
        for (size_t i = 0; i < added; i++) {
            const std::string why = dev->why(i);
            if (!why.empty()) return "shard " + std::to_string(i + 1) + ": " + why;
        }
        if (!host_why.empty()) return "shard " + std::to_string(added + 1) + ": " + host_why;
    }
    for (size_t i = 0; !dev && i < nshards; i++) {
        Fp4 t;
        std::string why = verify_shard(key, sps[i], cfg, &gc, &t);
        if (!why.empty()) return "shard " + std::to_string(i + 1) + ": " + why;
        total += t;
    }
    const Fp4 expect = commit_digest_term(gc, cp.public_values);
    if (total != expect) return "LogUp cumulative sums do not cancel across the shards (memory bus or public-values digest)";
    return "";
}

// the first part of verify_core, which the transcoders share: the shard proofs parsed (either form), their chaining through
// the public values and their chip sets, and the LogUp challenges common to all shards
static std::string core_shards(const VerifyingKey &key, const CoreProof &cp, std::vector<ShardProof> &sps, PermChallenges *gc_out) {
    const size_t nshards = cp.shards.size();
    sps.resize(nshards);
    for (size_t i = 0; i < nshards; i++) {
        WordReader sr(cp.shards[i].data(), cp.shards[i].size());
        sps[i] = read_shard_proof(sr);
        if (sr.p != sr.end) return "trailing words after a shard proof";
    }
    // shard chaining through the public values
    std::vector<uint32_t> headers(nshards * HEADER_WORDS);
    for (size_t i = 0; i < nshards; i++) {
        const ShardProof &sp = sps[i];
        if (sp.public_values.size() != N_PUB) return "wrong number of public values";
        uint32_t pubv[N_PUB];
        for (uint32_t k = 0; k < N_PUB; k++) pubv[k] = sp.public_values[k].canonical();
        const bool last = i + 1 == nshards;
        if (pubv[3] != i + 1) return "shard index out of sequence";
        if (pubv[4] != (last ? 1u : 0u)) return "is_last flag does not match the shard's position";
        if (i == 0 && pubv[0] != key.extra[0] % P) return "first shard does not start at the entry point";
        if (i > 0 && pubv[0] != sps[i - 1].public_values[1].canonical()) return "shards do not chain (pc)";
        // only a HALT row has next_pc = HALT_PC (tools/airgen/rv32.py): control flow that merely reaches address 0 does not count
        if (last && pubv[1] != rv32::HALT_PC) return "execution did not halt";
        if (!last && pubv[1] == rv32::HALT_PC) return "halt before the last shard";
        if (last && pubv[2] != cp.exit_code % P) return "exit code mismatch";
        // chip set: program, byte, cpu, mem_image always; mem_init in the last shard only; shift / muldiv when the shard uses them
        bool have[rv32::N_CHIPS] = {};
        for (auto &c : sp.chips) {
            if (c.chip_id >= (uint32_t)rv32::N_CHIPS) return "chip id out of range";
            have[c.chip_id] = true;
        }
        for (int c : {RV32_CHIP_PROGRAM, RV32_CHIP_BYTE, RV32_CHIP_CPU, RV32_CHIP_MEM_IMAGE})
            if (!have[c]) return "a mandatory chip is missing from a shard";
        if (have[RV32_CHIP_MEM_INIT] != last) return "mem_init must be part of exactly the last shard";
        for (int k = 0; k < 8; k++) headers[i * HEADER_WORDS + k] = sp.main_root.d[k].canonical();
        for (uint32_t k = 0; k < N_PUB; k++) headers[i * HEADER_WORDS + 8 + k] = pubv[k];
    }
    *gc_out = global_challenges(key, headers.data(), nshards);
    return "";
}

// dvt_proof_compact / dvt_proof_expand: every shard of a container (or the one machine-level shard proof) in the wanted form
static int transcode(const uint8_t *vk, size_t vk_len, const uint8_t *proof, size_t proof_len, uint32_t fri_queries, uint32_t pow_bits,
                     bool to_compact, uint8_t **out, size_t *out_len, char **reason) {
    if (reason) *reason = nullptr;
    if (out) *out = nullptr;
    if (!vk || !proof || !out || !out_len) return reject(reason, DVT_ERR_INPUT, "null argument");
    VerifyingKey key;
    if (!vk_parse(vk, vk_len, &key)) return reject(reason, DVT_ERR_INPUT, "malformed verifying key");
    return verify_words(proof, proof_len, DVT_ERR_REJECTED, reason, [&](WordReader &r, std::string &why) {
        if (fri_queries == 0 || fri_queries > 1024 || pow_bits > 30) {
            why = "fri_queries must be 1..1024 and pow_bits <= 30";
            return DVT_ERR_INPUT;
        }
        const StarkConfig cfg{fri_queries, pow_bits};
        auto one = [&](const ShardProof &sp, const PermChallenges *gc, std::vector<uint32_t> *words) {
            Fp4 t;
            ShardQueryCtx ctx;
            std::string w = verify_shard_host(key, sp, cfg, gc, gc ? &t : nullptr, &ctx);
            ShardProof other;
            if (w.empty()) w = to_compact ? compact_shard(ctx, &other) : expand_shard(ctx, &other);
            if (w.empty()) { WordWriter ww; write_shard_proof(ww, other); words->swap(ww.w); }
            return w;
        };
        std::vector<uint32_t> result;
        if (r.p < r.end && *r.p == CORE_PROOF_MAGIC) {
            if (key.machine != machine_rv32() || key.extra.size() != 1) { why = "malformed verifying key"; return DVT_ERR_INPUT; }
            CoreProof cp = read_core_proof(r);
            std::vector<ShardProof> sps;
            PermChallenges gc;
            why = core_shards(key, cp, sps, &gc);
            for (size_t i = 0; why.empty() && i < sps.size(); i++) {
                why = one(sps[i], &gc, &cp.shards[i]);
                if (!why.empty()) why = "shard " + std::to_string(i + 1) + ": " + why;
            }
            if (why.empty()) result = write_core_proof(cp);
        } else {
            const ShardProof sp = read_shard_proof(r);
            if (r.p != r.end) why = "trailing bytes after proof";
            else why = one(sp, nullptr, &result);
        }
        if (!why.empty()) return DVT_ERR_REJECTED;
        if (!(*out = copy_out(result, out_len))) { why = "out of host memory"; return DVT_ERR_DEVICE; }
        return DVT_OK;
    });
}

static std::vector<uint32_t> trace_blob(const rv32::HostTraces &T, const rv32::HostPrep *prep) {
    const MachineDesc *m = machine_rv32();
    std::vector<uint32_t> w;
    uint32_t present = 0;
    for (int c = 0; c < m->n_chips; c++) present += T.present[c];
    w.push_back(present);
    for (int c = 0; c < m->n_chips; c++)
        if (T.present[c]) { w.push_back(c); w.push_back(T.log_n[c]); w.push_back(m->chips[c].main_w); w.push_back(prep ? m->chips[c].prep_w : 0); }
    w.push_back((uint32_t)T.pubs.size());
    w.insert(w.end(), T.pubs.begin(), T.pubs.end());
    for (int c = 0; c < m->n_chips; c++) {
        if (!T.present[c]) continue;
        w.insert(w.end(), T.main[c].begin(), T.main[c].end());
        if (prep) w.insert(w.end(), prep->prep[c].begin(), prep->prep[c].end());
    }
    return w;
}

// the device half of dvt_setup on one member (its device is current): the preprocessed commitment and the program tables
static int setup_on(const Lane &c, const rv32::Program &prog, const rv32::HostPrep &prep, DeviceKey *dst) {
    std::vector<ChipRef> refs;
    std::vector<std::vector<uint32_t>> host;
    for (int c : {RV32_CHIP_PROGRAM, RV32_CHIP_BYTE, RV32_CHIP_MEM_IMAGE}) {
        refs.push_back({c, prep.log_n[c]});
        host.push_back(prep.prep[c]);
    }
    if (!c.eng.setup(machine_rv32(), refs, host, &dst->key)) return engine_fail(c.err, c.eng);
    dst->key.vk.extra = {prog.entry};
    std::vector<uint32_t> rowmap = rv32::program_row_map(prog);
    size_t ib = prog.instrs.size() * sizeof(rv32::Instr);
    if (hipMalloc(&dst->d_instrs, ib) != hipSuccess || hipMalloc(&dst->d_prog_row, rowmap.size() * 4) != hipSuccess ||
        hipMemcpy(dst->d_instrs, prog.instrs.data(), ib, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dst->d_prog_row, rowmap.data(), rowmap.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        return fail(c.err, DVT_ERR_DEVICE, "uploading the program table failed");
    return DVT_OK;
}

extern "C" {

// On a handle with several members the setup runs on every member, from the one decoded program: it needs no peer access
// between the devices (and none between two members on one device), and a member whose commitment differed would be caught
// here instead of in a proof that does not verify.
int dvt_setup(dvt_prover *p, const uint8_t *elf, size_t elf_len, dvt_pk **pk_out, uint8_t **vk, size_t *vk_len) {
    if (!p || !elf || !pk_out) return fail(p, DVT_ERR_INPUT, "null argument");
    Guard g(p); if (g.rc) return g.rc;
    dvt_pk *pk = new dvt_pk();
    std::string err;
    if (!rv32::load_elf(elf, elf_len, &pk->prog, &err)) return setup_finish(p, pk, fail(p, DVT_ERR_INPUT, "ELF: %s", err.c_str()), pk_out, vk, vk_len);
    rv32::build_prep(pk->prog, &pk->prep);
    pk->is_rv32 = true;
    pk->dev.reserve(n_members(p));
    int rc = DVT_OK;
    for (size_t m = 0; m < n_members(p) && !rc; m++) {
        pk->dev.emplace_back();   // (setup_finish releases a half-built one)
        rc = turn_to(p, m);
        if (!rc) rc = setup_on(lane0(p, m), pk->prog, pk->prep, &pk->dev[m]);
        if (!rc && vk_words(pk->dev[m].key.vk) != vk_words(pk->dev[0].key.vk))
            rc = fail(p, DVT_ERR_DEVICE, "member %zu (device %d) built a verifying key that differs from member 0's", m, member(p, m).eng.device);
    }
    if (turn_to(p, 0) && !rc) rc = DVT_ERR_DEVICE;
    return setup_finish(p, pk, rc, pk_out, vk, vk_len);
}

int dvt_execute_io(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint64_t max_cycles,
                   uint8_t **public_values, size_t *pv_len, uint8_t **stdout_bytes, size_t *stdout_len, dvt_report *report, char **err_text) {
    if (err_text) *err_text = nullptr;
    if (public_values) *public_values = nullptr;
    if (stdout_bytes) *stdout_bytes = nullptr;
    if (!elf || (nbuf && !stdin_bufs)) return DVT_ERR_INPUT;
    rv32::Program prog;
    std::string err;
    if (!rv32::load_elf(elf, elf_len, &prog, &err)) {
        if (err_text) *err_text = strdup(("ELF: " + err).c_str());
        return DVT_ERR_INPUT;
    }
    rv32::ExecResult res;
    rv32::execute(prog, collect_stdin(stdin_bufs, nbuf), false, max_cycles ? max_cycles : ~0ull, 21, &res);
    if (report) {
        report->cycles = res.cycles;
        report->exit_code = res.halted ? res.exit_code : -1;
        report->halted = res.halted;
        report->unprovable = res.unsupported;
    }
    if (public_values) *public_values = dup_bytes(res.public_values, pv_len);
    if (stdout_bytes) *stdout_bytes = dup_bytes(res.stdout_bytes, stdout_len);
    if (!res.error.empty()) {
        if (err_text) *err_text = strdup(res.error.c_str());
        return DVT_ERR_GUEST;
    }
    if (res.exit_code != 0) {
        if (err_text) *err_text = strdup("guest halted with a non-zero exit code");
        return DVT_ERR_GUEST;
    }
    return DVT_OK;
}
int dvt_execute(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint64_t max_cycles,
                uint8_t **public_values, size_t *pv_len, dvt_report *report, char **err_text) {
    return dvt_execute_io(elf, elf_len, stdin_bufs, nbuf, max_cycles, public_values, pv_len, nullptr, nullptr, report, err_text);
}

int dvt_rv32_prepare(dvt_prover *p, const dvt_pk *pk, const dvt_buf *stdin_bufs, size_t nbuf, dvt_job **job, dvt_report *report) {
    return dvt_rv32_prepare_part(p, pk, stdin_bufs, nbuf, 0, 1, job, report);
}
int dvt_rv32_prepare_part(dvt_prover *p, const dvt_pk *pk, const dvt_buf *stdin_bufs, size_t nbuf, size_t first, size_t stride, dvt_job **job,
                          dvt_report *report) {
    if (!p || !pk || !job || (nbuf && !stdin_bufs)) return fail(p, DVT_ERR_INPUT, "null argument");
    if (int rc = rv32_key(p, pk)) return rc;
    Guard g(p); if (g.rc) return g.rc;
    return job_prepare(p, pk, stdin_bufs, nbuf, first, stride, job, report);
}
int dvt_rv32_prove_job(dvt_prover *p, const dvt_pk *pk, dvt_job *job, uint8_t **proof, size_t *proof_len) {
    if (!p || !pk || !job || (proof && !proof_len)) return fail(p, DVT_ERR_INPUT, "null argument");
    Guard g(p); if (g.rc) return g.rc;
    return job_prove(p, pk, job, proof, proof_len);
}
void dvt_job_free(dvt_prover *p, dvt_job *job) {
    if (!p || !job) return;
    Guard g(p);
    job_release(p, job);
}
size_t dvt_rv32_job_shards(const dvt_job *job) { return job ? job->n_total : 0; }
int dvt_rv32_job_shard_member(const dvt_job *job, size_t shard) {
    size_t m = 0;
    return job && const_cast<dvt_job *>(job)->at(shard, &m) ? (int)m : -1;
}
uint32_t dvt_rv32_job_shard_device_rows(const dvt_job *job, size_t shard) {
    size_t m = 0;
    const ShardJob *s = job ? const_cast<dvt_job *>(job)->at(shard, &m) : nullptr;
    return s ? s->device_rows : 0;
}
uint32_t dvt_rv32_job_shard_chips(const dvt_job *job, size_t shard) {
    size_t m = 0;
    const ShardJob *s = job ? const_cast<dvt_job *>(job)->at(shard, &m) : nullptr;
    uint32_t mask = 0;
    for (int c = 0; s && c < rv32::N_CHIPS; c++) mask |= (uint32_t)s->present[c] << c;
    return mask;
}
double dvt_rv32_job_exec_wait_seconds(const dvt_job *job) { return job ? job->t_exec_wait : 0.0; }
// (read without the handle, like the getters above: between calls on the job, not during one)
int dvt_rv32_job_shard_kept(const dvt_job *job, size_t shard) {
    size_t m = 0;
    const ShardJob *s = job ? const_cast<dvt_job *>(job)->at(shard, &m) : nullptr;
    return s ? s->kept : -1;
}
uint64_t dvt_rv32_job_shard_kept_bytes(const dvt_job *job, size_t shard) {
    const int tier = dvt_rv32_job_shard_kept(job, shard);
    if (tier <= DVT_KEEP_NONE) return 0;
    size_t m = 0;
    const ShardJob *s = const_cast<dvt_job *>(job)->at(shard, &m);
    uint64_t n = s->cache.tree_bytes();
    if (tier == DVT_KEEP_FULL) n += s->cache.lde_bytes() + (s->d_cpu ? shard_k0_bytes(job, *s) : 0);
    return n;
}

int dvt_rv32_commit_shard(dvt_prover *p, const dvt_pk *pk, dvt_job *job, size_t shard, uint32_t *header) {
    if (!p || !pk || !job || !header) return fail(p, DVT_ERR_INPUT, "bad argument");
    if (int rc = same_members(p, pk, job)) return rc;
    size_t m = 0;
    ShardJob *s = job->at(shard, &m);
    if (!s) return fail(p, DVT_ERR_INPUT, "shard %zu is not held by this job", shard);
    Guard g(p); if (g.rc) return g.rc;
    if (!s->header_valid) {   // (the prepare pipeline already ran phase 1; a second proof of the same job runs it again)
        int rc = turn_to(p, m);
        if (!rc) rc = shard_commit(lane0(p, m), member_key(pk, m), job, *s);
        if (rc) return rc;
    }
    memcpy(header, s->header, sizeof(uint32_t) * HEADER_WORDS);
    return DVT_OK;
}
uint32_t dvt_rv32_header_words(void) { return HEADER_WORDS; }
int dvt_rv32_challenges(const uint8_t *vk, size_t vk_len, const uint32_t *headers, size_t n, uint32_t out[8]) {
    VerifyingKey key;
    if (!vk || !headers || !out || !n || !vk_parse(vk, vk_len, &key)) return DVT_ERR_INPUT;
    for (size_t i = 0; i < n * HEADER_WORDS; i++)
        if (headers[i] >= P && (i % HEADER_WORDS) < 8) return DVT_ERR_INPUT;
    PermChallenges c = global_challenges(key, headers, n);
    for (int k = 0; k < 4; k++) { out[k] = c.alpha.c[k].canonical(); out[4 + k] = c.beta.c[k].canonical(); }
    return DVT_OK;
}
int dvt_rv32_prove_shard(dvt_prover *p, const dvt_pk *pk, dvt_job *job, size_t shard, const uint32_t challenges[8], uint8_t **proof,
                         size_t *proof_len) {
    if (!p || !pk || !job || !challenges || (proof && !proof_len)) return fail(p, DVT_ERR_INPUT, "bad argument");
    if (int rc = same_members(p, pk, job)) return rc;
    size_t m = 0;
    ShardJob *s = job->at(shard, &m);
    if (!s) return fail(p, DVT_ERR_INPUT, "shard %zu is not held by this job", shard);
    const size_t G = n_members(p);
    PermChallenges gc;
    for (int k = 0; k < 4; k++) {
        if (challenges[k] >= P || challenges[4 + k] >= P) return fail(p, DVT_ERR_INPUT, "challenge not canonical");
        gc.alpha.c[k] = Fp::from_canonical(challenges[k]);
        gc.beta.c[k] = Fp::from_canonical(challenges[4 + k]);
    }
    // phase 2 runs ahead on the prover lanes of every member: the first call of a job starts the pipelines, later calls with
    // the same challenges collect from them; anything else drains them (the guard) and takes the one-lane path
    const size_t k = (size_t)(s - job->parts[m].shards.data());
    const PipeClaim claim{job, &member_key(pk, m), challenges, k};
    Guard g(p, &claim, m); if (g.rc) return g.rc;
    Member &mem = member(p, m);
    long slot = g.slot;
    int rc = DVT_OK;
    if (slot < 0 && (G == 1 || s->header_valid)) {   // (a shard whose phase-1 result was consumed is proven alone: no member runs ahead)
        for (size_t i = 0; i < G && !rc; i++) {      // the claimed shard's member first
            const size_t mm = (m + i) % G;
            const JobPart &q = job->parts[mm];
            // its own part from the claimed shard; the others from their first shard after it
            const size_t k0 = mm == m ? k : q.first > shard ? 0 : (shard - q.first) / q.stride + 1;
            rc = turn_to(p, mm);
            if (!rc) rc = pipe_start(p, member(p, mm), member_key(pk, mm), job, k0, gc, G > 1);
        }
        if (rc) { pipe_drain_all(p); return rc; }
        if (mem.pipe) slot = 0;
    }
    rc = turn_to(p, m);
    std::vector<uint32_t> words;
    if (!rc) rc = slot >= 0 ? pipe_claim(p, mem, (size_t)slot, &words) : shard_prove(lane0(p, m), member_key(pk, m), job, *s, gc, &words);
    if (rc && G > 1) pipe_drain_all(p);
    if (rc || !proof) return rc;
    *proof = copy_out(words, proof_len);
    return *proof ? DVT_OK : fail(p, DVT_ERR_DEVICE, "out of host memory");
}
int dvt_rv32_assemble(const dvt_job *job, const uint8_t *const *shard_proofs, const size_t *lens, size_t n, uint8_t **proof, size_t *proof_len) {
    if (!job || !shard_proofs || !lens || !proof || !proof_len || n != job->n_total) return DVT_ERR_INPUT;
    std::vector<std::vector<uint32_t>> shards(n);
    for (size_t i = 0; i < n; i++) {
        if (lens[i] % 4 || !shard_proofs[i]) return DVT_ERR_INPUT;
        shards[i].resize(lens[i] / 4);
        memcpy(shards[i].data(), shard_proofs[i], lens[i]);
    }
    *proof = copy_out(write_core_proof({(uint32_t)job->exit_code, job->public_values, std::move(shards)}), proof_len);
    return *proof ? DVT_OK : DVT_ERR_DEVICE;
}

int dvt_prove_core(dvt_prover *p, const dvt_pk *pk, const dvt_buf *stdin_bufs, size_t nbuf, uint8_t **proof, size_t *proof_len,
                   dvt_report *report) {
    if (!p || !pk || !proof || !proof_len || (nbuf && !stdin_bufs)) return fail(p, DVT_ERR_INPUT, "null argument");
    if (int rc = rv32_key(p, pk)) return rc;
    Guard g(p); if (g.rc) return g.rc;
    dvt_job *j = nullptr;
    int rc = job_prepare(p, pk, stdin_bufs, nbuf, 0, 1, &j, report);
    if (rc) return rc;
    rc = job_prove(p, pk, j, proof, proof_len);
    job_release(p, j);
    return rc;
}

int dvt_verify(const uint8_t *vk, size_t vk_len, const uint8_t *proof, size_t proof_len, uint32_t fri_queries, uint32_t pow_bits,
               int32_t *exit_code, uint8_t **public_values, size_t *pv_len, char **reason) {
    if (reason) *reason = nullptr;
    if (public_values) *public_values = nullptr;
    if (!vk || !proof) return reject(reason, DVT_ERR_INPUT, "null argument");
    VerifyingKey key;
    if (!vk_parse(vk, vk_len, &key) || key.machine != machine_rv32() || key.extra.size() != 1) return reject(reason, DVT_ERR_INPUT, "malformed verifying key");
    return verify_words(proof, proof_len, DVT_ERR_REJECTED, reason, [&](WordReader &r, std::string &why) {
        // the caller states the FRI parameters it accepts; refuse settings that verify nothing
        // (blow-up 2: one bit of security per query, plus the proof-of-work bits)
        if (fri_queries == 0 || fri_queries > 1024 || pow_bits > 30) {
            why = "fri_queries must be 1..1024 and pow_bits <= 30";
            return DVT_ERR_INPUT;
        }
        const CoreProof cp = read_core_proof(r);
        why = verify_core(key, cp, StarkConfig{fri_queries, pow_bits});
        if (!why.empty()) return DVT_ERR_REJECTED;
        if (exit_code) *exit_code = (int32_t)cp.exit_code;
        if (public_values) *public_values = dup_bytes(cp.public_values, pv_len);
        return DVT_OK;
    });
}

int dvt_debug_compact_list_sweep(const uint8_t *vk, size_t vk_len, const uint8_t *proof, size_t proof_len, uint32_t fri_queries,
                                 uint32_t pow_bits, uint64_t *n_words, uint64_t *n_accepted, char **reason) {
    if (reason) *reason = nullptr;
    if (!vk || !proof || !n_words || !n_accepted) return reject(reason, DVT_ERR_INPUT, "null argument");
    *n_words = *n_accepted = 0;
    VerifyingKey key;
    if (!vk_parse(vk, vk_len, &key) || key.machine != machine_rv32() || key.extra.size() != 1) return reject(reason, DVT_ERR_INPUT, "malformed verifying key");
    return verify_words(proof, proof_len, DVT_ERR_REJECTED, reason, [&](WordReader &r, std::string &why) {
        if (fri_queries == 0 || fri_queries > 1024 || pow_bits > 30) {
            why = "fri_queries must be 1..1024 and pow_bits <= 30";
            return DVT_ERR_INPUT;
        }
        const CoreProof cp = read_core_proof(r);
        std::vector<ShardProof> sps;
        PermChallenges gc;
        why = core_shards(key, cp, sps, &gc);
        for (size_t i = 0; why.empty() && i < sps.size(); i++) {
            Fp4 t;
            ShardQueryCtx ctx;
            why = verify_shard_host(key, sps[i], StarkConfig{fri_queries, pow_bits}, &gc, &t, &ctx);
            if (why.empty() && sps[i].compact) why = verify_compact_queries(ctx);   // (the sweep starts from a shard that verifies)
            if (why.empty() && sps[i].compact) compact_list_sweep(ctx, n_words, n_accepted);
            if (!why.empty()) why = "shard " + std::to_string(i + 1) + ": " + why;
        }
        return why.empty() ? DVT_OK : DVT_ERR_REJECTED;
    });
}

int dvt_proof_compact(const uint8_t *vk, size_t vk_len, const uint8_t *proof, size_t proof_len, uint32_t fri_queries, uint32_t pow_bits,
                      uint8_t **out, size_t *out_len, char **reason) {
    return transcode(vk, vk_len, proof, proof_len, fri_queries, pow_bits, true, out, out_len, reason);
}
int dvt_proof_expand(const uint8_t *vk, size_t vk_len, const uint8_t *proof, size_t proof_len, uint32_t fri_queries, uint32_t pow_bits,
                     uint8_t **out, size_t *out_len, char **reason) {
    return transcode(vk, vk_len, proof, proof_len, fri_queries, pow_bits, false, out, out_len, reason);
}

int dvt_prover_verify(dvt_prover *p, const uint8_t *vk, size_t vk_len, const uint8_t *proof, size_t proof_len, uint32_t fri_queries,
                      uint32_t pow_bits, int32_t *exit_code, uint8_t **public_values, size_t *pv_len, char **reason) {
    if (reason) *reason = nullptr;
    if (public_values) *public_values = nullptr;
    if (!p) return DVT_ERR_INPUT;
    if (!vk || !proof) return reject(reason, DVT_ERR_INPUT, "null argument");
    VerifyingKey key;
    if (!vk_parse(vk, vk_len, &key) || key.machine != machine_rv32() || key.extra.size() != 1) return reject(reason, DVT_ERR_INPUT, "malformed verifying key");
    Guard g(p); if (g.rc) return g.rc;
    int dev_rc = DVT_OK;
    const int rc = verify_words(proof, proof_len, DVT_ERR_REJECTED, reason, [&](WordReader &r, std::string &why) {
        if (fri_queries == 0 || fri_queries > 1024 || pow_bits > 30) {
            why = "fri_queries must be 1..1024 and pow_bits <= 30";
            return DVT_ERR_INPUT;
        }
        const CoreProof cp = read_core_proof(r);
        DeviceQueries dq(p);
        why = verify_core(key, cp, StarkConfig{fri_queries, pow_bits}, &dq);
        if ((dev_rc = dq.rc)) return DVT_OK;
        if (!why.empty()) return DVT_ERR_REJECTED;
        if (exit_code) *exit_code = (int32_t)cp.exit_code;
        if (public_values) *public_values = dup_bytes(cp.public_values, pv_len);
        return DVT_OK;
    });
    return dev_rc ? dev_rc : rc;
}

int dvt_rv32_debug_traces(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint32_t log_shard, uint32_t shard,
                          uint32_t *n_shards, uint32_t **blob, size_t *blob_words, char **err_text) {
    if (err_text) *err_text = nullptr;
    if (!elf || !blob || !blob_words) return DVT_ERR_INPUT;
    auto bad = [&](int code, const std::string &m) { if (err_text) *err_text = strdup(m.c_str()); return code; };
    rv32::Program prog;
    std::string err;
    if (!rv32::load_elf(elf, elf_len, &prog, &err)) return bad(DVT_ERR_INPUT, "ELF: " + err);
    rv32::HostPrep prep;
    rv32::build_prep(prog, &prep);
    rv32::ExecResult res;
    rv32::execute(prog, collect_stdin(stdin_bufs, nbuf), true, 1ull << 32, log_shard ? log_shard : 21, &res);
    if (!res.error.empty()) return bad(DVT_ERR_GUEST, res.error);
    if (n_shards) *n_shards = (uint32_t)res.shards.size();
    rv32::HostTraces T;
    if (!rv32::build_traces_host(prog, res, shard, prep, &T, &err)) return bad(DVT_ERR_UNSUPPORTED, err);
    const std::vector<uint32_t> w = trace_blob(T, &prep);
    if (!(*blob = reinterpret_cast<uint32_t *>(copy_out(w, blob_words)))) return bad(DVT_ERR_DEVICE, "out of host memory");
    *blob_words = w.size();
    return DVT_OK;
}

// test hook: run K0 on shard `shard` of a prepared job and return the device-generated main traces (canonical),
// same blob layout as dvt_rv32_debug_traces but without preprocessed columns (prep_width = 0)
int dvt_rv32_debug_device_traces(dvt_prover *p, const dvt_pk *pk, dvt_job *j, size_t shard, uint32_t **blob, size_t *blob_words) {
    if (!p || !pk || !j || !blob || !blob_words) return fail(p, DVT_ERR_INPUT, "bad argument");
    if (int rc = same_members(p, pk, j)) return rc;
    size_t mi = 0;
    ShardJob *held = j->at(shard, &mi);
    if (!held) return fail(p, DVT_ERR_INPUT, "bad argument");
    Guard g(p); if (g.rc) return g.rc;
    std::vector<ChipTrace> traces;
    ShardJob &sj = *held;
    int rc = turn_to(p, mi);
    // (K0 again, and the shard's flag with it: not through shard_view of capi_inspect.hip, which leaves the job as found)
    if (!rc) rc = shard_traces(lane0(p, mi), member_key(pk, mi), j, sj, &traces, false);
    if (rc) return rc;
    HIP_TRY(p, hipStreamSynchronize(member(p, mi).eng.stream));
    const MachineDesc *m = machine_rv32();
    rv32::HostTraces T;
    for (int c = 0; c < rv32::N_CHIPS; c++) T.present[c] = false;
    for (auto &t : traces) {
        size_t words = (size_t)m->chips[t.chip_id].main_w << t.log_n;
        T.present[t.chip_id] = true;
        T.log_n[t.chip_id] = t.log_n;
        T.main[t.chip_id].resize(words);
        HIP_TRY(p, hipMemcpy(T.main[t.chip_id].data(), t.d_main, words * 4, hipMemcpyDeviceToHost));
        for (auto &x : T.main[t.chip_id]) x = Fp::raw(x).canonical();
    }
    for (auto x : sj.pubs) T.pubs.push_back(x.canonical());
    const std::vector<uint32_t> w = trace_blob(T, nullptr);
    if (!(*blob = reinterpret_cast<uint32_t *>(copy_out(w, blob_words)))) return fail(p, DVT_ERR_DEVICE, "out of host memory");
    *blob_words = w.size();
    return DVT_OK;
}

// test hook: add the canonical field element `add` to one main-trace cell of a table a prepared job holds, so that the job is
// no longer honest (include/dvt_prover.h).  One word read and one word written on lane 0's stream of the member that holds the
// shard, inside a buffer whose extent is checked here; the cycle records are never touched.
int dvt_rv32_debug_poke_cell(dvt_prover *p, dvt_job *j, size_t shard, uint32_t chip, uint32_t col, uint32_t row, uint32_t add) {
    if (!p || !j) return fail(p, DVT_ERR_INPUT, "bad argument");
    if (int rc = same_members(p, nullptr, j)) return rc;
    size_t mi = 0;
    ShardJob *held = j->at(shard, &mi);
    if (!held) return fail(p, DVT_ERR_INPUT, "shard %zu is not held by this job", shard);
    ShardJob &s = *held;
    const MachineDesc *m = machine_rv32();
    if (chip >= (uint32_t)rv32::N_CHIPS || !s.present[chip]) return fail(p, DVT_ERR_INPUT, "shard %zu has no table of chip %u", shard, chip);
    const uint32_t main_w = (uint32_t)m->chips[chip].main_w, log_n = s.log_n[chip];
    if (col >= main_w || log_n > 22 || row >= (1u << log_n))
        return fail(p, DVT_ERR_INPUT, "cell (%u, %u) is outside the %u x 2^%u main trace of chip %s", col, row, main_w, log_n, m->chips[chip].name);
    if (!add || add >= P) return fail(p, DVT_ERR_INPUT, "the value to add must be 1 .. p-1");
    Guard g(p); if (g.rc) return g.rc;
    const size_t words = (size_t)main_w << log_n;
    const bool counts = chip == RV32_CHIP_BYTE || chip == RV32_CHIP_PROGRAM;   // plain integers: K0 converts its copy
    uint32_t *base = nullptr;
    if (chip == RV32_CHIP_CPU) {
        if (!s.d_cpu || !s.traces_valid)
            return fail(p, DVT_ERR_UNSUPPORTED, "shard %zu holds no valid K0 output: the cpu rows are rebuilt from the cycle records", shard);
        base = s.d_cpu;
    } else {
        if (counts && words != (chip == RV32_CHIP_BYTE ? j->byte_words : j->prog_words))
            return fail(p, DVT_ERR_DEVICE, "the multiplicities of chip %s have another size than its table", m->chips[chip].name);
        base = s.d_aux[chip];
    }
    if (!base) return fail(p, DVT_ERR_DEVICE, "chip %s of shard %zu has no buffer", m->chips[chip].name, shard);
    if (int rc = turn_to(p, mi)) return rc;
    Member &mem = member(p, mi);
    HIP_TRY(p, sync_lanes(mem));   // (a kept K0 output is of the lane that committed the shard)
    uint32_t *cell = base + ((size_t)col << log_n) + row;
    uint32_t w = 0;
    HIP_TRY(p, hipMemcpyAsync(&w, cell, 4, hipMemcpyDeviceToHost, mem.eng.stream));
    HIP_TRY(p, hipStreamSynchronize(mem.eng.stream));
    w = counts ? (uint32_t)(((uint64_t)w + add) % P) : (Fp::raw(w) + Fp::from_canonical(add)).v;
    HIP_TRY(p, hipMemcpyAsync(cell, &w, 4, hipMemcpyHostToDevice, mem.eng.stream));
    HIP_TRY(p, hipStreamSynchronize(mem.eng.stream));
    // no later proof combines an honest phase-1 commitment with the poked table; a kept K0 output no longer matches poked counts
    s.header_valid = false;
    s.cache.valid = false;
    if (counts) s.traces_valid = false;
    return DVT_OK;
}

// test hook (host only, no device): the admission rule of "keep_phase1" (keep_plan.h) on the caller's figures
int dvt_debug_keep_plan(int mode, uint64_t free_bytes, uint64_t total_bytes, uint64_t reserve_bytes, uint64_t full_bytes, uint64_t tree_bytes,
                        uint64_t later_bytes, uint64_t remaining, int count_known, int64_t full_cap, uint64_t full_kept) {
    KeepPlanIn in;
    in.mode = mode == 0 || mode == 2 ? mode : 1;   // (as dvt_prover_create reads the key)
    in.free_b = free_bytes; in.total_b = total_bytes; in.reserve = reserve_bytes;
    in.full_b = full_bytes; in.tree_b = tree_bytes; in.later_b = later_bytes;
    in.remaining = remaining; in.count_known = count_known != 0;
    in.full_cap = full_cap; in.full_kept = full_kept;
    return keep_plan(in);
}

// measurement hook (host only): guest cycles per second of the executor alone, fast mode (trace = 0: what the
// sequential pass of the prove pipeline runs) or trace mode (one 48-byte record per cycle into a reused buffer)
double dvt_debug_exec_rate(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint32_t log_shard, int trace) {
    rv32::Program prog;
    std::string err;
    if (!elf || !rv32::load_elf(elf, elf_len, &prog, &err)) return 0.0;
    const std::vector<std::vector<uint8_t>> inputs = collect_stdin(stdin_bufs, nbuf);
    std::vector<rv32::CycleRec> buf;
    if (trace) buf.resize((size_t)1 << log_shard);
    rv32::ShardOut out;
    out.recs = buf.data();
    const auto t0 = Clock::now();
    rv32::Vm vm(prog, &inputs, log_shard);
    for (;;) {
        vm.run_shard(trace != 0, &out, ~0ull);
        if (vm.halted || !vm.error.empty() || !vm.next_shard()) break;
    }
    const double dt = std::chrono::duration<double>(Clock::now() - t0).count();
    return vm.halted ? (double)vm.cycles / dt : 0.0;
}

// test hook (host only): the FP64 formulation of Poseidon2 that the hashing kernels run, evaluated on the host
// (IEEE doubles + fma, the same arithmetic) against the integer permutation on n pseudo-random and edge-case states,
// through the same Montgomery conversions the kernels use.  Returns the number of differing words.
uint64_t dvt_debug_p2_f64_selfcheck(uint32_t n, uint32_t seed) {
    uint64_t bad = 0, x = 0x9e3779b97f4a7c15ull ^ seed;
    for (uint32_t t = 0; t < n; t++) {
        Fp a[16];
        double b[16];
        for (int i = 0; i < 16; i++) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            uint32_t v = (uint32_t)(x % P);
            if (t < 4) v = t == 0 ? 0 : t == 1 ? P - 1 : t == 2 ? (P - 1) / 2 + (i & 1) : (i ? P - i : 1);
            a[i] = Fp::from_canonical(v);
            b[i] = p2f::from_mont(a[i].v);
        }
        for (int rep = 0; rep < 3; rep++) {  // chained: the second and third calls start from lazy (signed) outputs
            p2_permute(a);
            p2f::permute(b);
            for (int i = 0; i < 16; i++) bad += (a[i].v != p2f::to_mont(b[i])) + (a[i].canonical() != p2f::to_canonical(b[i]));
        }
    }
    return bad;
}

// test hook (host only): p2f::sbox against x^7 mod p in integer arithmetic, on n pseudo-random integers of
// [-SBOX_IN, SBOX_IN] and on the edge families +-(2^e + d) (e = 20..36), m p + d (|m| <= 36) and m (p - 1)/2 + d
// (|m| <= 72), |d| <= 2000, clamped to the input bound (none is skipped).  Returns the number of inputs whose result is not an integer
// congruent to x^7; max_abs = the largest |x2|, |x3|, |x4|, |x7| met (the bounds stated at sbox).
uint64_t dvt_debug_p2_f64_sbox_check(uint32_t n, uint32_t seed, double *max_abs) {
    uint64_t bad = 0, s = 0x9e3779b97f4a7c15ull ^ seed;
    double mx[4] = {0, 0, 0, 0};
    const int64_t lim = (int64_t)p2f::SBOX_IN;
    auto check = [&](int64_t xi) {
        xi = xi > lim ? lim : xi < -lim ? -lim : xi;
        double v[4];
        v[3] = p2f::sbox_steps((double)xi, v[0], v[1], v[2]);
        for (int k = 0; k < 4; k++) mx[k] = fmax(mx[k], fabs(v[k]));
        const uint64_t x = (uint64_t)((xi % (int64_t)P + (int64_t)P) % (int64_t)P);
        const uint64_t x2 = x * x % P, x3 = x2 * x % P, x4 = x2 * x2 % P, want = x3 * x4 % P;
        // (an inexact step leaves a non-integer or a value far outside the bound: the cast must stay defined)
        const bool sane = fabs(v[3]) < 9e15 && v[3] == floor(v[3]);
        bad += !sane || (uint64_t)(((int64_t)v[3] % (int64_t)P + (int64_t)P) % (int64_t)P) != want;
    };
    for (uint32_t t = 0; t < n; t++) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        check((int64_t)(s % (2 * (uint64_t)lim + 1)) - lim);
    }
    for (int64_t d = -2000; d <= 2000; d++) {
        for (int e = 20; e <= 36; e++) { check(((int64_t)1 << e) + d); check(-(((int64_t)1 << e) + d)); }
        for (int64_t m = -36; m <= 36; m++) check(m * (int64_t)P + d);
        for (int64_t m = -72; m <= 72; m++) check(m * (((int64_t)P - 1) / 2) + d);
    }
    for (int k = 0; k < 4; k++) max_abs[k] = mx[k];
    return bad;
}

// test hook (host only): ntg::dif_group (with and without UNIT) and ntg::dit_group against three butterfly stages in
// integer arithmetic mod p.  Inputs: n pseudo-random groups over the whole stated input range with random twiddles, and
// the grid {0, 1, (p - 1)/2, p - 1, 0.52 p} (clamped to the input bound) x all 256 sign patterns of the eight inputs
// (whatever pattern maximises |a - b| at a stage is among them) x twiddles +-1, +-(p - 1)/2 chosen per stage (4^3) and
// eight random sets.  Two columns per call: the second holds the negated inputs.  Returns the number of outputs that are
// not integers congruent to the reference; max_*[8] = the largest magnitudes met (slots: ntg::NoProbe).
namespace {
struct NtgProbe {
    double *mx;
    DVT_HD void operator()(int k, double x) const { mx[k] = fmax(mx[k], fabs(x)); }
};
inline int64_t ntg_mod(int64_t x) { return (x % (int64_t)P + (int64_t)P) % (int64_t)P; }
// kind 0: DIF, 1: DIF with unit twiddles at j mod dist = 0, 2: DIT
uint64_t ntg_check_one(int kind, const int64_t in[8], const int64_t tw[7], double *mx) {
    double v[8][2], w[7], wp[7];
    int64_t ref[8], t[7];
    for (int k = 0; k < 7; k++) t[k] = tw[k];
    if (kind == 1) t[0] = t[4] = t[6] = 1;
    for (int k = 0; k < 7; k++) { w[k] = (double)t[k]; wp[k] = w[k] * p2f::PINV; }
    for (int j = 0; j < 8; j++) { v[j][0] = (double)in[j]; v[j][1] = -(double)in[j]; ref[j] = ntg_mod(in[j]); }
    if (kind == 0) ntg::dif_group<2, false>(v, w, wp, NtgProbe{mx});
    else if (kind == 1) ntg::dif_group<2, true>(v, w, wp, NtgProbe{mx});
    else ntg::dit_group<2>(v, w, wp, NtgProbe{mx});
    for (int s = 0; s < 3; s++) {
        const int dist = kind == 2 ? 1 << s : 4 >> s;
        const int first = kind == 2 ? (s == 0 ? 0 : s == 1 ? 1 : 3) : (s == 0 ? 0 : s == 1 ? 4 : 6);
        for (int j = 0; j < 8; j++) {
            if (j & dist) continue;
            const int64_t wj = ntg_mod(t[first + (j & (dist - 1))]);
            if (kind == 2) {
                const int64_t a = ref[j], b = ref[j + dist] * wj % (int64_t)P;
                ref[j] = (a + b) % (int64_t)P; ref[j + dist] = ntg_mod(a - b);
            } else {
                const int64_t a = ref[j], b = ref[j + dist];
                ref[j] = (a + b) % (int64_t)P; ref[j + dist] = ntg_mod(a - b) * wj % (int64_t)P;
            }
        }
    }
    uint64_t bad = 0;
    for (int j = 0; j < 8; j++)
        for (int c = 0; c < 2; c++) {
            // (an inexact step leaves a non-integer or a value far outside the bound: the cast must stay defined)
            const double x = v[j][c];
            const bool sane = fabs(x) < 9e15 && x == floor(x);
            bad += !sane || ntg_mod((int64_t)x) != (c ? ntg_mod(-ref[j]) : ref[j]);
        }
    return bad;
}
}  // namespace

uint64_t dvt_debug_ntt_group_check(uint32_t n, uint32_t seed, double *max_dif, double *max_dif_unit, double *max_dit) {
    uint64_t bad = 0, s = 0x9e3779b97f4a7c15ull ^ seed;
    double mx[3][8] = {};
    const int64_t lim[3] = {(int64_t)ntg::DIF_IN, (int64_t)ntg::DIF_IN, (int64_t)ntg::DIT_IN}, half = ((int64_t)P - 1) / 2;
    auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    auto uniform = [&](int64_t m) { return (int64_t)(next() % (2 * (uint64_t)m + 1)) - m; };
    int64_t in[8], tw[7];
    for (uint32_t g = 0; g < n; g++)
        for (int kind = 0; kind < 3; kind++) {
            for (int j = 0; j < 8; j++) in[j] = uniform(lim[kind]);
            for (int k = 0; k < 7; k++) tw[k] = uniform(half);
            bad += ntg_check_one(kind, in, tw, mx[kind]);
        }
    const int64_t mags[5] = {0, 1, half, (int64_t)P - 1, (int64_t)(0.52 * p2f::PD)};
    const int64_t tws[4] = {1, -1, half, -half};
    for (int kind = 0; kind < 3; kind++)
        for (int m = 0; m < 5; m++)
            for (int signs = 0; signs < 256; signs++) {
                if (m == 0 && signs) break;
                const int64_t mag = mags[m] > lim[kind] ? lim[kind] : mags[m];
                for (int j = 0; j < 8; j++) in[j] = (signs >> j) & 1 ? -mag : mag;
                for (int c = 0; c < 64 + 8; c++) {
                    for (int k = 0; k < 7; k++) {
                        const int stage = kind == 2 ? (k < 1 ? 0 : k < 3 ? 1 : 2) : (k < 4 ? 0 : k < 6 ? 1 : 2);
                        tw[k] = c < 64 ? tws[(c >> (2 * stage)) & 3] : uniform(half);
                    }
                    bad += ntg_check_one(kind, in, tw, mx[kind]);
                }
            }
    for (int k = 0; k < 8; k++) { max_dif[k] = mx[0][k]; max_dif_unit[k] = mx[1][k]; max_dit[k] = mx[2][k]; }
    return bad;
}

}  // extern "C"
