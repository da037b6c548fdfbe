// The host's end of the join hunt (hunt_join.cuh) on one lane: the requests' checks, the challenges from the seed, the supply
// set, the honest tables' precondition, the split of the candidates into bounded launches, the two JOIN kernels (they do not
// depend on a chip) and the groups.  SUPPLY, HONEST and EMIT are instantiated per chip in hunt_join_toy.hip,
// hunt_join_rv32.hip and hunt_join_rv32_wide.hip.
#include <algorithm>
#include <array>
#include <map>
#include <set>
#include <tuple>

#include "capi_internal.h"
#include "challenger.h"
#include "hunt_join.cuh"

namespace dvt {
namespace {
static_assert(sizeof(dvt_join_cell) == 28 && sizeof(dvt_join_summary) == 72, "as the header says");

// xi of the closed-form identities and the key of the fingerprints: as the hunt's (hunt.hip), under a domain tag of its own
void join_challenges(uint64_t seed, Fp4 *xi, uint64_t *key) {
    Challenger g;
    for (const char *t = "dvt-hunt-join-1"; *t; t++) g.observe_u32((uint8_t)*t);
    g.observe_u32((uint32_t)(seed & 0x3fffffffu));
    g.observe_u32((uint32_t)((seed >> 30) & 0x3fffffffu));
    g.observe_u32((uint32_t)(seed >> 60));
    *xi = g.sample_ext();
    *key = 0;
    for (int k = 0; k < 3; k++) *key ^= (uint64_t)g.sample().canonical() << (k == 2 ? 33 : 31 * k);
}

// INSERT: one thread per open record
__global__ void __launch_bounds__(256) join_insert_kernel(JoinTable t) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= t.n_recs) return;
    uint32_t c[3];
    const uint32_t side = join_canonical(t.recs[i].d, c);
    const uint64_t key = join_slot_key(c);
    uint32_t s = join_start(key);
    for (uint32_t k = 0; k < JOIN_PROBES; k++, s++) {
        JoinSlot &slot = t.slots[s & t.slot_mask];
        const unsigned long long old = atomicCAS(&slot.key, 0ull, (unsigned long long)key);
        if (old == 0 || old == key) {
            atomicAdd(&slot.n[side], 1u);
            return;
        }
    }
    t.flags[JOIN_FLAG_NO_SLOT] = 1;
}
// PROBE: one thread per open record; whole waves reach the ballot of join_emit
__global__ void __launch_bounds__(256) join_probe_kernel(JoinTable t) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const JoinRecord r = t.recs[i < t.n_recs ? i : t.n_recs - 1];
    uint32_t c[3];
    join_canonical(r.d, c);
    const uint64_t key = join_slot_key(c);
    uint32_t s = join_start(key);
    bool both = false;
    for (uint32_t k = 0; k < JOIN_PROBES; k++, s++) {
        const JoinSlot &slot = t.slots[s & t.slot_mask];
        const unsigned long long have = slot.key;
        if (have == key) both = slot.n[0] != 0 && slot.n[1] != 0;
        if (have == key || have == 0) break;
    }
    join_emit(both && i < t.n_recs, t.counters + 2, t.out, t.cap_out, r);
}

unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }
uint32_t pow2_at_least(uint64_t x) {
    uint32_t l = 0;
    while (((uint64_t)1 << l) < x) l++;
    return l;
}
using CellKey = std::tuple<uint32_t, uint32_t, uint32_t, uint32_t, uint32_t>;   // (tag, chip, row, col, delta)
CellKey cell_of(const JoinDev &j, const JoinRecord &r) {
    return {r.where & 0xffffu, r.where >> 16, r.row, r.col, j.deltas[r.delta < j.n_deltas ? r.delta : 0]};
}
dvt_join_cell cell_out(const CellKey &k, uint32_t group, uint32_t side) {
    return {group, side, std::get<0>(k), std::get<1>(k), std::get<3>(k), std::get<2>(k), std::get<4>(k)};
}

// the supply set from the tables kept so far: sized by their keys, built once, before the first window
int build_supply(const Lane &c, JoinDev &j, uint64_t key, uint32_t log_cap) {
    Engine &e = c.eng;
    HIP_TRY(c.err, e.pool.alloc_bytes(&j.d_supply, (size_t)8 << log_cap));
    HIP_TRY(c.err, hipMemsetAsync(j.d_supply, 0, (size_t)8 << log_cap, e.stream));
    HIP_TRY(c.err, hipMemsetAsync(j.d_flags, 0, 8, e.stream));
    j.supply_mask = (uint32_t)(((uint64_t)1 << log_cap) - 1);
    for (const JoinSupplyRef &s : j.supply) {
        JoinArgs a{};
        a.h.main = s.main; a.h.prep = s.prep;
        a.h.pub = static_cast<const uint32_t *>(e.upload_vec(s.pub_mont));
        if (!a.h.pub) return engine_fail(c.err, e);
        a.h.log_n = s.log_n;
        a.h.key = key;
        a.supply = static_cast<unsigned long long *>(j.d_supply);
        a.supply_mask = j.supply_mask;
        a.flags = static_cast<uint32_t *>(j.d_flags);
        HIP_TRY(c.err, s.d->launch_supply(e.stream, a));
    }
    uint32_t flags[2];
    if (!e.download(flags, j.d_flags, sizeof flags)) return engine_fail(c.err, e);
    if (flags[JOIN_FLAG_SUPPLY_FULL]) return fail(c.err, DVT_ERR_INPUT, "supply set too small: a key found no slot in %u probes of 2^%u", JOIN_PROBES, log_cap);
    return DVT_OK;
}
int seal_supply(const Lane &c, JoinDev &j, uint64_t key) {
    uint64_t n_keys = 0;
    for (const JoinSupplyRef &s : j.supply) n_keys += (uint64_t)s.d->n_interactions << s.log_n;
    if (n_keys) {
        const uint32_t log_cap = std::max(10u, pow2_at_least(4 * n_keys));
        if (log_cap > 30) return fail(c.err, DVT_ERR_INPUT, "%llu supply keys", (unsigned long long)n_keys);
        if (int rc = build_supply(c, j, key, log_cap)) {   // (no half-built set is ever read: the next window builds it again)
            (void)hipStreamSynchronize(c.eng.stream);
            c.eng.pool.free(j.d_supply);
            j.d_supply = nullptr;
            return rc;
        }
    }
    j.sealed = true;
    return DVT_OK;
}
}  // namespace

int join_check_new(std::string &err, uint32_t n_deltas, const uint32_t *deltas, size_t cap_records, size_t cap_absorbed, uint32_t log_slots) {
    if (!deltas || n_deltas == 0 || n_deltas > HUNT_MAX_DELTAS) return fail(err, DVT_ERR_INPUT, "n_deltas %u (1..%u)", n_deltas, HUNT_MAX_DELTAS);
    for (uint32_t e = 0; e < n_deltas; e++)
        if (deltas[e] == 0 || deltas[e] >= P) return fail(err, DVT_ERR_INPUT, "delta %u is 0 or not below p", e);
    if (cap_records > HUNT_MAX_RECORDS || cap_absorbed > HUNT_MAX_RECORDS) return fail(err, DVT_ERR_INPUT, "a capacity above 2^22 records");
    if (log_slots && (log_slots < 6 || log_slots > 26)) return fail(err, DVT_ERR_INPUT, "log_slots %u (0, 6..26)", log_slots);
    return DVT_OK;
}

int join_init(const Lane &c, JoinDev *j, const MachineDesc *m, uint64_t seed, const uint32_t *deltas, uint32_t n_deltas, size_t cap_records,
              size_t cap_absorbed, uint32_t log_slots) {
    if (int rc = join_check_new(c.err, n_deltas, deltas, cap_records, cap_absorbed, log_slots)) return rc;
    j->m = m;
    j->seed = seed;
    j->n_deltas = n_deltas;
    for (uint32_t e = 0; e < n_deltas; e++) j->deltas[e] = deltas[e];
    j->cap_open = cap_records ? cap_records : (size_t)HUNT_MAX_RECORDS;
    j->cap_absorbed = cap_absorbed ? cap_absorbed : (size_t)HUNT_MAX_RECORDS;
    j->log_slots = log_slots;
    j->pool = &c.eng.pool;
    if (c.eng.pool.alloc_bytes(&j->d_open, j->cap_open * sizeof(JoinRecord)) != hipSuccess ||
        c.eng.pool.alloc_bytes(&j->d_absorbed, j->cap_absorbed * sizeof(JoinRecord)) != hipSuccess ||
        c.eng.pool.alloc_bytes(&j->d_counters, 32) != hipSuccess || c.eng.pool.alloc_bytes(&j->d_flags, 8) != hipSuccess) {
        join_release(j);
        return fail(c.err, DVT_ERR_DEVICE, "no device memory for %zu + %zu join records", j->cap_open, j->cap_absorbed);
    }
    HIP_TRY(c.err, hipMemsetAsync(j->d_counters, 0, 32, c.eng.stream));
    HIP_TRY(c.err, hipMemsetAsync(j->d_flags, 0, 8, c.eng.stream));
    return DVT_OK;
}

void join_release(JoinDev *j) {
    if (!j->pool) return;
    for (void *q : {j->d_open, j->d_absorbed, j->d_counters, j->d_flags, j->d_supply}) j->pool->free(q);
    j->d_open = j->d_absorbed = j->d_counters = j->d_flags = j->d_supply = nullptr;
    j->pool = nullptr;
}

int join_supply(std::string &err, JoinDev &j, const CheckTable &t, const std::vector<uint32_t> &pub_mont) {
    if (j.sealed) return fail(err, DVT_ERR_INPUT, "a supply table after the first window");
    if (t.log_n > 22) return fail(err, DVT_ERR_INPUT, "log_n %u > 22", t.log_n);
    if (!t.d->launch_supply) return fail(err, DVT_ERR_UNSUPPORTED, "chip %s cannot serve as a supply table", t.d->name);
    j.supply.push_back({t.d, t.main, t.prep, t.log_n, pub_mont});
    return DVT_OK;
}

int join_check_add(std::string &err, const JoinDev &j, uint32_t tag, uint32_t chip, const ChipDesc &d, uint32_t log_n, uint32_t row_first,
                   uint32_t row_count, const uint32_t *cols, uint32_t n_cols, uint64_t max_evals, std::vector<uint32_t> *cols_out) {
    if (j.matched) return fail(err, DVT_ERR_INPUT, "a window after match");
    if (j.broken) return fail(err, DVT_ERR_INPUT, "an earlier window failed half way: free this join");
    if (log_n > 22) return fail(err, DVT_ERR_INPUT, "log_n %u > 22", log_n);
    if (tag >= (1u << 16)) return fail(err, DVT_ERR_INPUT, "tag %u >= 2^16", tag);
    if (chip >= 64) return fail(err, DVT_ERR_INPUT, "chip %u", chip);
    const uint64_t n = (uint64_t)1 << log_n;
    if (row_count == 0 || (uint64_t)row_first + row_count > n)
        return fail(err, DVT_ERR_INPUT, "rows %u + %u outside the table of %llu rows", row_first, row_count, (unsigned long long)n);
    if (cols && n_cols == 0) return fail(err, DVT_ERR_INPUT, "empty column list");
    for (uint32_t k = 0; cols && k < n_cols; k++)
        if (cols[k] >= (uint32_t)d.main_w) return fail(err, DVT_ERR_INPUT, "column %u: chip %s has %d", cols[k], d.name, d.main_w);
    for (const JoinInstance &in : j.instances) {
        if (in.tag != tag || in.chip != chip) continue;
        if (in.log_n != log_n) return fail(err, DVT_ERR_INPUT, "tag %u chip %s was added with 2^%u rows", tag, d.name, in.log_n);
        for (const auto &w : in.windows)
            if (row_first < w.first + w.second && w.first < row_first + row_count)
                return fail(err, DVT_ERR_INPUT, "rows %u + %u overlap the window %u + %u of tag %u chip %s", row_first, row_count, w.first, w.second, tag, d.name);
    }
    if (!d.launch_join || !d.launch_check) return fail(err, DVT_ERR_UNSUPPORTED, "chip %s has no join hunt", d.name);
    if (cols) {
        cols_out->assign(cols, cols + n_cols);
        std::sort(cols_out->begin(), cols_out->end());
        cols_out->erase(std::unique(cols_out->begin(), cols_out->end()), cols_out->end());
    } else {
        cols_out->clear();
        for (int c = 0; c < d.main_w; c++) cols_out->push_back((uint32_t)c);
    }
    const uint64_t evals = (uint64_t)j.n_deltas * cols_out->size() * row_count * std::min<uint64_t>(2, n);
    const uint64_t limit = max_evals ? max_evals : HUNT_DEFAULT_MAX_EVALS;
    if (evals > limit)
        return fail(err, DVT_ERR_INPUT, "%llu evaluations (candidates x touched rows) exceed max_evals %llu", (unsigned long long)evals, (unsigned long long)limit);
    return DVT_OK;
}

int join_add(const Lane &c, JoinDev &j, uint32_t tag, uint32_t chip, const CheckTable &t, const std::vector<uint32_t> &pub_mont, uint32_t row_first,
             uint32_t row_count, const std::vector<uint32_t> &cols) {
    Engine &e = c.eng;
    const ChipDesc &d = *t.d;
    const size_t n = (size_t)1 << t.log_n;
    Fp4 xi;
    uint64_t key;
    join_challenges(j.seed, &xi, &key);
    // the precondition: the honest table violates nothing
    {
        std::vector<CheckTableOut> res;
        const CheckChallenges ch{xi, Fp4::zero(), Fp4::zero()};
        if (int rc = check_tables(c, j.m, {t}, pub_mont, ch, true, false, &res)) return rc;
        if (res[0].r.violations)
            return fail(c.err, DVT_ERR_REJECTED, "the table is not honest: row %u violates constraint %d of chip %s (%llu violations)", res[0].r.first_row,
                        res[0].r.first_constraint, d.name, (unsigned long long)res[0].r.violations);
    }
    if (!j.sealed)
        if (int rc = seal_supply(c, j, key)) return rc;
    const uint32_t k = (uint32_t)cols.size(), nd = j.n_deltas;
    StageBuf honest{e.pool}, d_cols{e.pool};
    HIP_TRY(c.err, e.pool.alloc_bytes(&honest.ptr, 24 * n));
    HIP_TRY(c.err, e.pool.alloc_bytes(&d_cols.ptr, (size_t)k * 4));
    HIP_TRY(c.err, hipMemcpyAsync(d_cols.ptr, cols.data(), (size_t)k * 4, hipMemcpyHostToDevice, e.stream));
    int n_beta, n_alpha;
    challenge_power_counts(j.m, &n_beta, &n_alpha);
    JoinArgs a{};
    a.h.main = t.main; a.h.prep = t.prep;
    a.h.pub = static_cast<const uint32_t *>(e.upload_vec(pub_mont));
    if (!a.h.pub || !e.upload_powers(xi, (size_t)n_alpha, true, &a.h.xi_pows, &a.h.xi_d)) return engine_fail(c.err, e);
    a.h.log_n = t.log_n;
    a.h.key = key;
    a.h.row_first = row_first;
    a.h.n_deltas = nd;
    for (uint32_t i = 0; i < nd; i++) { a.h.delta_c[i] = j.deltas[i]; a.h.delta_m[i] = Fp::from_canonical(j.deltas[i]).v; }
    a.h.cols = static_cast<const uint32_t *>(d_cols.ptr);
    a.h.n_cols = k;
    a.supply = static_cast<unsigned long long *>(j.d_supply);
    a.supply_mask = j.supply_mask;
    a.honest = static_cast<uint32_t *>(honest.ptr);
    a.where = tag | (chip << 16);
    a.open = static_cast<JoinRecord *>(j.d_open);
    a.absorbed = static_cast<JoinRecord *>(j.d_absorbed);
    a.cap_open = (uint32_t)j.cap_open;
    a.cap_absorbed = (uint32_t)j.cap_absorbed;
    a.counters = static_cast<unsigned long long *>(j.d_counters);
    a.flags = static_cast<uint32_t *>(j.d_flags);

    // the launches of one pass: at most HUNT_LAUNCH_EVALS lane slots each, and the stream's status between them
    auto pass = [&](uint32_t mode, unsigned row_blocks, uint32_t rows, uint64_t n_candidates, uint32_t touched) -> int {
        a.mode = mode;
        a.h.rows = rows;
        const uint64_t per = (uint64_t)row_blocks * 256 * touched;
        const uint64_t step = std::max<uint64_t>(1, std::min<uint64_t>(HUNT_MAX_CANDIDATES, HUNT_LAUNCH_EVALS / per));
        for (uint64_t at = 0; at < n_candidates; at += step) {
            a.h.cand_first = (uint32_t)at;
            HIP_TRY(c.err, d.launch_join(e.stream, a, row_blocks, (unsigned)std::min<uint64_t>(step, n_candidates - at)));
            HIP_TRY(c.err, hipStreamSynchronize(e.stream));
        }
        return DVT_OK;
    };
    if (int rc = pass(JOIN_HONEST, blocks_of(n), (uint32_t)n, 1, 1)) return rc;
    if (int rc = pass(JOIN_EMIT, blocks_of(row_count), row_count, (uint64_t)nd * k, 2)) {
        j.broken = true;   // (records of a window the host does not know may be in the arrays)
        return rc;
    }
    j.summary.candidates += (uint64_t)nd * k * row_count;
    auto it = std::find_if(j.instances.begin(), j.instances.end(), [&](const JoinInstance &in) { return in.tag == tag && in.chip == chip; });
    if (it == j.instances.end()) it = j.instances.insert(j.instances.end(), JoinInstance{tag, chip, t.log_n, {}});
    it->windows.push_back({row_first, row_count});
    return DVT_OK;
}

int join_match(const Lane &c, JoinDev &j) {
    if (j.matched) return fail(c.err, DVT_ERR_INPUT, "match was called already");
    if (j.broken) return fail(c.err, DVT_ERR_INPUT, "a window failed half way: free this join");
    if (j.instances.empty()) return fail(c.err, DVT_ERR_INPUT, "match without a window");
    Engine &e = c.eng;
    unsigned long long cnt[4];
    if (!e.download(cnt, j.d_counters, sizeof cnt)) return engine_fail(c.err, e);
    dvt_join_summary s = j.summary;
    s.open_emitted = cnt[0];
    s.open_stored = std::min<uint64_t>(cnt[0], j.cap_open);
    s.absorbed_emitted = cnt[1];
    s.absorbed_stored = std::min<uint64_t>(cnt[1], j.cap_absorbed);
    s.truncated = (s.open_stored < s.open_emitted ? DVT_JOIN_TRUNC_RECORDS : 0) | (s.absorbed_stored < s.absorbed_emitted ? DVT_JOIN_TRUNC_ABSORBED : 0);
    std::vector<JoinRecord> hit, soaked(s.absorbed_stored);
    if (!soaked.empty() && !e.download(soaked.data(), j.d_absorbed, soaked.size() * sizeof(JoinRecord))) return engine_fail(c.err, e);
    if (s.open_stored) {
        const uint32_t n_recs = (uint32_t)s.open_stored;
        const uint32_t log_slots = j.log_slots ? j.log_slots : std::max(6u, pow2_at_least(2 * (uint64_t)n_recs));
        StageBuf slots{e.pool}, out{e.pool};
        HIP_TRY(c.err, e.pool.alloc_bytes(&slots.ptr, sizeof(JoinSlot) << log_slots));
        HIP_TRY(c.err, e.pool.alloc_bytes(&out.ptr, (size_t)n_recs * sizeof(JoinRecord)));
        HIP_TRY(c.err, hipMemsetAsync(slots.ptr, 0, sizeof(JoinSlot) << log_slots, e.stream));
        JoinTable t{};
        t.recs = static_cast<const JoinRecord *>(j.d_open);
        t.n_recs = n_recs;
        t.slots = static_cast<JoinSlot *>(slots.ptr);
        t.slot_mask = (1u << log_slots) - 1;
        t.out = static_cast<JoinRecord *>(out.ptr);
        t.cap_out = n_recs;
        t.counters = static_cast<unsigned long long *>(j.d_counters);
        t.flags = static_cast<uint32_t *>(j.d_flags);
        join_insert_kernel<<<blocks_of(n_recs), 256, 0, e.stream>>>(t);
        HIP_TRY(c.err, hipGetLastError());
        join_probe_kernel<<<blocks_of(n_recs), 256, 0, e.stream>>>(t);
        HIP_TRY(c.err, hipGetLastError());
        uint32_t flags[2];
        if (!e.download(cnt, j.d_counters, sizeof cnt) || !e.download(flags, j.d_flags, sizeof flags)) return engine_fail(c.err, e);
        s.matched = cnt[2];
        if (flags[JOIN_FLAG_NO_SLOT]) s.truncated |= DVT_JOIN_TRUNC_PROBES;
        if (cnt[2] > t.cap_out) s.truncated |= DVT_JOIN_TRUNC_OUTPUT;
        hit.resize((size_t)std::min<uint64_t>(cnt[2], t.cap_out));
        if (!hit.empty() && !e.download(hit.data(), out.ptr, hit.size() * sizeof(JoinRecord))) return engine_fail(c.err, e);
    }
    // ---- the groups: by the exact canonical words; two D that shared a slot key part here
    std::map<std::array<uint32_t, 3>, std::array<std::vector<CellKey>, 2>> by;
    for (const JoinRecord &r : hit) {
        std::array<uint32_t, 3> cw;
        const uint32_t side = join_canonical(r.d, cw.data());
        by[cw][side].push_back(cell_of(j, r));
    }
    auto rows_of = [&](uint32_t tag, uint32_t chip) -> uint32_t {
        for (const JoinInstance &in : j.instances)
            if (in.tag == tag && in.chip == chip) return 1u << in.log_n;
        return 1;
    };
    struct Group { std::vector<CellKey> side[2]; uint64_t pairs; };
    std::vector<Group> groups;
    for (auto &kv : by) {
        auto &sd = kv.second;
        if (sd[0].empty() || sd[1].empty()) continue;
        for (auto &v : sd) std::sort(v.begin(), v.end());
        // the exclusion rule: same (tag, chip), circular row distance <= 1
        std::map<std::tuple<uint32_t, uint32_t, uint32_t>, uint64_t> at;   // (tag, chip, row) -> cells of side 1
        for (const CellKey &k : sd[1]) at[{std::get<0>(k), std::get<1>(k), std::get<2>(k)}]++;
        uint64_t excluded = 0;
        for (const CellKey &k : sd[0]) {
            const uint32_t n = rows_of(std::get<0>(k), std::get<1>(k)), r = std::get<2>(k);
            for (uint32_t near : std::set<uint32_t>{r, (r + 1) % n, (r + n - 1) % n}) {
                auto f = at.find({std::get<0>(k), std::get<1>(k), near});
                if (f != at.end()) excluded += f->second;
            }
        }
        const uint64_t pairs = (uint64_t)sd[0].size() * sd[1].size() - excluded;
        if (!pairs) continue;
        if (sd[1].front() < sd[0].front()) std::swap(sd[0], sd[1]);   // side 0 holds the group's lowest cell
        groups.push_back({{std::move(sd[0]), std::move(sd[1])}, pairs});
    }
    std::sort(groups.begin(), groups.end(), [](const Group &x, const Group &y) { return x.side[0].front() < y.side[0].front(); });
    j.cells.clear();
    s.groups = groups.size();
    s.pairs = 0;
    for (size_t g = 0; g < groups.size(); g++) {
        s.pairs += groups[g].pairs;
        for (uint32_t side = 0; side < 2; side++)
            for (const CellKey &k : groups[g].side[side]) j.cells.push_back(cell_out(k, (uint32_t)g, side));
    }
    std::vector<CellKey> ab;
    for (const JoinRecord &r : soaked) ab.push_back(cell_of(j, r));
    std::sort(ab.begin(), ab.end());
    j.absorbed.clear();
    for (const CellKey &k : ab) j.absorbed.push_back(cell_out(k, DVT_JOIN_NO_GROUP, 0));
    j.summary = s;
    j.matched = true;
    return DVT_OK;
}
}  // namespace dvt
