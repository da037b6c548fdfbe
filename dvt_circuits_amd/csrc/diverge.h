// Divergence (include/dvt_prover.h: dvt_rv32_job_diverge, dvt_execute_diverge): where two executions of one guest stop doing the
// same thing, and which values differed before they did; from the cycle records of both.  Nothing is executed again.  The rule,
// in plain C++ for both entry points (classify() and make_pair() also run in the kernels of diverge.hip; Tally is the host path's
// pass, rejoin() and finish() serve both):
//
//   Streams.  Execution X is its records in execution order: global record g is (shard = (g >> log_shard) + 1, row = g & mask),
//   every shard but the last holding exactly 2^log_shard records (rv32_exec.hip).  A call names a start in each execution,
//   (shard, row), at global numbers gA and gB (the number of records before it: a start past the end is the end).  Pair k is (A[gA + k], B[gB + k]) for k < N = min(lenA - gA, lenB - gB,
//   max_pairs), max_pairs = 0 meaning no limit.
//
//   Class of a pair.  watch::decode says what is bad and which register a record writes.
//       BAD      either record decodes as bad.
//       CONTROL  the two idx differ.
//       DATA     same idx, and at least one of the words a, b, c, m_prev differs.  mask: one bit per differing word,
//                DVT_DIV_RD (a), _RS1 (b), _RS2 (c), _MEM (m_prev).
//       SAME     everything else.
//     The timestamp words of a record (pa_prev, pa_ts, pb_ts, pc_ts, m_ts, sh_ab, sh_cm) are NOT compared: they are the
//     bookkeeping of the memory argument (when a register or word was last accessed, and in which shard), and they differ
//     wherever an address history does, also between runs that compute the same values.
//
//   Stop.  stop = the smallest k whose class is CONTROL (reason DVT_DIV_SPLIT) or BAD (DVT_DIV_BAD); without one stop = N and
//   the reason is END_BOTH (gA + N == lenA and gB + N == lenB), END_A or END_B (only that stream ends at pair N), else LIMIT.
//   Only pairs k < stop count in anything below.
//
//   Report.  summary: n_pairs = stop, reason, n_data, first_data, last_data (pair numbers, DVT_DIV_NONE without), mask = the OR
//   of the masks, n_load_diffs (DATA pairs of a load with the MEM bit: the word it read differs), n_store_diffs (pairs of a store
//   whose Decoded::after differ), the positions of pair `stop` in A and B (snap::locate: past the end, the last shard and its
//   record count), both records of pair `stop` and of pair stop - 1 with their pc (valid = 0 where the stream has none, or stop
//   is 0).  Pair stop - 1 is the deciding instruction: the branch or jalr whose operands differed.
//   regs[r], r >= 1: n_diff = pairs that write r (the rd of watch::decode, so ECALL writes t0) with a differing a; first_diff,
//   last_diff, last_write: pair numbers; live = last_write != NONE && last_write == last_diff.  With both starts at the entry
//   the live set is exactly the set of registers that hold different values at the stop; with later starts it is relative to
//   the starts: a register that differed before them and was not written since is not in it.
//   first[] / last[]: the first and the last min(K, n_data) DATA pairs, K = cap_each <= DVT_DIVERGE_MAX_KEEP, by watch::keep_of
//   (rank r < first_end to first[r], rank r >= last_begin to last[r - last_begin]).
//
//   Rejoin.  Only with DVT_DIVERGE_REJOIN and reason SPLIT.  Each side is walked from its record of pair `stop` for at most
//   `window` records (<= DVT_DIVERGE_MAX_WINDOW, 0: the default 4096), to its end or to a bad record, with a relative depth
//   d = 0 and the call tree's events (calltree::event_of: EV_CALL d + 1, EV_RET d - 1).  A record is a candidate at level 0 if
//   d == 0 when it executes.  If a RET makes d < 0 the next record is the one candidate BELOW, and the walk ends.  A match is a
//   candidate i of A and a candidate j of B with the same idx and the same level; the match with the smallest i + j, then the
//   smallest i, gives rejoin_a / rejoin_b (positions) and rejoin_skip_a = i, rejoin_skip_b = j, else DVT_DIVERGE_NO_REJOIN.
//   It finds the join of an if / else, steps over calls made on one side only, finds the exit of a loop one side runs longer
//   and falls back to the return of the frame.  It is a heuristic: the same idx at the same level need not be the same point
//   of the computation.  What confirms it is the lock-step call from the rejoin positions.
#pragma once
#include <map>
#include <string>

#include "calltree.h"
#include "snapshot.h"

namespace dvt {
namespace diverge {

constexpr uint32_t SPAN = DVT_DIVERGE_SPAN, MAX_KEEP = DVT_DIVERGE_MAX_KEEP, MAX_WINDOW = DVT_DIVERGE_MAX_WINDOW, DEFAULT_WINDOW = DVT_DIVERGE_DEFAULT_WINDOW,
                   NO_REJOIN = DVT_DIVERGE_NO_REJOIN;
constexpr unsigned long long NONE = DVT_DIV_NONE, BATCH_PAIRS = DVT_DIVERGE_BATCH_PAIRS;

// The class of a pair in one word: the mask in bits 0..3, then
enum : uint32_t { C_STOP = 1u << 4, C_BAD = 1u << 5, C_LOAD_DIFF = 1u << 6, C_STORE_DIFF = 1u << 7, C_RD_SHIFT = 8, C_RD_MASK = 31u << 8, C_MASK = 15 };

// (C_STOP: CONTROL or BAD; a word without C_STOP and with a mask is DATA; rd only without C_STOP)
DVT_HD uint32_t classify(const rv32::CycleRec &ra, const rv32::CycleRec &rb, const watch::Decoded &da, const watch::Decoded &db) {
    if (da.bad || db.bad) return C_STOP | C_BAD;
    if (ra.idx != rb.idx) return C_STOP;
    const uint32_t mask = (ra.a != rb.a ? DVT_DIV_RD : 0) | (ra.b != rb.b ? DVT_DIV_RS1 : 0) | (ra.c != rb.c ? DVT_DIV_RS2 : 0) | (ra.m_prev != rb.m_prev ? DVT_DIV_MEM : 0);
    uint32_t w = mask | (da.st & watch::ST_RD_MASK) << C_RD_SHIFT;
    if (da.dir == DVT_WATCH_LOAD && (mask & DVT_DIV_MEM)) w |= C_LOAD_DIFF;
    if (da.dir == DVT_WATCH_STORE && da.after != db.after) w |= C_STORE_DIFF;
    return w;
}

// the entry of first[] / last[] of DATA pair k
DVT_HD dvt_diverge_pair make_pair(unsigned long long k, uint32_t mask, const rv32::CycleRec &ra, const rv32::CycleRec &rb, const watch::Decoded &da,
                                  const watch::Decoded &db, uint32_t shard_a, uint32_t row_a, uint32_t shard_b, uint32_t row_b) {
    dvt_diverge_pair e{};
    e.k = k;
    e.shard_a = shard_a; e.row_a = row_a; e.shard_b = shard_b; e.row_b = row_b;
    e.idx = ra.idx; e.pc = da.pc; e.mask = mask; e.dir = da.dir;
    e.a_a = ra.a; e.b_a = ra.b; e.c_a = ra.c; e.m_a = ra.m_prev;
    e.a_b = rb.a; e.b_b = rb.b; e.c_b = rb.c; e.m_b = rb.m_prev;
    if (da.dir) {
        e.addr_a = da.addr; e.before_a = da.before; e.after_a = da.after;
        e.addr_b = db.addr; e.before_b = db.before; e.after_b = db.after;
    }
    return e;
}

// the running entry of one register; `at` are pair numbers
struct Reg {
    unsigned long long n_diff = 0, first_diff = NONE, last_diff = NONE, last_write = NONE;
};

}  // namespace diverge

// What the kernels of diverge.hip take by value (kernels.h declares the launches).  A segment is a run of pairs in which each
// side stays inside one shard: rec_a / rec_b point at the records of its first pair.  Span s of the call holds the pairs
// [k0 + 4096 (s - span0), ...) of its segment; the spans of a call are numbered in pair order across segments.
struct DivergeArgs {
    watch::Shapes sh;
    const uint32_t *statics, *offs;   // [n_instr], device
    const rv32::CycleRec *rec_a, *rec_b;
    unsigned long long k0;            // the pair number of the segment's first pair
    uint32_t n_instr, text_base, n_pairs, span0;
    uint32_t shard_a, row_a, shard_b, row_b;   // the positions of the segment's first pair
};
// One span's share, restricted to its pairs before its own stop (local pair numbers; 0xffffffff: none).
struct DivergeSpan {
    unsigned long long k_base;        // the pair number of the span's first pair
    uint32_t stop;                    // the local number of its first CONTROL or BAD pair, or the number of its pairs
    uint32_t stopped;                 // 0: no stop; 1: CONTROL; 2: BAD
    uint32_t n_data, first_data, last_data, mask, n_load, n_store;
};
static_assert(sizeof(DivergeSpan) == 40, "the span records are relayed as bytes");
// per span and register (SoA: [span][32] each): n_diff, first_diff, last_diff + 1, last_write + 1 (0: none), local
struct DivergeSpanRegs {
    uint32_t n_diff[32], first_diff[32], last_diff1[32], last_write1[32];
};
// What the merge pass leaves: the call's counts over the spans up to the first with a stop.
struct DivergeMerged {
    unsigned long long stop;          // pair number of the stop, or the number of pairs merged
    unsigned long long n_data, first_data, last_data, n_load, n_store;
    unsigned long long reg_n_diff[32], reg_first_diff[32], reg_last_diff[32], reg_last_write[32];
    uint32_t stopped, mask, n_used, pad;   // n_used: the spans that count (the stopping one included)
};

namespace diverge {

// ---------------------------------------------------------------- host only
// nullptr, or what is wrong with the arguments of a call
inline const char *input_error(uint32_t flags, uint32_t window, size_t cap_each, const dvt_diverge_pair *first, const dvt_diverge_pair *last,
                               const dvt_diverge_reg *regs, std::string *text) {
    if (flags & ~(uint32_t)DVT_DIVERGE_REJOIN) return (*text = "unknown flag").c_str();
    if (window > MAX_WINDOW) return (*text = "window " + std::to_string(window) + " (at most " + std::to_string(MAX_WINDOW) + ")").c_str();
    if (cap_each > MAX_KEEP) return (*text = "cap_each " + std::to_string(cap_each) + " (at most " + std::to_string(MAX_KEEP) + ")").c_str();
    if (!regs || (cap_each && (!first || !last))) return (*text = "null array").c_str();
    return nullptr;
}

// An execution as the rule sees it: the record counts of its shards.  global_of: the number of records before a position
// (positions compare as (shard, row) pairs, as the snapshot's do: one past the end of the execution is its end).
struct Stream {
    std::vector<uint64_t> shard_n;
    uint64_t len() const {
        uint64_t n = 0;
        for (uint64_t s : shard_n) n += s;
        return n;
    }
    uint64_t global_of(dvt_diverge_pos at) const {
        uint64_t g = 0;
        for (size_t k = 0; k < shard_n.size(); k++) g += k + 1 < at.shard ? shard_n[k] : k + 1 == at.shard ? std::min<uint64_t>(shard_n[k], at.row) : 0;
        return g;
    }
    dvt_diverge_pos locate(uint64_t g) const {
        dvt_diverge_pos p{};
        snap::locate(shard_n, g, &p.shard, &p.row);
        return p;
    }
};

inline dvt_diverge_rec rec_of(const rv32::Program &prog, const rv32::CycleRec *r) {
    dvt_diverge_rec o{};
    if (!r) return o;
    o.valid = 1; o.pc = prog.text_base + 4 * r->idx; o.idx = r->idx; o.a = r->a; o.b = r->b; o.c = r->c; o.m_prev = r->m_prev;
    return o;
}

// The rejoin of the rule.  wa / wb: the records of each side from its record of pair `stop` on, at most `window` of them
// (fewer at the end of the stream).  Returns false without a match.
struct Candidate { uint32_t i, idx, level; };   // level 0, or 1: below
inline std::vector<Candidate> candidates(const rv32::Program &prog, const watch::Statics &wst, const watch::Shapes &sh, const rv32::CycleRec *w, size_t n) {
    std::vector<Candidate> out;
    long d = 0;
    for (size_t i = 0; i < n; i++) {
        if (watch::decode(w[i], (uint32_t)wst.n(), prog.text_base, wst.statics(), wst.offs(), sh).bad) break;
        if (d < 0) { out.push_back({(uint32_t)i, w[i].idx, 1}); break; }
        if (d == 0) out.push_back({(uint32_t)i, w[i].idx, 0});
        const uint32_t ev = calltree::event_of(prog.instrs[w[i].idx].raw);
        if (ev == calltree::EV_CALL) d++;
        else if (ev == calltree::EV_RET) d--;
    }
    return out;
}
inline bool rejoin(const rv32::Program &prog, const watch::Statics &wst, const watch::Shapes &sh, const rv32::CycleRec *wa, size_t na, const rv32::CycleRec *wb,
                   size_t nb, uint32_t *skip_a, uint32_t *skip_b) {
    const std::vector<Candidate> ca = candidates(prog, wst, sh, wa, na), cb = candidates(prog, wst, sh, wb, nb);
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> first_b;   // (idx, level) -> the smallest j
    for (const Candidate &c : cb) first_b.emplace(std::make_pair(c.idx, c.level), c.i);
    bool found = false;
    for (const Candidate &c : ca) {   // (i ascending: a later equal sum does not replace)
        const auto it = first_b.find(std::make_pair(c.idx, c.level));
        if (it == first_b.end()) continue;
        if (!found || (uint64_t)c.i + it->second < (uint64_t)*skip_a + *skip_b) { *skip_a = c.i; *skip_b = it->second; found = true; }
    }
    return found;
}

// What both entry points know once the pairs are classified, and the summary it becomes.  rec(side, g): the record at global
// number g of side 0 (A) or 1 (B), nullptr past the end; window(side, g, n, out): the records [g, g + n) of that side.
struct Counts {
    unsigned long long stop = 0, n_data = 0, first_data = NONE, last_data = NONE, n_load = 0, n_store = 0;
    uint32_t stopped = 0, mask = 0;   // stopped: 0 none, 1 CONTROL, 2 BAD
    Reg reg[32];
};
template <class Rec, class Window>
inline void finish(const rv32::Program &prog, const watch::Statics &wst, const watch::Shapes &sh, const Stream &A, const Stream &B, uint64_t gA, uint64_t gB,
                   uint32_t flags, uint32_t window, uint32_t K, const Counts &c, Rec rec, Window fetch, dvt_diverge_reg regs[32],
                   dvt_diverge_summary *summary) {
    dvt_diverge_summary s{};
    const uint64_t lenA = A.len(), lenB = B.len(), stop = c.stop;
    s.n_pairs = stop;
    s.reason = c.stopped == 1 ? DVT_DIV_SPLIT : c.stopped == 2 ? DVT_DIV_BAD : gA + stop == lenA && gB + stop == lenB ? DVT_DIV_END_BOTH :
               gA + stop == lenA ? DVT_DIV_END_A : gB + stop == lenB ? DVT_DIV_END_B : DVT_DIV_LIMIT;
    s.n_data = c.n_data; s.first_data = c.first_data; s.last_data = c.last_data; s.mask = c.mask;
    s.n_load_diffs = c.n_load; s.n_store_diffs = c.n_store;
    s.cycles_a = lenA; s.cycles_b = lenB;
    const dvt_diverge_pos pa = A.locate(gA + stop), pb = B.locate(gB + stop);
    s.stop_shard_a = pa.shard; s.stop_row_a = pa.row; s.stop_shard_b = pb.shard; s.stop_row_b = pb.row;
    s.stop_a = rec_of(prog, rec(0, gA + stop)); s.stop_b = rec_of(prog, rec(1, gB + stop));
    if (stop) { s.prev_a = rec_of(prog, rec(0, gA + stop - 1)); s.prev_b = rec_of(prog, rec(1, gB + stop - 1)); }
    s.n_kept = (uint32_t)std::min<uint64_t>(K, c.n_data);
    s.span = SPAN;
    s.batch_pairs = (uint32_t)BATCH_PAIRS;
    s.window = window ? window : DEFAULT_WINDOW;
    s.rejoin_shard_a = s.rejoin_row_a = s.rejoin_shard_b = s.rejoin_row_b = s.rejoin_skip_a = s.rejoin_skip_b = NO_REJOIN;
    if ((flags & DVT_DIVERGE_REJOIN) && s.reason == DVT_DIV_SPLIT) {
        std::vector<rv32::CycleRec> wa, wb;
        fetch(0, gA + stop, std::min<uint64_t>(s.window, lenA - gA - stop), &wa);
        fetch(1, gB + stop, std::min<uint64_t>(s.window, lenB - gB - stop), &wb);
        uint32_t i = 0, j = 0;
        if (rejoin(prog, wst, sh, wa.data(), wa.size(), wb.data(), wb.size(), &i, &j)) {
            const dvt_diverge_pos ra = A.locate(gA + stop + i), rb = B.locate(gB + stop + j);
            s.rejoin_shard_a = ra.shard; s.rejoin_row_a = ra.row; s.rejoin_shard_b = rb.shard; s.rejoin_row_b = rb.row;
            s.rejoin_skip_a = i; s.rejoin_skip_b = j;
        }
    }
    for (uint32_t r = 0; r < 32; r++) {
        dvt_diverge_reg o{};
        o.n_diff = c.reg[r].n_diff; o.first_diff = c.reg[r].first_diff; o.last_diff = c.reg[r].last_diff; o.last_write = c.reg[r].last_write;
        o.live = o.last_write != NONE && o.last_write == o.last_diff;
        regs[r] = o;
    }
    *summary = s;
}

// The host path's state: the records of one run from its start on.
struct Kept {
    static constexpr uint64_t MAX_KEPT = (uint64_t)1 << 24;
    Stream st;
    std::vector<rv32::CycleRec> recs;   // from global number g0 on
    uint64_t g0 = 0;
    bool too_many = false;
    // the records of the next shard; start: the position the call names
    void scan(const rv32::CycleRec *r, size_t n, dvt_diverge_pos start) {
        const uint32_t shard = (uint32_t)st.shard_n.size() + 1;
        size_t from = shard < start.shard ? n : shard == start.shard ? std::min<size_t>(n, start.row) : 0;
        if (recs.empty() && from < n) g0 = st.len() + from;
        if (recs.size() + (n - from) > MAX_KEPT) too_many = true;
        else recs.insert(recs.end(), r + from, r + n);
        st.shard_n.push_back(n);
    }
    const rv32::CycleRec *at(uint64_t g) const { return g >= g0 && g - g0 < recs.size() ? &recs[g - g0] : nullptr; }
};

// The host path: the rule over the kept records of both runs, sequentially.
inline void compare(const rv32::Program &prog, const Kept &A, const Kept &B, uint64_t gA, uint64_t gB, uint64_t max_pairs, uint32_t flags, uint32_t window,
                    uint32_t K, dvt_diverge_pair *first, dvt_diverge_pair *last, dvt_diverge_reg regs[32], dvt_diverge_summary *summary) {
    const watch::Statics wst(prog);
    const watch::Shapes sh = watch::shapes();
    const uint64_t lenA = A.st.len(), lenB = B.st.len();
    uint64_t N = std::min(lenA - gA, lenB - gB);
    if (max_pairs) N = std::min(N, max_pairs);
    Counts c;
    std::vector<dvt_diverge_pair> ring(K);
    auto decode = [&](const rv32::CycleRec &r) { return watch::decode(r, (uint32_t)wst.n(), prog.text_base, wst.statics(), wst.offs(), sh); };
    uint64_t k = 0;
    for (; k < N; k++) {
        const rv32::CycleRec &ra = *A.at(gA + k), &rb = *B.at(gB + k);
        const watch::Decoded da = decode(ra), db = decode(rb);
        const uint32_t w = classify(ra, rb, da, db);
        if (w & C_STOP) { c.stopped = w & C_BAD ? 2 : 1; break; }
        if (const uint32_t rd = (w & C_RD_MASK) >> C_RD_SHIFT) {
            c.reg[rd].last_write = k;
            if (w & DVT_DIV_RD) {
                c.reg[rd].n_diff++;
                if (c.reg[rd].first_diff == NONE) c.reg[rd].first_diff = k;
                c.reg[rd].last_diff = k;
            }
        }
        if (!(w & C_MASK)) continue;
        if (K) {
            const dvt_diverge_pos pa = A.st.locate(gA + k), pb = B.st.locate(gB + k);
            const dvt_diverge_pair e = make_pair(k, w & C_MASK, ra, rb, da, db, pa.shard, pa.row, pb.shard, pb.row);
            if (c.n_data < K) first[c.n_data] = e;
            ring[c.n_data % K] = e;
        }
        if (c.first_data == NONE) c.first_data = k;
        c.last_data = k;
        c.n_data++;
        c.mask |= w & C_MASK;
        c.n_load += (w & C_LOAD_DIFF) != 0;
        c.n_store += (w & C_STORE_DIFF) != 0;
    }
    c.stop = k;
    const watch::Keep keep = watch::keep_of(c.n_data, K);
    for (unsigned long long r = keep.last_begin; r < c.n_data; r++) last[r - keep.last_begin] = ring[r % K];
    const Kept *side[2] = {&A, &B};
    finish(prog, wst, sh, A.st, B.st, gA, gB, flags, window, K, c, [&](int x, uint64_t g) { return side[x]->at(g); },
           [&](int x, uint64_t g, uint64_t n, std::vector<rv32::CycleRec> *out) {
               for (uint64_t i = 0; i < n; i++) out->push_back(*side[x]->at(g + i));
           },
           regs, summary);
}

}  // namespace diverge
}  // namespace dvt
