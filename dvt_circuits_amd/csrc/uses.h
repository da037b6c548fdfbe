// Uses (include/dvt_prover.h: dvt_rv32_job_uses, dvt_execute_uses): who reads the value of a register or of a memory word, and
// what those readers produce, as the forward data-flow slice over the cycle records of an execution.  Nothing is executed again.
// What a record writes and what it reads is dataflow.h's (flow::for_written, flow::for_read), shared with the origin search; this
// header holds the forward search over it (Search below; the host path answers its definitions with Keeper, the job entry point
// with the kernels of uses.hip):
//
//   Positions, decode(), call_match(), the shapes and SPAN are watch.h's and snapshot.h's; roles and node kinds are origin.h's;
//   reads() below is flow::for_read asked about one target.
//
//   Definition (what, target, F): the value the register (DVT_USES_REG, 1..31) or the 4-aligned word below ADDR_LIMIT
//   (DVT_USES_WORD) holds from position F on.
//       Next writer N   the first record at a position >= F that writes the target, by flow::for_written: rd == k (so
//                       ECALL writes t0), a sw / sh / sb to the word, a call whose PRE_WRITE words contain it.  None: N = NONE
//                       and the definition is LIVE_AT_EXIT.
//       Uses            every input edge of every record at a position in [F, N] whose (REG | WORD, target) is the definition's.
//                       N itself is included: addi a0,a0,1 both uses and ends a0, a sb both reads and rewrites its word.  A
//                       record that reads the register as rs1 and as rs2 is two uses.
//       Roles           origin's ADDR / RS1 / RS2 / MEM with origin's conditions: ADDR only with DVT_USES_FOLLOW_ADDR, ECALL reads
//                       no registers, sw has no MEM input, the words a call reads are MEM.
//   Consequence: record C uses the definition made by record W if and only if origin's question (what, target, position of C)
//   is answered by W.  For the root definition (what, target, P): if and only if no writer of the target lies in [P, C).
//
//   Outputs of a node: the definitions it adds at F = its position + 1, in this order:
//       1. rd when non-zero, value rec.a;
//       2. the word of a store, value `after`;
//       3. every PRE_WRITE word of a call in call_match order (array 0 first), value 0 with NO_VALUE.
//   A branch, or a sw whose word nothing reads, is a leaf.
//
//   The root definition is (what, target, P) for the position the caller names, node = NONE; (0xffffffff, 0xffffffff) = the exit is
//   legal and has no uses.  Its value is what its first kept use read (rec.b, rec.c or the word before the access; NO_VALUE when
//   that use is a call's), else NO_VALUE.
//
//   Search, breadth first in discovery order, identical on both entry points.  Level 0 is the root definition.  The definitions
//   of level d are answered in order: N, the exact number of uses n_uses, and the first min(fan, n_uses) uses in execution order
//   (within one record ADDR, RS1, RS2, MEM).  Each kept use is an edge {def, to, role, flags, dst_shard, dst_row}: the consumer's
//   record is already a node: link to it; else, if n_nodes < cap_nodes, a new node at depth d + 1 (the fields of an origin node);
//   else CUT with to = NONE.  n_uses > fan: TRUNCATED.  Then the new nodes define their outputs, in order: a node with
//   depth >= max_depth is UNEXPANDED; a node whose outputs would take the definitions past cap_defs, or the edges past cap_edges
//   if every definition of the level kept `fan` uses, is UNEXPANDED with every later node, and the search ends after this level's
//   answers (the nodes those answers add are UNEXPANDED too).  A node defines its outputs once, however often it is reached.
//
//   Limits: DVT_USES_MAX_NODES 1024, _MAX_DEFS 4096, _MAX_EDGES 8192, _MAX_DEPTH 64, _MAX_FAN 16 (at least 1), _PASS_DEFS 256
//   (the definitions of one device pass: a wider level takes ceil(defs / 256) passes), _SPAN 4096.
//
//   summary: n_nodes, n_defs, n_edges, depth (the deepest node's); cut (edges), unexpanded (nodes), truncated, live_at_exit,
//   no_value, dead (definitions; dead: n_uses == 0); uses_total (the sum of n_uses); levels, passes (0 on the host path);
//   position, cycles, shard, row as the snapshot's; shards_total, span, ms.
//
// A bad record (watch.h's bad) anywhere at or after P fails the call with DVT_ERR_INPUT.
// What the slice cannot say: the values of the words a call wrote are not in the records; data dependence only, so a branch is a
// consumer and a leaf.
#pragma once
#include "origin.h"

namespace dvt {
namespace uses {

constexpr uint32_t SPAN = DVT_USES_SPAN, MAX_NODES = DVT_USES_MAX_NODES, MAX_DEFS = DVT_USES_MAX_DEFS, MAX_EDGES = DVT_USES_MAX_EDGES,
                   MAX_DEPTH = DVT_USES_MAX_DEPTH, MAX_FAN = DVT_USES_MAX_FAN, PASS_DEFS = DVT_USES_PASS_DEFS, NONE = DVT_USES_NONE;
constexpr unsigned long long NO_POS = ~0ull;   // no next writer
static_assert(SPAN == origin::SPAN && PASS_DEFS == origin::PASS_Q, "the launch shape of origin.hip");
static_assert((int)DVT_USES_REG == DVT_ORIGIN_REG && (int)DVT_USES_WORD == DVT_ORIGIN_WORD && (int)DVT_USES_ADDR == DVT_ORIGIN_ADDR &&
                  (int)DVT_USES_RS1 == DVT_ORIGIN_RS1 && (int)DVT_USES_RS2 == DVT_ORIGIN_RS2 && (int)DVT_USES_MEM == DVT_ORIGIN_MEM &&
                  (int)DVT_USES_OP == DVT_ORIGIN_OP && (int)DVT_USES_LOAD == DVT_ORIGIN_LOAD && (int)DVT_USES_STORE == DVT_ORIGIN_STORE &&
                  (int)DVT_USES_CALL == DVT_ORIGIN_CALL && (int)DVT_USES_SYSCALL == DVT_ORIGIN_SYSCALL && (int)DVT_USES_FOLLOW_ADDR == DVT_ORIGIN_FOLLOW_ADDR,
              "the kinds, roles and flags of origin.h");

// A definition as a pass takes it: origin's question with Q = F, sorted by origin::sorts_before.
using Def = origin::Question;

// The inputs of a record (flow::for_read) that name (what, target): n = 0..2 of them, their roles in the rule's order.  ow: the
// record's word of flow::Statics.  A word is tested against the words a call reads by range, not by walking them: the emit pass
// asks this of every record of a span.
struct Reads {
    uint32_t n, role0, role1;
};
DVT_HD Reads reads(const watch::Decoded &d, uint32_t ow, const watch::Shapes &sh, uint32_t what, uint32_t target, uint32_t flags) {
    Reads r{0, 0, 0};
    auto add = [&](uint32_t role) {
        if (r.n == 0) r.role0 = role;
        else r.role1 = role;
        r.n++;
    };
    flow::for_read_direct(d, ow, flags, true, [&](uint32_t role, uint32_t w, uint32_t t) {
        if (w == what && t == target) add(role);
    });
    if (const memrep::PreShape *ps = what == DVT_USES_WORD ? flow::call_shape(d, sh) : nullptr) {
        auto among_read = [&](uint32_t arr) {
            const memrep::CallArray e = memrep::call_array(*ps, arr, d.a0, d.a1);
            return target >= e.base && (unsigned long long)target < (unsigned long long)e.base + 4ull * e.n_read;
        };
        if (among_read(0)) add(DVT_USES_MEM);
        if (among_read(1)) add(DVT_USES_MEM);
    }
    return r;
}

}  // namespace uses

// What the kernels of uses.hip take by value (kernels.h declares the launches): the sorted definitions of a pass (PassArgs,
// pos = F) and, once known, d_next [n] (the windows [F, N], N all ones without a writer).  min_from / max_next: the smallest F
// and the largest N of the pass.
struct UsesArgs : PassArgs {
    const uint32_t *ostat;               // [n_instr], device: flow::Statics
    const unsigned long long *d_next;    // device
    uint32_t flags, fan;
    unsigned long long min_from, max_next;
};
// one span that holds kept uses of one definition: its ranks from `rank` on
struct UsesItem {
    const rv32::CycleRec *recs;
    uint32_t n_recs, shard, span, def, rank, pad;
};

namespace uses {

// ---------------------------------------------------------------- host only
// nullptr, or what is wrong with the arguments of a call
inline const char *input_error(uint32_t what, uint32_t target, uint32_t flags, uint32_t max_depth, uint32_t fan, const dvt_uses_node *nodes, size_t cap_nodes,
                               const dvt_uses_def *defs, size_t cap_defs, const dvt_uses_edge *edges, size_t cap_edges, std::string *text) {
    if (const char *why = flow::target_error(what, target, flags, max_depth, MAX_DEPTH, text)) return why;
    if (!fan || fan > MAX_FAN) return (*text = "fan " + std::to_string(fan) + " (1.." + std::to_string(MAX_FAN) + ")").c_str();
    if (cap_nodes > MAX_NODES) return (*text = "cap_nodes " + std::to_string(cap_nodes) + " (at most " + std::to_string(MAX_NODES) + ")").c_str();
    if (!cap_defs || cap_defs > MAX_DEFS) return (*text = "cap_defs " + std::to_string(cap_defs) + " (1.." + std::to_string(MAX_DEFS) + ")").c_str();
    if (cap_edges < fan || cap_edges > MAX_EDGES)
        return (*text = "cap_edges " + std::to_string(cap_edges) + " (fan.." + std::to_string(MAX_EDGES) + ")").c_str();
    if (!defs || !edges || (cap_nodes && !nodes)) return (*text = "null array").c_str();
    return nullptr;
}

// One kept use: the consumer's position, the role it reads the target in, its record.
struct Use {
    unsigned long long pos;
    uint32_t role;
    rv32::CycleRec rec;
};
// The answer to a definition: its next writer (NO_POS: none), the exact number of its uses and the first min(fan, n_uses).
struct Found {
    unsigned long long next = NO_POS;
    uint64_t n_uses = 0;
    std::vector<Use> uses;
};

// The search of the rule, for both entry points.  answer(defs, &found) fills found[i] for defs[i] and returns false when it
// could not (the caller knows why).  Returns 0, 1 when answer failed, 2 when an answer is no use of its definition (*why says
// which).  The counters of the summary are filled; position, cycles, shard, row, shards_total, passes and ms are the caller's.
struct Search {
    const rv32::Program &prog;
    const watch::Statics &wst;
    const watch::Shapes &sh;
    flow::Statics ost;
    unsigned long long P;
    uint32_t what, target, flags, max_depth, fan;
    dvt_uses_node *nodes;
    size_t cap_nodes;
    dvt_uses_def *defs;
    size_t cap_defs;
    dvt_uses_edge *edges;
    size_t cap_edges;
    dvt_uses_summary s{};
    std::vector<rv32::CycleRec> recs;                    // of the nodes
    std::vector<unsigned long long> from;                // F of the definitions
    std::map<unsigned long long, uint32_t> node_at;      // position -> node
    std::string why;

    Search(const rv32::Program &prog, const watch::Statics &wst, const watch::Shapes &sh, unsigned long long P, uint32_t what, uint32_t target, uint32_t flags,
           uint32_t max_depth, uint32_t fan, dvt_uses_node *nodes, size_t cap_nodes, dvt_uses_def *defs, size_t cap_defs, dvt_uses_edge *edges,
           size_t cap_edges)
        : prog(prog), wst(wst), sh(sh), ost(prog), P(P), what(what), target(target), flags(flags), max_depth(max_depth), fan(fan), nodes(nodes),
          cap_nodes(cap_nodes), defs(defs), cap_defs(cap_defs), edges(edges), cap_edges(cap_edges) {}

    watch::Decoded decode(const rv32::CycleRec &rec) const {
        return watch::decode(rec, (uint32_t)wst.n(), prog.text_base, wst.statics(), wst.offs(), sh);
    }
    static dvt_uses_def make_def(uint32_t node, uint32_t what, uint32_t target, uint32_t value, uint32_t flags) {
        dvt_uses_def d{};
        d.node = node; d.what = what; d.target = target; d.value = value; d.flags = flags;
        d.next_shard = d.next_row = NONE;
        return d;
    }
    // the definitions node i adds, in the rule's order
    void outputs_of(uint32_t i, std::vector<dvt_uses_def> *out) const {
        out->clear();
        const rv32::CycleRec &rec = recs[i];
        const watch::Decoded d = decode(rec);
        flow::for_written(d, sh, true, [&](uint32_t w, uint32_t tgt) {
            const bool valued = w == DVT_USES_REG || d.dir;   // (the words a call writes are not in the records)
            out->push_back(make_def(i, w, tgt, w == DVT_USES_REG ? rec.a : d.dir ? d.after : 0, valued ? 0 : (uint32_t)DVT_USES_NO_VALUE));
        });
    }
    // definition di with its answer: its edges, the links, the new nodes
    bool resolve(uint32_t di, const Found &f, uint32_t depth) {
        dvt_uses_def &D = defs[di];
        const unsigned long long F = from[di];
        auto no = [&](unsigned long long pos, const char *what_) {
            why = "the record at shard " + std::to_string((uint32_t)(pos >> 32)) + ", row " + std::to_string((uint32_t)pos) + " is no " + what_ +
                  " of the definition asked for";
            return false;
        };
        if (f.next == NO_POS) D.flags |= DVT_USES_LIVE_AT_EXIT;
        else {
            if (f.next < F) return no(f.next, "next writer");
            D.next_shard = (uint32_t)(f.next >> 32); D.next_row = (uint32_t)f.next;
        }
        D.n_uses = f.n_uses;
        if (f.n_uses > fan) D.flags |= DVT_USES_TRUNCATED;
        if (f.uses.size() != std::min<uint64_t>(fan, f.n_uses)) {
            why = "a definition came back with " + std::to_string(f.uses.size()) + " kept uses of " + std::to_string(f.n_uses);
            return false;
        }
        D.first_edge = f.uses.empty() ? 0 : s.n_edges;
        D.n_edges = (uint32_t)f.uses.size();
        if (s.n_edges + f.uses.size() > cap_edges) { why = "more edges than the level reserved"; return false; }
        if (D.node == NONE && f.uses.empty()) D.flags |= DVT_USES_NO_VALUE;
        for (size_t k = 0; k < f.uses.size(); k++) {
            const Use &u = f.uses[k];
            const watch::Decoded d = decode(u.rec);
            if (d.bad || u.pos < F || u.pos > f.next || (k && u.pos < f.uses[k - 1].pos)) return no(u.pos, "use");
            const Reads r = reads(d, ost.words[u.rec.idx], sh, D.what, D.target, flags);
            if (!(r.n >= 1 && r.role0 == u.role) && !(r.n == 2 && r.role1 == u.role)) return no(u.pos, "use");
            if (D.node == NONE && k == 0) {   // the root's value: what its first kept use read
                if (u.role == DVT_USES_MEM) {
                    if (d.dir) D.value = d.before;
                    else D.flags |= DVT_USES_NO_VALUE;
                } else
                    D.value = u.role == DVT_USES_RS2 ? u.rec.c : u.rec.b;
            }
            dvt_uses_edge e{di, NONE, u.role, 0, (uint32_t)(u.pos >> 32), (uint32_t)u.pos};
            const auto it = node_at.find(u.pos);
            if (it != node_at.end()) e.to = it->second;
            else if (s.n_nodes >= cap_nodes) e.flags |= DVT_USES_CUT;
            else {
                e.to = s.n_nodes;
                node_at[u.pos] = s.n_nodes;
                nodes[s.n_nodes++] = flow::node_of<dvt_uses_node>(u.pos, d, u.rec, depth);
                recs.push_back(u.rec);
            }
            edges[s.n_edges++] = e;
        }
        return true;
    }
    template <class Answer>
    int run(Answer answer) {
        defs[0] = make_def(NONE, what, target, 0, 0);
        from.assign(1, P);
        s.n_defs = 1;
        std::vector<dvt_uses_def> out;
        bool full = false;
        for (uint32_t lo = 0, d = 0; lo < s.n_defs; d++) {
            const uint32_t hi = s.n_defs, node_lo = s.n_nodes;
            std::vector<Def> qs;
            for (uint32_t i = lo; i < hi; i++) qs.push_back(Def{defs[i].what, defs[i].target, from[i]});
            std::vector<Found> found(qs.size());
            if (!answer(qs, &found)) return 1;
            s.levels++;
            for (uint32_t i = lo; i < hi; i++)
                if (!resolve(i, found[i - lo], d + 1)) return 2;
            if (full) {   // the level that hit a cap is answered: the nodes its answers add stay unexpanded
                for (uint32_t i = node_lo; i < s.n_nodes; i++) nodes[i].flags |= DVT_USES_UNEXPANDED;
                break;
            }
            lo = hi;
            for (uint32_t i = node_lo; i < s.n_nodes; i++) {
                if (nodes[i].depth < max_depth && !full) {
                    outputs_of(i, &out);
                    full = s.n_defs + out.size() > cap_defs || s.n_edges + (uint64_t)(s.n_defs - lo + out.size()) * fan > cap_edges;
                }
                if (nodes[i].depth >= max_depth || full) { nodes[i].flags |= DVT_USES_UNEXPANDED; continue; }
                nodes[i].first_def = out.empty() ? 0 : s.n_defs;
                nodes[i].n_defs = (uint32_t)out.size();
                for (const dvt_uses_def &o : out) {
                    defs[s.n_defs++] = o;
                    from.push_back(watch::position(nodes[i].shard, nodes[i].row) + 1);
                }
            }
        }
        for (uint32_t i = 0; i < s.n_nodes; i++) {
            s.unexpanded += (nodes[i].flags & DVT_USES_UNEXPANDED) != 0;
            s.depth = std::max(s.depth, nodes[i].depth);
        }
        for (uint32_t i = 0; i < s.n_defs; i++) {
            s.truncated += (defs[i].flags & DVT_USES_TRUNCATED) != 0;
            s.live_at_exit += (defs[i].flags & DVT_USES_LIVE_AT_EXIT) != 0;
            s.no_value += (defs[i].flags & DVT_USES_NO_VALUE) != 0;
            s.dead += defs[i].n_uses == 0;
            s.uses_total += defs[i].n_uses;
        }
        for (uint32_t i = 0; i < s.n_edges; i++) s.cut += (edges[i].flags & DVT_USES_CUT) != 0;
        s.span = SPAN;
        return 0;
    }
};

// The host path's state: the records at and after P of the shards of an execution (flow::Keeper), and the answers by one forward
// scan per level.
struct Keeper : flow::Keeper {
    Keeper(const rv32::Program &prog, uint32_t shard, uint32_t row) : flow::Keeper(prog, shard, row, false) {}
    bool answer(const rv32::Program &prog, const std::vector<Def> &qs, std::vector<Found> *found, uint32_t flags, uint32_t fan) const {
        std::unordered_map<unsigned long long, std::vector<uint32_t>> open;   // (what, target) -> its definitions without a next writer yet
        unsigned long long min_f = NO_POS;
        for (size_t i = 0; i < qs.size(); i++) {
            open[(unsigned long long)qs[i].what << 32 | qs[i].target].push_back((uint32_t)i);
            min_f = std::min(min_f, qs[i].Q);
        }
        size_t left = qs.size();
        std::vector<unsigned long long> keys;
        for (size_t k = 0; k < kept.size() && left; k++) {
            const uint32_t shard = (uint32_t)k + 1;
            if (shard < (uint32_t)(min_f >> 32)) continue;
            for (size_t r = 0; r < kept[k].size() && left; r++) {
                const unsigned long long pos = watch::position(shard, first_row[k] + (uint32_t)r);
                if (pos < min_f) continue;
                const rv32::CycleRec &rec = kept[k][r];
                const watch::Decoded d = decode(prog, rec);
                if (d.bad) continue;
                // every (what, target) the record reads or writes
                keys.clear();
                auto key = [&](uint32_t what, uint32_t tgt) {
                    const unsigned long long kk = (unsigned long long)what << 32 | tgt;
                    if (std::find(keys.begin(), keys.end(), kk) == keys.end()) keys.push_back(kk);
                };
                const uint32_t ow = ost.words[rec.idx];
                flow::for_read(d, ow, sh, flags, true, [&](uint32_t, uint32_t what, uint32_t tgt) { key(what, tgt); });
                flow::for_written(d, sh, true, key);
                for (const unsigned long long kk : keys) {
                    const auto it = open.find(kk);
                    if (it == open.end()) continue;
                    const uint32_t what = (uint32_t)(kk >> 32), tgt = (uint32_t)kk;
                    const Reads rd = reads(d, ow, sh, what, tgt, flags);
                    const bool wr = origin::writes(d, sh, what, tgt);
                    std::vector<uint32_t> &w = it->second;
                    for (size_t q = 0; q < w.size();) {
                        Found &f = (*found)[w[q]];
                        if (qs[w[q]].Q > pos) { q++; continue; }
                        for (uint32_t u = 0; u < rd.n; u++)
                            if (f.n_uses++ < fan) f.uses.push_back(Use{pos, u ? rd.role1 : rd.role0, rec});
                        if (wr) {
                            f.next = pos;
                            w[q] = w.back();
                            w.pop_back();
                            left--;
                        } else
                            q++;
                    }
                    if (w.empty()) open.erase(it);
                }
            }
        }
        return true;
    }
};

}  // namespace uses
}  // namespace dvt
