// Origins (include/dvt_prover.h: dvt_rv32_job_origin, dvt_execute_origin): where the value of a register or of a memory word
// comes from, as the backward data-flow slice over the cycle records of an execution.  Nothing is executed again: a record
// holds the value it wrote (rec.a), the values it read (rec.b, rec.c) and the word before its load or store, and the
// instruction statics and the shapes of the precompile calls say which register or word each of them is.  What a record writes
// and what it reads is stated once, in dataflow.h (flow::for_written, flow::for_read), for this search, for the uses search
// (uses.h) and for the kernels of both; this header holds the search over it (Search below; the host path answers its questions
// with Keeper, the job entry point with the kernels of origin.hip):
//
//   Positions, decode(), call_match(), the shapes and SPAN are watch.h's and snapshot.h's.  A call names a position
//   P = (shard, row), (0xffffffff, 0xffffffff) = the exit, and a target:
//       DVT_ORIGIN_REG k (1..31)                               the value x_k holds before P
//       DVT_ORIGIN_WORD addr (4-aligned, below ADDR_LIMIT)     the word before P
//
//   Question (what, target, Q): the last record before position Q that WRITES the target (flow::for_written).
//       REG k    the last record with rd == k: snapshot.h's register rule, so ECALL counts as a writer of t0.
//       WORD a   the last record that is a store (sw / sh / sb) to word a, or a precompile call whose PRE_WRITE entries
//                contain a.  Loads are no writers: on purpose other than the snapshot's deciding accesses.
//       No such record: the target is INITIAL.
//
//   Node = one record.  kind: DVT_ORIGIN_LOAD, _STORE, _CALL (an ECALL with a shape), _SYSCALL (any other ECALL), _OP (any
//   other record, among them every writer of a register that is no load).  Its fields are those of a watch hit (shard, row, pc,
//   idx, rd_value = rec.a, rs1 = rec.b, rs2 = rec.c, and of a load or store addr, before, after), plus kind, depth, first_edge,
//   n_edges, flags.
//
//   The input edges of a node depend only on its record, never on how it was reached, and come in this order (flow::for_read):
//       1. ADDR    loads and stores: register rs1, value rec.b.  Only with DVT_ORIGIN_FOLLOW_ADDR; otherwise the edge is not
//                  emitted, so sp chains do not drown the slice.
//       2. RS1     every other instruction whose decode sets F_RS1_EN, except ECALL: register rs1, value rec.b.
//       3. RS2     F_RS2_EN and not ECALL (stores: the data): register rs2, value rec.c.
//       4. MEM     loads: word d.addr, value d.before.  sb / sh: the same, because the bytes they keep come from the earlier
//                  word.  sw: none.
//       5. _CALL   one MEM edge per word the call reads, in call_match order (array 0 first, then array 1): an array-0 word
//                  is read when its index k < r0, every array-1 word is read.  Value 0 with NO_VALUE.
//       6. _SYSCALL  none.
//   An edge whose register is x0 is not emitted.
//
//   Edge = {from, to, role, target, value, flags, src_shard, src_row}.  Its question is (REG for ADDR / RS1 / RS2 or WORD for
//   MEM, target, the position of node `from`).  flags: INITIAL (no writer, to = NONE), IMAGE (an INITIAL word that lies in the
//   program image), NO_VALUE, CUT (the writer exists and its position is in src_*, but the node cap was reached; to = NONE).
//   src_* is filled whenever a writer exists.
//   Edge 0 is the root: from = NONE, role ROOT, its question is (what, target, P).  Its value: REG: the writer's rec.a, or 0
//   with INITIAL.  WORD: the writer is a store: its `after`; a call: NO_VALUE; no writer: the image word with INITIAL | IMAGE,
//   else INITIAL | NO_VALUE.
//
//   Search.  The order is discovery order, so that both entry points run it identically.  Level 0 is the root's writer.  For
//   level d, go through its nodes in order: if d == max_depth the node is UNEXPANDED with n_edges = 0; otherwise its edges are
//   appended, and if they would exceed cap_edges this node and every later node is UNEXPANDED and the search ends after this
//   level's answers (the nodes those answers add are UNEXPANDED too).  Then all questions of the level are answered and the
//   edges resolved in order: the writer is already a node: link to it; else, if n_nodes < cap_nodes, a new node at depth
//   d + 1; else CUT.
//
//   Limits: DVT_ORIGIN_MAX_NODES 1024, DVT_ORIGIN_MAX_EDGES 8192, DVT_ORIGIN_MAX_DEPTH 64, DVT_ORIGIN_PASS_QUESTIONS 256 (the
//   questions of one device pass: a wider level takes ceil(q / 256) passes).
//
//   summary: n_nodes, n_edges, depth (the deepest node's); cut, unexpanded, initial, no_value (edges, nodes, edges, edges);
//   questions, levels (answered, the root's among them), passes (0 on the host path); position, cycles, shard, row as the
//   snapshot's; shards_total, span, ms.
//
// A bad record (watch.h's bad) anywhere before P fails the call with DVT_ERR_INPUT, as in the snapshot.
// What the slice cannot say: the values of the words a call read or wrote are not in the records; a hinted word nothing wrote
// is INITIAL, as in snapshot.h; it follows data dependence only, no control dependence.
#pragma once
#include <map>
#include <string>
#include <unordered_map>

#include "dataflow.h"

namespace dvt {
namespace origin {

constexpr uint32_t SPAN = DVT_ORIGIN_SPAN, MAX_NODES = DVT_ORIGIN_MAX_NODES, MAX_EDGES = DVT_ORIGIN_MAX_EDGES, MAX_DEPTH = DVT_ORIGIN_MAX_DEPTH,
                   PASS_Q = DVT_ORIGIN_PASS_QUESTIONS, NONE = DVT_ORIGIN_NONE;

// the last record before Q that writes `target` (a register number or a word address, by `what`)
struct Question {
    uint32_t what, target;
    unsigned long long Q;
};
// the order a device pass takes its questions in: the register questions by register, then the word questions by address
inline bool sorts_before(const Question &a, const Question &b) {
    return a.what != b.what ? a.what < b.what : a.target != b.target ? a.target < b.target : a.Q < b.Q;
}

}  // namespace origin

// What the reduce pass of origin.hip takes by value (kernels.h declares the launches): the sorted questions of a pass (PassArgs,
// dataflow.h) and max_q = the largest position asked at
struct OriginArgs : PassArgs {
    unsigned long long max_q;
};
// one record to copy out: row `row` of the shard whose records are recs
struct OriginFetch {
    const rv32::CycleRec *recs;
    uint32_t n_recs, row;
};

namespace origin {

// ---------------------------------------------------------------- host only
using flow::Statics;
using flow::writes;

// nullptr, or what is wrong with the arguments of a call
inline const char *input_error(uint32_t what, uint32_t target, uint32_t flags, uint32_t max_depth, const dvt_origin_node *nodes, size_t cap_nodes,
                               const dvt_origin_edge *edges, size_t cap_edges, std::string *text) {
    if (const char *why = flow::target_error(what, target, flags, max_depth, MAX_DEPTH, text)) return why;
    if (cap_nodes > MAX_NODES) return (*text = "cap_nodes " + std::to_string(cap_nodes) + " (at most " + std::to_string(MAX_NODES) + ")").c_str();
    if (!cap_edges || cap_edges > MAX_EDGES) return (*text = "cap_edges " + std::to_string(cap_edges) + " (1.." + std::to_string(MAX_EDGES) + ")").c_str();
    if (!edges || (cap_nodes && !nodes)) return (*text = "null array").c_str();
    return nullptr;
}

// the answer to a question: the writer's position (0: no writer; every position has shard >= 1) and its record
struct Found {
    unsigned long long pos;
    rv32::CycleRec rec;
};

// The search of the rule, for both entry points.  answer(questions, &found) fills found[i] for questions[i] and returns false
// when it could not (the caller knows why).  Returns 0, 1 when answer failed, 2 when an answer is no writer of its target
// (*why says which).  The counters of the summary are filled; position, cycles, shard, row, shards_total, passes and ms are
// the caller's.
struct Search {
    const rv32::Program &prog;
    const watch::Statics &wst;
    const watch::Shapes &sh;
    Statics ost;
    unsigned long long P;
    uint32_t what, target, flags, max_depth;
    dvt_origin_node *nodes;
    size_t cap_nodes;
    dvt_origin_edge *edges;
    size_t cap_edges;
    dvt_origin_summary s{};
    std::vector<rv32::CycleRec> recs;                    // of the nodes
    std::map<unsigned long long, uint32_t> node_at;      // position -> node
    std::string why;

    Search(const rv32::Program &prog, const watch::Statics &wst, const watch::Shapes &sh, unsigned long long P, uint32_t what, uint32_t target, uint32_t flags,
           uint32_t max_depth, dvt_origin_node *nodes, size_t cap_nodes, dvt_origin_edge *edges, size_t cap_edges)
        : prog(prog), wst(wst), sh(sh), ost(prog), P(P), what(what), target(target), flags(flags), max_depth(max_depth), nodes(nodes),
          cap_nodes(cap_nodes), edges(edges), cap_edges(cap_edges) {}

    watch::Decoded decode(const rv32::CycleRec &rec) const {
        return watch::decode(rec, (uint32_t)wst.n(), prog.text_base, wst.statics(), wst.offs(), sh);
    }
    Question question_of(const dvt_origin_edge &e) const {
        if (e.from == NONE) return Question{what, target, P};
        return Question{e.role == DVT_ORIGIN_MEM ? (uint32_t)DVT_ORIGIN_WORD : (uint32_t)DVT_ORIGIN_REG, e.target, watch::position(nodes[e.from].shard, nodes[e.from].row)};
    }
    // the input edges of node i, in the rule's order
    void inputs_of(uint32_t i, std::vector<dvt_origin_edge> *out) const {
        out->clear();
        const rv32::CycleRec &rec = recs[i];
        const watch::Decoded d = decode(rec);
        flow::for_read(d, ost.words[rec.idx], sh, flags, true, [&](uint32_t role, uint32_t, uint32_t tgt) {
            const uint32_t value = role == DVT_ORIGIN_RS2 ? rec.c : role != DVT_ORIGIN_MEM ? rec.b : d.dir ? d.before : 0;
            out->push_back(dvt_origin_edge{i, NONE, role, tgt, value, role == DVT_ORIGIN_MEM && !d.dir ? (uint32_t)DVT_ORIGIN_NO_VALUE : 0, 0, 0});
        });
    }
    // edge e with its answer: the link, the new node or the leaf
    bool resolve(uint32_t ei, const Found &f, uint32_t depth) {
        dvt_origin_edge &e = edges[ei];
        const Question q = question_of(e);
        const bool root = e.from == NONE;
        if (!f.pos) {
            e.flags |= DVT_ORIGIN_INITIAL;
            const uint32_t *iw = q.what == DVT_ORIGIN_WORD ? snap::image_word(prog, q.target) : nullptr;
            if (iw) e.flags |= DVT_ORIGIN_IMAGE;
            if (root && q.what == DVT_ORIGIN_WORD) {
                if (iw) e.value = *iw;
                else e.flags |= DVT_ORIGIN_NO_VALUE;
            }
            return true;
        }
        const watch::Decoded d = decode(f.rec);
        e.src_shard = (uint32_t)(f.pos >> 32); e.src_row = (uint32_t)f.pos;
        if (f.pos >= q.Q || !writes(d, sh, q.what, q.target)) {
            why = "the record at shard " + std::to_string(e.src_shard) + ", row " + std::to_string(e.src_row) + " is no writer of the target asked for";
            return false;
        }
        if (root) {
            if (q.what == DVT_ORIGIN_REG) e.value = f.rec.a;
            else if (d.dir) e.value = d.after;
            else e.flags |= DVT_ORIGIN_NO_VALUE;
        }
        const auto it = node_at.find(f.pos);
        if (it != node_at.end()) { e.to = it->second; return true; }
        if (s.n_nodes >= cap_nodes) { e.flags |= DVT_ORIGIN_CUT; return true; }
        e.to = s.n_nodes;
        node_at[f.pos] = s.n_nodes;
        nodes[s.n_nodes++] = flow::node_of<dvt_origin_node>(f.pos, d, f.rec, depth);
        recs.push_back(f.rec);
        return true;
    }
    // the questions of edges [lo, n_edges) answered and resolved; the nodes they add have depth `depth`
    template <class Answer>
    int answer_level(uint32_t lo, uint32_t depth, Answer &answer) {
        std::vector<Question> qs;
        for (uint32_t ei = lo; ei < s.n_edges; ei++) qs.push_back(question_of(edges[ei]));
        std::vector<Found> found(qs.size(), Found{});
        if (!answer(qs, &found)) return 1;
        s.levels++;
        s.questions += (uint32_t)qs.size();
        for (uint32_t ei = lo; ei < s.n_edges; ei++)
            if (!resolve(ei, found[ei - lo], depth)) return 2;
        return 0;
    }
    template <class Answer>
    int run(Answer answer) {
        edges[0] = dvt_origin_edge{NONE, NONE, DVT_ORIGIN_ROOT, target, 0, 0, 0, 0};
        s.n_edges = 1;
        if (int rc = answer_level(0, 0, answer)) return rc;
        std::vector<dvt_origin_edge> in;
        uint32_t lo = 0, hi = s.n_nodes;
        for (uint32_t d = 0; lo < hi; d++) {
            const uint32_t first = s.n_edges;
            bool full = false;
            for (uint32_t i = lo; i < hi; i++) {
                if (d < max_depth && !full) {
                    inputs_of(i, &in);
                    full = s.n_edges + in.size() > cap_edges;
                }
                if (d >= max_depth || full) { nodes[i].flags |= DVT_ORIGIN_UNEXPANDED; continue; }
                nodes[i].first_edge = in.empty() ? 0 : s.n_edges;
                nodes[i].n_edges = (uint32_t)in.size();
                for (const dvt_origin_edge &e : in) edges[s.n_edges++] = e;
            }
            if (s.n_edges == first) break;
            if (int rc = answer_level(first, d + 1, answer)) return rc;
            lo = hi; hi = s.n_nodes;
            if (full) {
                for (uint32_t i = lo; i < hi; i++) nodes[i].flags |= DVT_ORIGIN_UNEXPANDED;
                break;
            }
        }
        for (uint32_t i = 0; i < s.n_nodes; i++) {
            s.unexpanded += (nodes[i].flags & DVT_ORIGIN_UNEXPANDED) != 0;
            s.depth = std::max(s.depth, nodes[i].depth);
        }
        for (uint32_t ei = 0; ei < s.n_edges; ei++) {
            s.cut += (edges[ei].flags & DVT_ORIGIN_CUT) != 0;
            s.initial += (edges[ei].flags & DVT_ORIGIN_INITIAL) != 0;
            s.no_value += (edges[ei].flags & DVT_ORIGIN_NO_VALUE) != 0;
        }
        s.span = SPAN;
        return 0;
    }
};

// The host path's state: the records before P of the shards of an execution (flow::Keeper), and the answers by one backward
// scan per level.
struct Keeper : flow::Keeper {
    Keeper(const rv32::Program &prog, uint32_t shard, uint32_t row) : flow::Keeper(prog, shard, row, true) {}
    bool answer(const rv32::Program &prog, const std::vector<Question> &qs, std::vector<Found> *found) const {
        std::unordered_map<unsigned long long, std::vector<uint32_t>> waiting;   // (what, target) -> its questions
        unsigned long long max_q = 0;
        for (size_t i = 0; i < qs.size(); i++) {
            waiting[(unsigned long long)qs[i].what << 32 | qs[i].target].push_back((uint32_t)i);
            max_q = std::max(max_q, qs[i].Q);
        }
        size_t left = qs.size();
        auto offer = [&](uint32_t what, uint32_t tgt, unsigned long long pos, const rv32::CycleRec &rec) {
            const auto it = waiting.find((unsigned long long)what << 32 | tgt);
            if (it == waiting.end()) return;
            std::vector<uint32_t> &w = it->second;
            for (size_t k = 0; k < w.size();) {
                if (qs[w[k]].Q > pos) {
                    (*found)[w[k]] = Found{pos, rec};
                    w[k] = w.back();
                    w.pop_back();
                    left--;
                } else
                    k++;
            }
            if (w.empty()) waiting.erase(it);
        };
        const uint32_t q_shard = (uint32_t)(max_q >> 32), q_row = (uint32_t)max_q;
        for (size_t k = std::min<size_t>(kept.size(), q_shard); k-- > 0 && left;) {
            const std::vector<rv32::CycleRec> &recs = kept[k];
            const uint32_t shard = (uint32_t)k + 1;
            for (size_t r = shard == q_shard ? std::min<size_t>(recs.size(), q_row) : recs.size(); r-- > 0 && left;) {
                const rv32::CycleRec &rec = recs[r];
                const watch::Decoded d = decode(prog, rec);
                if (d.bad) continue;
                const unsigned long long pos = watch::position(shard, (uint32_t)r);
                flow::for_written(d, sh, true, [&](uint32_t what, uint32_t tgt) { offer(what, tgt, pos, rec); });
            }
        }
        return true;
    }
};

}  // namespace origin
}  // namespace dvt
