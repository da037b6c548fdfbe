// Origins (include/dvt_prover.h: dvt_rv32_job_origin, dvt_execute_origin): where the value of a register or of a memory word
// comes from, as the backward data-flow slice over the cycle records of an execution.  Nothing is executed again: a record
// holds the value it wrote (rec.a), the values it read (rec.b, rec.c) and the word before its load or store, and the
// instruction statics and the shapes of the precompile calls say which register or word each of them is.  The rule, in plain
// C++ for both entry points (search() below; the host path answers its questions with Keeper, the job entry point with the
// kernels of origin.hip):
//
//   Positions, decode(), call_match(), the shapes and SPAN are watch.h's and snapshot.h's.  A call names a position
//   P = (shard, row), (0xffffffff, 0xffffffff) = the exit, and a target:
//       DVT_ORIGIN_REG k (1..31)                               the value x_k holds before P
//       DVT_ORIGIN_WORD addr (4-aligned, below ADDR_LIMIT)     the word before P
//
//   Question (what, target, Q): the last record before position Q that WRITES the target.
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
//   The input edges of a node depend only on its record, never on how it was reached, and come in this order:
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

#include "snapshot.h"

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

// What the kernels of origin.hip take by value (kernels.h declares the launches).  The questions of a pass are sorted
// (origin::sorts_before): q_target / q_pos [n_q], n_q <= PASS_Q; the questions of register k are [reg_off[k], reg_off[k + 1]),
// the word questions [reg_off[32], n_q); max_q = the largest position asked at.
struct OriginArgs {
    watch::Shapes sh;
    const uint32_t *statics, *offs;    // [n_instr], device
    const uint32_t *q_target;          // device
    const unsigned long long *q_pos;   // device
    uint32_t reg_off[33];
    uint32_t n_instr, text_base, shard, n_q;
    unsigned long long max_q;
};
// one record to copy out: row `row` of the shard whose records are recs
struct OriginFetch {
    const rv32::CycleRec *recs;
    uint32_t n_recs, row;
};

namespace origin {

// ---------------------------------------------------------------- host only
// What the search reads per instruction besides watch::Statics: the source registers and whether the instruction reads them.
enum : uint32_t { OS_RS1_MASK = 31, OS_RS2_SHIFT = 5, OS_RS1_EN = 1u << 10, OS_RS2_EN = 1u << 11 };
struct Statics {
    std::vector<uint32_t> words;
    explicit Statics(const rv32::Program &prog) : words(prog.instrs.size() - 1) {
        for (size_t i = 0; i < words.size(); i++) {
            const rv32::Instr &in = prog.instrs[i];
            words[i] = (in.rs1 & OS_RS1_MASK) | (in.rs2 & 31) << OS_RS2_SHIFT | (in.flags >> rv32::F_RS1_EN & 1 ? OS_RS1_EN : 0) |
                       (in.flags >> rv32::F_RS2_EN & 1 ? OS_RS2_EN : 0);
        }
    }
};

// nullptr, or what is wrong with the arguments of a call
inline const char *input_error(uint32_t what, uint32_t target, uint32_t flags, uint32_t max_depth, const dvt_origin_node *nodes, size_t cap_nodes,
                               const dvt_origin_edge *edges, size_t cap_edges, std::string *text) {
    if (what == DVT_ORIGIN_REG) {
        if (target < 1 || target > 31) return (*text = "register " + std::to_string(target) + " outside 1..31").c_str();
    } else if (what == DVT_ORIGIN_WORD) {
        if (target & 3) return (*text = "word address not 4-aligned").c_str();
        if (target >= rv32::ADDR_LIMIT) return (*text = "word address at or past the address limit").c_str();
    } else
        return (*text = "unknown target kind " + std::to_string(what)).c_str();
    if (flags & ~(uint32_t)DVT_ORIGIN_FOLLOW_ADDR) return (*text = "unknown flag").c_str();
    if (max_depth > MAX_DEPTH) return (*text = "max_depth " + std::to_string(max_depth) + " (at most " + std::to_string(MAX_DEPTH) + ")").c_str();
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

// does the record write the question's target?
inline bool writes(const watch::Decoded &d, const watch::Shapes &sh, uint32_t what, uint32_t target) {
    if (d.bad) return false;
    if (what == DVT_ORIGIN_REG) return target && (d.st & watch::ST_RD_MASK) == target;
    if (d.dir) return d.dir == DVT_WATCH_STORE && d.addr == target;
    return d.shape >= 0 && d.shape < (int)memrep::MAX_PRE && watch::call_match(sh.s[d.shape], d.a0, d.a1, target, target + 4, DVT_WATCH_PRE_WRITE).n != 0;
}

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
        const uint32_t kind = nodes[i].kind, ow = ost.words[rec.idx], rs1 = ow & OS_RS1_MASK, rs2 = ow >> OS_RS2_SHIFT & 31;
        auto add = [&](uint32_t role, uint32_t tgt, uint32_t value, uint32_t fl) { out->push_back(dvt_origin_edge{i, NONE, role, tgt, value, fl, 0, 0}); };
        const bool ecall = kind == DVT_ORIGIN_CALL || kind == DVT_ORIGIN_SYSCALL, mem = kind == DVT_ORIGIN_LOAD || kind == DVT_ORIGIN_STORE;
        if (mem) {
            if ((flags & DVT_ORIGIN_FOLLOW_ADDR) && rs1) add(DVT_ORIGIN_ADDR, rs1, rec.b, 0);
        } else if (!ecall && (ow & OS_RS1_EN) && rs1)
            add(DVT_ORIGIN_RS1, rs1, rec.b, 0);
        if (!ecall && (ow & OS_RS2_EN) && rs2) add(DVT_ORIGIN_RS2, rs2, rec.c, 0);
        if (kind == DVT_ORIGIN_LOAD || (kind == DVT_ORIGIN_STORE && (d.st & (watch::ST_HALF | watch::ST_BYTE)))) add(DVT_ORIGIN_MEM, d.addr, d.before, 0);
        if (kind == DVT_ORIGIN_CALL && d.shape >= 0 && d.shape < (int)memrep::MAX_PRE) {
            const memrep::PreShape &ps = sh.s[d.shape];
            for (uint32_t arr = 0; arr < 2; arr++) {
                const uint32_t base = arr ? d.a1 : d.a0, n = arr ? ps.n1 : ps.n0, r = arr ? ps.n1 : ps.r0;
                for (uint32_t k = 0; k < n && k < memrep::MAX_CALL_WORDS; k++)
                    if (k < r) add(DVT_ORIGIN_MEM, base + 4 * k, 0, DVT_ORIGIN_NO_VALUE);
            }
        }
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
        dvt_origin_node n{};
        n.shard = e.src_shard; n.row = e.src_row; n.pc = d.pc; n.idx = f.rec.idx; n.depth = depth;
        n.kind = d.st & watch::ST_LOAD ? DVT_ORIGIN_LOAD : d.st & watch::ST_STORE ? DVT_ORIGIN_STORE : !(d.st & watch::ST_ECALL) ? DVT_ORIGIN_OP :
                 d.shape >= 0 ? DVT_ORIGIN_CALL : DVT_ORIGIN_SYSCALL;
        n.rd_value = f.rec.a; n.rs1 = f.rec.b; n.rs2 = f.rec.c;
        if (d.dir) { n.addr = d.addr; n.before = d.before; n.after = d.after; }
        e.to = s.n_nodes;
        node_at[f.pos] = s.n_nodes;
        nodes[s.n_nodes++] = n;
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

// The host path's state: the records before P of the shards of an execution, and the answers by one backward scan per level.
struct Keeper {
    static constexpr uint64_t MAX_KEPT = (uint64_t)1 << 24;
    unsigned long long P;
    watch::Statics wst;
    watch::Shapes sh;
    std::vector<std::vector<rv32::CycleRec>> kept;   // kept[k]: the records of shard k + 1 that lie before P
    std::vector<uint64_t> shard_n;
    uint64_t cycles = 0, position = 0, bad = 0;
    bool too_many = false;
    Keeper(const rv32::Program &prog, uint32_t shard, uint32_t row) : P(watch::position(shard, row)), wst(prog), sh(watch::shapes()) {}
    watch::Decoded decode(const rv32::Program &prog, const rv32::CycleRec &rec) const {
        return watch::decode(rec, (uint32_t)wst.n(), prog.text_base, wst.statics(), wst.offs(), sh);
    }
    // the records of shard `shard` (numbered from 1, in order)
    void scan(const rv32::Program &prog, const rv32::CycleRec *recs, size_t n, uint32_t shard) {
        const uint32_t p_shard = (uint32_t)(P >> 32), p_row = (uint32_t)P;
        const size_t n_pre = shard < p_shard ? n : shard == p_shard ? std::min<size_t>(n, p_row) : 0;
        if (position + n_pre > MAX_KEPT) too_many = true;
        if (n_pre && !too_many) {
            kept.resize(shard);
            kept[shard - 1].assign(recs, recs + n_pre);
            for (size_t r = 0; r < n_pre; r++) bad += decode(prog, recs[r]).bad;
        }
        position += n_pre;
        cycles += n;
        shard_n.push_back(n);
    }
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
                if (const uint32_t rd = d.st & watch::ST_RD_MASK) offer(DVT_ORIGIN_REG, rd, pos, rec);
                if (d.dir == DVT_WATCH_STORE) offer(DVT_ORIGIN_WORD, d.addr, pos, rec);
                else if (!d.dir && d.shape >= 0 && d.shape < (int)memrep::MAX_PRE) {
                    const memrep::PreShape &ps = sh.s[d.shape];
                    for (uint32_t arr = 0; arr < 2; arr++) {
                        const uint32_t base = arr ? d.a1 : d.a0, n = arr ? ps.n1 : ps.n0, w = arr ? ps.w1 : ps.w0;
                        for (uint32_t i = 0; i < n && i < memrep::MAX_CALL_WORDS; i++)
                            if (i + w >= n) offer(DVT_ORIGIN_WORD, base + 4 * i, pos, rec);
                    }
                }
            }
        }
        return true;
    }
    // position, cycles, shard, row and shards_total of the summary
    void place(dvt_origin_summary *s) const {
        s->position = position; s->cycles = cycles;
        snap::locate(shard_n, position, &s->shard, &s->row);
        s->shards_total = (uint32_t)shard_n.size();
    }
};

}  // namespace origin
}  // namespace dvt
