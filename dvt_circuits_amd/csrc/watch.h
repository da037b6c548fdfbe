// Watchpoints (include/dvt_prover.h: dvt_rv32_job_watch, dvt_execute_watch): which records of an execution ran a pc, wrote a
// register or accessed a word, with what values, and in what order; from the cycle records of the execution.  The rule, in
// plain C++ for the host path (scan_records) and, through the same decode() and test(), for the kernels of watch.hip over
// the records a prepared job holds in HBM:
//
//   A call carries 1..DVT_WATCH_MAX_QUERIES queries.  Every record is tested against every query and is a hit of a query at
//   most once.  A query has a kind, lo, hi, flags, mask, want and a window.
//
//   DVT_WATCH_PC.   pc = text_base + 4 rec.idx lies in [lo, hi).
//   DVT_WATCH_REG.  The instruction has rd == lo, lo in 1..31 (x0 never hits).  The value is rec.a.  With DVT_WATCH_VALUE the
//                   hit also requires (value & mask) == (want & mask).  (ECALL is decoded with rd = t0 and writes t0 back.)
//   DVT_WATCH_MEM.  A memory access in the sense of memreport.h whose word address lies in [lo, hi); the registers and the
//                   a1 port read of COMMIT and the precompile ECALLs are never accesses.  flags selects among LOAD, STORE,
//                   PRE_READ and PRE_WRITE.
//     loads and stores   the word is (rec.b + instr.off) & ~3, before = rec.m_prev.  A load: after = before.  A store: rec.c
//                        is the rs2 value (the executor's PORT_C, fill_cpu_row's c, the model's c: all three read rs2 on
//                        sb sh sw, and 0 on loads); after = rec.c for sw, and for sh / sb the low half / byte of rec.c merged
//                        into before at byte offset (rec.b + instr.off) & 3.  DVT_WATCH_VALUE tests `after`.
//     precompile calls   id = rec.b, a0 = rec.c, a1 = rec.m_prev and the shapes of memrep::pre_shapes(), as in memreport.h.
//                        A word of array 0 is a read when its index is below r0 and a write when it is among the last w0; a
//                        word of array 1 is a read, and a write when among the last w1.  The call hits when any entry of
//                        its arrays lies in [lo, hi) with a selected direction: ONE hit per call, addr = the lowest such
//                        word, n_words = the number of such entries, flags = the selected directions found.  The values of
//                        the words are not in the records: before = after = 0, the hit carries DVT_WATCH_HIT_NO_VALUE, and
//                        a query with DVT_WATCH_VALUE never matches a call.
//   Window.  Only positions from <= (shard, row) < to, compared lexicographically, are searched.  shard = ShardJob::index (from
//            1), row = the record's index within its shard = the row of the shard's cpu table = clk / 4 - 1 of the row's
//            timestamps.
//
//   A hit (dvt_watch_hit): query, shard, row, pc, idx, kind (the query's), rd_value = rec.a, rs1 = rec.b, rs2 = rec.c; and for a
//   load or a store, whatever the kind of the query: flags = LOAD or STORE, addr, n_words = 1, before, after and the previous
//   access of the word (prev_shard, prev_clk) = (rec.sh_cm >> 16, rec.m_ts), (0, 0) on a first touch.  Under a PC or REG query a
//   precompile call carries no access fields (they are relative to a range); every field not named is 0.
//
//   Per query: total = the exact number of hits, and the first and the last min(K, total) of them in execution order (shards
//   by number, rows ascending), K = cap_each <= DVT_WATCH_MAX_KEEP.
//
// A record the executor never writes (idx outside the text; a load, store or call whose address lies outside guest memory)
// hits nothing and is counted as bad: the call fails with DVT_ERR_INPUT.
#pragma once
#include <string>

#include "memreport.h"

namespace dvt {
namespace watch {

constexpr uint32_t SPAN = DVT_WATCH_SPAN, MAX_Q = DVT_WATCH_MAX_QUERIES, MAX_KEEP = DVT_WATCH_MAX_KEEP;
constexpr uint32_t DIRECTIONS = DVT_WATCH_LOAD | DVT_WATCH_STORE | DVT_WATCH_PRE_READ | DVT_WATCH_PRE_WRITE;

// What the passes read per instruction besides the records: rd, the class bits of memreport.h and the width of a store; and
// the address offset.
enum : uint32_t { ST_RD_MASK = 31, ST_LOAD = 1u << 5, ST_STORE = 1u << 6, ST_ECALL = 1u << 7, ST_HALF = 1u << 8, ST_BYTE = 1u << 9 };
inline uint32_t instr_static(const rv32::Instr &in) {
    const uint32_t cls = memrep::instr_class(in);
    return (in.rd & ST_RD_MASK) | (cls & memrep::CLS_LOAD ? ST_LOAD : 0) | (cls & memrep::CLS_STORE ? ST_STORE : 0) | (cls & memrep::CLS_ECALL ? ST_ECALL : 0) |
           (in.kind == rv32::K_SH ? ST_HALF : 0) | (in.kind == rv32::K_SB ? ST_BYTE : 0);
}
// Host only: both of a program, [statics | offs] in one piece, as the device passes take them in one upload.
struct Statics {
    std::vector<uint32_t> words;
    explicit Statics(const rv32::Program &prog) : words(2 * (prog.instrs.size() - 1)) {
        for (size_t i = 0; i < n(); i++) {
            words[i] = instr_static(prog.instrs[i]);
            words[n() + i] = prog.instrs[i].off;
        }
    }
    size_t n() const { return words.size() / 2; }   // n_instr
    size_t bytes() const { return words.size() * 4; }
    const uint32_t *statics() const { return words.data(); }
    const uint32_t *offs() const { return words.data() + n(); }
};

// The shapes of the precompile calls as the passes take them (by value on the device): the rows of memrep::pre_shapes().
struct Shapes {
    uint32_t n;
    memrep::PreShape s[memrep::MAX_PRE];
};
inline Shapes shapes() {
    Shapes out{};
    for (const memrep::PreShape &s : memrep::pre_shapes())
        if (out.n < memrep::MAX_PRE) out.s[out.n++] = s;
    return out;
}

// A record, decoded once for all queries.
struct Decoded {
    uint32_t st;          // the instruction's static word; 0 with bad set
    uint32_t pc;
    uint32_t dir;         // DVT_WATCH_LOAD or _STORE of a load / store, else 0
    uint32_t addr, before, after;
    int shape;            // of a precompile call: its row of Shapes, else -1
    uint32_t a0, a1;      // of a precompile call (word aligned)
    bool bad;             // a record the executor never writes
};

DVT_HD Decoded decode(const rv32::CycleRec &rec, uint32_t n_instr, uint32_t text_base, const uint32_t *statics, const uint32_t *offs, const Shapes &sh) {
    Decoded d{};
    d.shape = -1;
    if (rec.idx >= n_instr) { d.bad = true; return d; }
    d.st = statics[rec.idx];
    d.pc = text_base + 4 * rec.idx;
    if (d.st & (ST_LOAD | ST_STORE)) {
        const uint32_t byte_addr = rec.b + offs[rec.idx], s8 = 8 * (byte_addr & 3);
        d.addr = byte_addr & ~3u;
        if (d.addr >= rv32::ADDR_LIMIT) { d.bad = true; d.st = 0; return d; }
        d.before = d.after = rec.m_prev;
        d.dir = DVT_WATCH_LOAD;
        if (d.st & ST_STORE) {
            d.dir = DVT_WATCH_STORE;
            const uint32_t m = d.st & ST_BYTE ? 0xffu << s8 : d.st & ST_HALF ? 0xffffu << s8 : 0xffffffffu;
            d.after = (rec.m_prev & ~m) | ((d.st & (ST_BYTE | ST_HALF) ? rec.c << s8 : rec.c) & m);
        }
    } else if (d.st & ST_ECALL) {
        for (uint32_t k = 0; k < sh.n && k < memrep::MAX_PRE; k++) {
            if (sh.s[k].id != rec.b) continue;
            d.a0 = rec.c & ~3u;
            d.a1 = rec.m_prev & ~3u;
            if (sh.s[k].n0 + sh.s[k].n1 > memrep::MAX_CALL_WORDS || (unsigned long long)d.a0 + 4 * sh.s[k].n0 > rv32::ADDR_LIMIT ||
                (unsigned long long)d.a1 + 4 * sh.s[k].n1 > rv32::ADDR_LIMIT) { d.bad = true; d.st = 0; return d; }
            d.shape = (int)k;
            break;
        }
    }
    return d;
}

// What a precompile call has in [lo, hi) with the directions of `flags`: the number of entries, the lowest word, the directions.
struct CallMatch { uint32_t n, addr, dirs; };
DVT_HD CallMatch call_match(const memrep::PreShape &s, uint32_t a0, uint32_t a1, uint32_t lo, uint32_t hi, uint32_t flags) {
    CallMatch m{0, 0xffffffffu, 0};
    memrep::for_call_words(s, a0, a1, [&](uint32_t addr, bool read, bool written) {
        if (addr < lo || addr >= hi) return;
        const uint32_t dirs = ((read ? DVT_WATCH_PRE_READ : 0) | (written ? DVT_WATCH_PRE_WRITE : 0)) & flags;
        if (!dirs) return;
        m.n++;
        m.dirs |= dirs;
        if (addr < m.addr) m.addr = addr;
    });
    return m;
}

DVT_HD unsigned long long position(uint32_t shard, uint32_t row) { return (unsigned long long)shard << 32 | row; }

// Is the record at (shard, row) a hit of q?  cm: of a MEM hit of a precompile call, what matched.
DVT_HD bool test(const dvt_watch_query &q, const Decoded &d, const rv32::CycleRec &rec, uint32_t shard, uint32_t row, const Shapes &sh, CallMatch *cm) {
    if (d.bad) return false;
    const unsigned long long pos = position(shard, row);
    if (pos < position(q.from_shard, q.from_row) || pos >= position(q.to_shard, q.to_row)) return false;
    switch (q.kind) {
    case DVT_WATCH_PC: return d.pc >= q.lo && d.pc < q.hi;
    case DVT_WATCH_REG:
        if ((d.st & ST_RD_MASK) != q.lo || !q.lo) return false;
        return !(q.flags & DVT_WATCH_VALUE) || ((rec.a ^ q.want) & q.mask) == 0;
    case DVT_WATCH_MEM:
        if (d.dir) {
            if (!(d.dir & q.flags) || d.addr < q.lo || d.addr >= q.hi) return false;
            return !(q.flags & DVT_WATCH_VALUE) || ((d.after ^ q.want) & q.mask) == 0;
        }
        if (d.shape < 0 || (q.flags & DVT_WATCH_VALUE) || !(q.flags & (DVT_WATCH_PRE_READ | DVT_WATCH_PRE_WRITE))) return false;
        *cm = call_match(sh.s[d.shape], d.a0, d.a1, q.lo, q.hi, q.flags);
        return cm->n != 0;
    }
    return false;
}

// the hit of query qi at (shard, row), once test() said so
DVT_HD dvt_watch_hit make_hit(uint32_t qi, const dvt_watch_query &q, const Decoded &d, const rv32::CycleRec &rec, uint32_t shard, uint32_t row, const CallMatch &cm) {
    dvt_watch_hit h{};
    h.query = qi; h.shard = shard; h.row = row; h.pc = d.pc; h.idx = rec.idx; h.kind = q.kind;
    h.rd_value = rec.a; h.rs1 = rec.b; h.rs2 = rec.c;
    if (d.dir) {
        h.flags = d.dir; h.addr = d.addr; h.n_words = 1; h.before = d.before; h.after = d.after;
        h.prev_shard = rec.sh_cm >> 16; h.prev_clk = rec.m_ts;
    } else if (q.kind == DVT_WATCH_MEM) {
        h.flags = cm.dirs | DVT_WATCH_HIT_NO_VALUE; h.addr = cm.addr; h.n_words = cm.n;
    }
    return h;
}

// The kept slots of one query, given its total: rank r < first_end goes to slot r of the first list, rank r >= last_begin to
// slot r - last_begin of the last list.
struct Keep {
    unsigned long long first_end, last_begin;
};
DVT_HD Keep keep_of(unsigned long long total, uint32_t K) {
    const unsigned long long k = total < K ? total : K;
    return Keep{k, total - k};
}

}  // namespace watch

// What the kernels of watch.hip take by value (kernels.h declares the launches).
struct WatchArgs {
    dvt_watch_query q[DVT_WATCH_MAX_QUERIES];
    watch::Shapes sh;
    const uint32_t *statics, *offs;   // [n_instr], device
    uint32_t n_instr, text_base, n_queries, shard;
};
struct WatchEmitArgs {
    unsigned long long base[DVT_WATCH_MAX_QUERIES], total[DVT_WATCH_MAX_QUERIES];
    uint32_t cap_each;
};

namespace watch {

// ---------------------------------------------------------------- host only
// nullptr, or what is wrong with the queries of a call
inline const char *input_error(const dvt_watch_query *q, size_t n, size_t cap_each, const dvt_watch_hit *hits, const uint64_t *totals, std::string *text) {
    auto say = [&](size_t i, const char *what) { *text = "query " + std::to_string(i) + ": " + what; return text->c_str(); };
    if (!n || n > MAX_Q) return (*text = "n_queries " + std::to_string(n) + " (1.." + std::to_string(MAX_Q) + ")").c_str();
    if (cap_each > MAX_KEEP) return (*text = "cap_each " + std::to_string(cap_each) + " (at most " + std::to_string(MAX_KEEP) + ")").c_str();
    if (!q || !totals || (cap_each && !hits)) return (*text = "null array").c_str();
    for (size_t i = 0; i < n; i++) {
        uint32_t allowed = 0;
        if (q[i].kind == DVT_WATCH_PC) allowed = 0;
        else if (q[i].kind == DVT_WATCH_REG) allowed = DVT_WATCH_VALUE;
        else if (q[i].kind == DVT_WATCH_MEM) allowed = DIRECTIONS | DVT_WATCH_VALUE;
        else return say(i, "unknown kind");
        if (q[i].flags & ~allowed) return say(i, "a flag the kind does not take");
        if (q[i].kind == DVT_WATCH_MEM && !(q[i].flags & DIRECTIONS)) return say(i, "a memory query selects at least one of LOAD, STORE, PRE_READ, PRE_WRITE");
        if (q[i].kind == DVT_WATCH_REG) {
            if (q[i].lo < 1 || q[i].lo > 31) return say(i, "register outside 1..31");
        } else if (q[i].lo >= q[i].hi) return say(i, "lo >= hi");
        if (position(q[i].from_shard, q[i].from_row) >= position(q[i].to_shard, q[i].to_row)) return say(i, "from >= to");
    }
    return nullptr;
}

// The host path's state: per query the total, the first K hits and a ring of the last K.
struct Search {
    std::vector<dvt_watch_query> queries;
    uint32_t K;
    Statics st;
    Shapes sh;
    std::vector<uint64_t> total;
    std::vector<std::vector<dvt_watch_hit>> first, ring;
    uint64_t cycles = 0, bad = 0;
    uint32_t shards = 0;
    Search(const rv32::Program &prog, const dvt_watch_query *q, size_t n, uint32_t cap_each)
        : queries(q, q + n), K(cap_each), st(prog), sh(shapes()), total(n, 0), first(n), ring(n) {
        for (auto &r : ring) r.resize(K);
    }
};

// the records of shard `shard` (numbered from 1), in execution order
inline void scan_records(const rv32::Program &prog, const rv32::CycleRec *recs, size_t n, uint32_t shard, Search *s) {
    const uint32_t n_instr = (uint32_t)s->st.n();
    for (size_t r = 0; r < n; r++) {
        const Decoded d = decode(recs[r], n_instr, prog.text_base, s->st.statics(), s->st.offs(), s->sh);
        if (d.bad) { s->bad++; continue; }
        for (size_t qi = 0; qi < s->queries.size(); qi++) {
            CallMatch cm{};
            if (!test(s->queries[qi], d, recs[r], shard, (uint32_t)r, s->sh, &cm)) continue;
            if (s->K) {
                const dvt_watch_hit h = make_hit((uint32_t)qi, s->queries[qi], d, recs[r], shard, (uint32_t)r, cm);
                if (s->total[qi] < s->K) s->first[qi].push_back(h);
                s->ring[qi][s->total[qi] % s->K] = h;
            }
            s->total[qi]++;
        }
    }
    s->cycles += n;
    s->shards++;
}

inline void emit(const rv32::Program &prog, const Search &s, uint32_t shards_total, double ms, dvt_watch_hit *hits, uint64_t *totals, dvt_watch_summary *summary) {
    for (size_t qi = 0; qi < s.queries.size(); qi++) {
        totals[qi] = s.total[qi];
        const Keep k = keep_of(s.total[qi], s.K);
        for (size_t i = 0; i < s.first[qi].size(); i++) hits[2 * qi * s.K + i] = s.first[qi][i];
        for (unsigned long long r = k.last_begin; r < s.total[qi]; r++) hits[(2 * qi + 1) * s.K + (r - k.last_begin)] = s.ring[qi][r % s.K];
    }
    dvt_watch_summary out{};
    out.cycles = s.cycles;
    out.n_queries = (uint32_t)s.queries.size();
    out.cap_each = s.K;
    out.shards_searched = s.shards;
    out.shards_total = shards_total;
    out.text_base = prog.text_base;
    out.n_instr = (uint32_t)s.st.n();
    out.span = SPAN;
    out.ms = (float)ms;
    *summary = out;
}

}  // namespace watch
}  // namespace dvt
