// Stand-alone driver of the uses search's host rule (csrc/uses.h) for AddressSanitizer / UBSan, on the CPU:
//   make -C dvt_circuits_amd/csrc asan-uses && build/asan/uses_host GUEST.elf [STDIN.bin ...]
// Runs the guest in trace mode (rv32::execute, shards of 2^12 cycles), feeds every shard's cycle records to uses::Keeper and
// runs uses::Search at seven positions (the first record, span and shard edges, the middle, the end in two spellings) for
// every register, for the first and last words the executor lists, with and without FOLLOW_ADDR, at the full limits and at
// small ones (depth 3, 7 nodes, 9 definitions, 20 edges, fan 2; depth 0 with no node); then does the same over the records
// with their fields overwritten by a fixed pseudo-random stream (instruction indices outside the text, addresses outside guest
// memory, unknown syscall ids, call arrays that leave guest memory), which the rule must skip as bad or follow like any other
// record without reading or writing out of bounds.  Exit code 0 when, on the records as executed,
//   every consumer with a node reads, in the role of its edge, the value of its definition (rs1, rs2, or `before` of a load or
//   store), every consumer lies at or after its definition's record and at or before the definition's next writer, every index
//   lies inside the arrays, the limits asked for hold, n_edges = min(fan, n_uses) for every definition, and the two spellings
//   of the end give equal answers (one dead definition that is live at the exit).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>

#include "../../dvt_circuits_amd/csrc/uses.h"

using namespace dvt;

static bool read_file(const char *path, std::vector<uint8_t> *out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    out->assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}

struct Limits { uint32_t depth, fan; size_t nodes, defs, edges; };
struct Answer {
    std::vector<dvt_uses_node> nodes;
    std::vector<dvt_uses_def> defs;
    std::vector<dvt_uses_edge> edges;
    dvt_uses_summary s;
    uint64_t bad;
    int rc;
};

static void slice(const rv32::Program &prog, const std::vector<std::vector<rv32::CycleRec>> &shards, uint32_t shard, uint32_t row, uint32_t what, uint32_t target,
                  uint32_t flags, const Limits &l, Answer *out) {
    uses::Keeper k(prog, shard, row);
    for (size_t i = 0; i < shards.size(); i++) k.scan(prog, shards[i].data(), shards[i].size(), (uint32_t)i + 1);
    out->nodes.assign(l.nodes + 1, dvt_uses_node{});
    out->defs.assign(l.defs, dvt_uses_def{});
    out->edges.assign(l.edges, dvt_uses_edge{});
    uses::Search search(prog, k.wst, k.sh, k.P, what, target, flags, l.depth, l.fan, out->nodes.data(), l.nodes, out->defs.data(), l.defs, out->edges.data(),
                        l.edges);
    out->rc = search.run([&](const std::vector<uses::Def> &qs, std::vector<uses::Found> *found) { return k.answer(prog, qs, found, flags, l.fan); });
    k.place(&search.s);
    out->s = search.s;
    out->bad = k.bad;
    out->nodes.resize(out->s.n_nodes);
    out->defs.resize(out->s.n_defs);
    out->edges.resize(out->s.n_edges);
}

// the laws that hold on any records; exact: also the ones that hold on records as executed
static bool lawful(const Answer &a, const Limits &l, bool exact) {
    bool good = a.rc == 0 && a.s.n_nodes <= l.nodes && a.s.n_defs <= l.defs && a.s.n_defs >= 1 && a.s.n_edges <= l.edges;
    uint64_t total = 0;
    for (const dvt_uses_node &n : a.nodes) good = good && n.depth >= 1 && (size_t)n.first_def + n.n_defs <= a.defs.size() && (n.depth < l.depth || !n.n_defs);
    for (size_t i = 0; i < a.defs.size() && good; i++) {
        const dvt_uses_def &d = a.defs[i];
        good = good && (d.node == DVT_USES_NONE ? i == 0 : d.node < a.nodes.size()) && (size_t)d.first_edge + d.n_edges <= a.edges.size() &&
               d.n_edges == std::min<uint64_t>(l.fan, d.n_uses) && ((d.flags & DVT_USES_TRUNCATED) != 0) == (d.n_uses > l.fan) &&
               ((d.flags & DVT_USES_LIVE_AT_EXIT) != 0) == (d.next_shard == DVT_USES_NONE);
        total += d.n_uses;
    }
    good = good && total == a.s.uses_total;
    for (size_t i = 0; i < a.edges.size() && good; i++) {
        const dvt_uses_edge &e = a.edges[i];
        good = good && e.def < a.defs.size() && (e.to == DVT_USES_NONE ? (e.flags & DVT_USES_CUT) != 0 : e.to < a.nodes.size()) && e.role >= DVT_USES_ADDR &&
               e.role <= DVT_USES_MEM;
        if (!good) break;
        const dvt_uses_def &d = a.defs[e.def];
        const unsigned long long at = watch::position(e.dst_shard, e.dst_row);
        if (d.node != DVT_USES_NONE) good = good && at > watch::position(a.nodes[d.node].shard, a.nodes[d.node].row);
        if (d.next_shard != DVT_USES_NONE) good = good && at <= watch::position(d.next_shard, d.next_row);
        if (e.to == DVT_USES_NONE) continue;
        const dvt_uses_node &to = a.nodes[e.to];
        good = good && to.shard == e.dst_shard && to.row == e.dst_row;
        if (!exact || (d.flags & DVT_USES_NO_VALUE)) continue;
        if (e.role == DVT_USES_ADDR || e.role == DVT_USES_RS1) good = good && to.rs1 == d.value;
        if (e.role == DVT_USES_RS2) good = good && to.rs2 == d.value;
        if (e.role == DVT_USES_MEM && (to.kind == DVT_USES_LOAD || to.kind == DVT_USES_STORE)) good = good && to.before == d.value;
    }
    return good;
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: uses_host GUEST.elf [STDIN.bin ...]\n"); return 2; }
    std::vector<uint8_t> elf;
    if (!read_file(argv[1], &elf)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<std::vector<uint8_t>> stdin_bufs(argc - 2);
    for (int i = 2; i < argc; i++)
        if (!read_file(argv[i], &stdin_bufs[i - 2])) { fprintf(stderr, "cannot read %s\n", argv[i]); return 2; }
    rv32::Program prog;
    std::string err;
    if (!rv32::load_elf(elf.data(), elf.size(), &prog, &err)) { fprintf(stderr, "ELF: %s\n", err.c_str()); return 2; }
    rv32::ExecResult res;
    rv32::execute(prog, stdin_bufs, true, 1ull << 26, 12, &res);
    if (!res.halted) { fprintf(stderr, "the guest did not halt: %s\n", res.error.c_str()); return 2; }
    std::vector<std::vector<rv32::CycleRec>> real, over;
    for (auto &sh : res.shards) real.push_back(sh.recs);
    std::vector<uint32_t> words;   // the first and the last eight words the executor lists outside the image
    for (const rv32::MemInitRow &m : res.mem_rows)
        if (!(m.addr >= rv32::REG_BASE && m.addr < rv32::REG_BASE + 32) && m.addr < rv32::ADDR_LIMIT && !m.is_img) words.push_back(m.addr & ~3u);
    if (words.size() > 16) words.erase(words.begin() + 8, words.end() - 8);
    words.push_back(rv32::ADDR_LIMIT - 4);
    struct Target { uint32_t what, target; };
    std::vector<Target> targets;
    for (uint32_t k = 1; k < 32; k++) targets.push_back({DVT_USES_REG, k});
    for (uint32_t w : words) targets.push_back({DVT_USES_WORD, w});
    const uint32_t S = (uint32_t)real.size(), last_n = S ? (uint32_t)real.back().size() : 0;
    const uint32_t places[][2] = {{1, 0}, {1, 1}, {1, 4095}, {2, 0}, {(S + 1) / 2, 2048}, {S, last_n}, {0xffffffffu, 0xffffffffu}};
    const Limits limits[] = {{DVT_USES_MAX_DEPTH, DVT_USES_MAX_FAN, DVT_USES_MAX_NODES, DVT_USES_MAX_DEFS, DVT_USES_MAX_EDGES}, {3, 2, 7, 9, 20}, {0, 1, 0, 1, 1}};
    bool ok = true;
    for (auto &at : places) {
        uint64_t checked = 0, nodes = 0;
        bool good = true;
        for (const Target &t : targets)
            for (uint32_t flags : {0u, (uint32_t)DVT_USES_FOLLOW_ADDR})
                for (const Limits &l : limits) {
                    Answer a{};
                    slice(prog, real, at[0], at[1], t.what, t.target, flags, l, &a);
                    good = good && !a.bad && a.s.cycles == res.cycles && lawful(a, l, true);
                    if (a.s.position == a.s.cycles)   // the end, by its position or by its name: nothing reads the value any more
                        good = good && a.nodes.empty() && a.edges.empty() && a.defs.size() == 1 && a.defs[0].n_uses == 0 &&
                               a.defs[0].flags == (DVT_USES_LIVE_AT_EXIT | DVT_USES_NO_VALUE);
                    checked += a.s.n_edges; nodes += a.s.n_nodes;
                }
        printf("as executed at %u:%u: %zu targets, %llu nodes, %llu edges%s\n", at[0], at[1], targets.size(), (unsigned long long)nodes,
               (unsigned long long)checked, good ? "" : "  <- the laws fail");
        ok = ok && good;
    }
    // the same records with one field of each overwritten
    uint64_t x = 0x9e3779b97f4a7c15ull;
    for (auto &sh : res.shards) {
        std::vector<rv32::CycleRec> recs = sh.recs;
        for (auto &r : recs) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            switch (x & 7) {
            case 0: r.idx = (uint32_t)(x >> 32); break;
            case 1: r.b = (uint32_t)(x >> 32); break;
            case 2: r.c = (uint32_t)(x >> 32); break;
            case 3: r.m_prev = (uint32_t)(x >> 32); break;
            case 4: r.b = rv32::ADDR_LIMIT - (uint32_t)((x >> 32) & 0xff); break;
            case 5: r.c = rv32::ADDR_LIMIT - (uint32_t)((x >> 32) & 0x1ff); break;
            default: break;
            }
        }
        over.push_back(std::move(recs));
    }
    for (auto &at : places) {
        uint64_t bad = 0, nodes = 0;
        bool good = true;
        for (const Target &t : targets)
            for (const Limits &l : limits) {
                Answer a{};
                slice(prog, over, at[0], at[1], t.what, t.target, DVT_USES_FOLLOW_ADDR, l, &a);
                good = good && a.s.cycles == res.cycles && lawful(a, l, false);
                bad = a.bad; nodes += a.s.n_nodes;
            }
        printf("overwritten at %u:%u: bad=%llu nodes=%llu%s\n", at[0], at[1], (unsigned long long)bad, (unsigned long long)nodes, good ? "" : "  <- the laws fail");
        ok = ok && good;
    }
    return ok ? 0 : 1;
}
