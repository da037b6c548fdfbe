// Stand-alone driver of the origin search's host rule (csrc/origin.h) for AddressSanitizer / UBSan, on the CPU:
//   make -C dvt_circuits_amd/csrc asan-origin && build/asan/origin_host GUEST.elf [STDIN.bin ...]
// Runs the guest in trace mode (rv32::execute, shards of 2^12 cycles), feeds every shard's cycle records to origin::Keeper and
// runs origin::Search at seven positions (the first record, span and shard edges, the middle, the end in two spellings) for
// every register, for the first and last words the executor lists, with and without FOLLOW_ADDR, at the full limits and at
// small ones (depth 3, 7 nodes, 20 edges); then does the same over the records with their fields overwritten by a fixed
// pseudo-random stream (instruction indices outside the text, addresses outside guest memory, unknown syscall ids, call arrays
// that leave guest memory), which the rule must skip as bad or follow like any other record without reading or writing out of
// bounds.  Exit code 0 when, on the records as executed,
//   every edge with a node behind it and a value carries the value its producer wrote (rd_value, or `after` of a store),
//   every producer lies before its consumer, every index lies inside the arrays and the limits asked for hold,
//   at the end the root of a register carries the executor's final value (the mem_init row of the register), and the two
//   spellings of the end give equal answers.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>

#include "../../dvt_circuits_amd/csrc/origin.h"

using namespace dvt;

static bool read_file(const char *path, std::vector<uint8_t> *out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    out->assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}

struct Answer {
    std::vector<dvt_origin_node> nodes;
    std::vector<dvt_origin_edge> edges;
    dvt_origin_summary s;
    uint64_t bad;
};

static void slice(const rv32::Program &prog, const std::vector<std::vector<rv32::CycleRec>> &shards, uint32_t shard, uint32_t row, uint32_t what, uint32_t target,
                  uint32_t flags, uint32_t depth, size_t cap_nodes, size_t cap_edges, Answer *out) {
    origin::Keeper k(prog, shard, row);
    for (size_t i = 0; i < shards.size(); i++) k.scan(prog, shards[i].data(), shards[i].size(), (uint32_t)i + 1);
    out->nodes.assign(cap_nodes + 1, dvt_origin_node{});
    out->edges.assign(cap_edges, dvt_origin_edge{});
    origin::Search search(prog, k.wst, k.sh, k.P, what, target, flags, depth, out->nodes.data(), cap_nodes, out->edges.data(), cap_edges);
    search.run([&](const std::vector<origin::Question> &qs, std::vector<origin::Found> *found) { return k.answer(prog, qs, found); });
    k.place(&search.s);
    out->s = search.s;
    out->bad = k.bad;
    out->nodes.resize(out->s.n_nodes);
    out->edges.resize(out->s.n_edges);
}

// the laws that hold on any records; exact: also the ones that hold on records as executed
static bool lawful(const Answer &a, uint32_t depth, size_t cap_nodes, size_t cap_edges, bool exact) {
    bool good = a.s.n_nodes <= cap_nodes && a.s.n_edges <= cap_edges && a.s.n_edges >= 1 && a.s.depth <= depth && a.s.questions == a.s.n_edges;
    for (const dvt_origin_node &n : a.nodes) good = good && n.depth <= depth && (size_t)n.first_edge + n.n_edges <= a.edges.size();
    for (size_t i = 0; i < a.edges.size(); i++) {
        const dvt_origin_edge &e = a.edges[i];
        good = good && (e.from == DVT_ORIGIN_NONE ? i == 0 : e.from < a.nodes.size()) && (e.to == DVT_ORIGIN_NONE || e.to < a.nodes.size());
        if (!good || e.to == DVT_ORIGIN_NONE) continue;
        const dvt_origin_node &to = a.nodes[e.to];
        good = good && to.shard == e.src_shard && to.row == e.src_row;
        if (e.from != DVT_ORIGIN_NONE) good = good && watch::position(to.shard, to.row) < watch::position(a.nodes[e.from].shard, a.nodes[e.from].row);
        if (!exact || (e.flags & DVT_ORIGIN_NO_VALUE)) continue;
        if (e.role == DVT_ORIGIN_RS1 || e.role == DVT_ORIGIN_RS2 || e.role == DVT_ORIGIN_ADDR) good = good && to.rd_value == e.value;
        if (e.role == DVT_ORIGIN_MEM && to.kind == DVT_ORIGIN_STORE) good = good && to.after == e.value;
    }
    return good;
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: origin_host GUEST.elf [STDIN.bin ...]\n"); return 2; }
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
    uint32_t final_reg[32] = {};
    std::vector<uint32_t> words;   // the first and the last eight words the executor lists outside the image
    for (const rv32::MemInitRow &m : res.mem_rows) {
        if (m.addr >= rv32::REG_BASE && m.addr < rv32::REG_BASE + 32) final_reg[m.addr - rv32::REG_BASE] = m.f;
        else if (m.addr < rv32::ADDR_LIMIT && !m.is_img) words.push_back(m.addr & ~3u);
    }
    if (words.size() > 16) words.erase(words.begin() + 8, words.end() - 8);
    words.push_back(rv32::ADDR_LIMIT - 4);
    struct Target { uint32_t what, target; };
    std::vector<Target> targets;
    for (uint32_t k = 1; k < 32; k++) targets.push_back({DVT_ORIGIN_REG, k});
    for (uint32_t w : words) targets.push_back({DVT_ORIGIN_WORD, w});
    const uint32_t S = (uint32_t)real.size(), last_n = S ? (uint32_t)real.back().size() : 0;
    const uint32_t places[][2] = {{1, 0}, {1, 1}, {1, 4095}, {2, 0}, {(S + 1) / 2, 2048}, {S, last_n}, {0xffffffffu, 0xffffffffu}};
    struct Limits { uint32_t depth; size_t nodes, edges; };
    const Limits limits[] = {{DVT_ORIGIN_MAX_DEPTH, DVT_ORIGIN_MAX_NODES, DVT_ORIGIN_MAX_EDGES}, {3, 7, 20}, {0, 0, 1}};
    bool ok = true;
    for (auto &at : places) {
        uint64_t checked = 0, nodes = 0;
        bool good = true;
        for (const Target &t : targets)
            for (uint32_t flags : {0u, (uint32_t)DVT_ORIGIN_FOLLOW_ADDR})
                for (const Limits &l : limits) {
                    Answer a{};
                    slice(prog, real, at[0], at[1], t.what, t.target, flags, l.depth, l.nodes, l.edges, &a);
                    good = good && !a.bad && a.s.cycles == res.cycles && lawful(a, l.depth, l.nodes, l.edges, true);
                    if (a.s.position == a.s.cycles && t.what == DVT_ORIGIN_REG) good = good && a.edges[0].value == final_reg[t.target];
                    if (at[0] == S && at[1] == last_n) {   // the end by its position and by its name
                        Answer b{};
                        slice(prog, real, 0xffffffffu, 0xffffffffu, t.what, t.target, flags, l.depth, l.nodes, l.edges, &b);
                        good = good && a.nodes.size() == b.nodes.size() && a.edges.size() == b.edges.size() &&
                               (a.nodes.empty() || !memcmp(a.nodes.data(), b.nodes.data(), a.nodes.size() * sizeof(dvt_origin_node))) &&
                               !memcmp(a.edges.data(), b.edges.data(), a.edges.size() * sizeof(dvt_origin_edge));
                    }
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
                slice(prog, over, at[0], at[1], t.what, t.target, DVT_ORIGIN_FOLLOW_ADDR, l.depth, l.nodes, l.edges, &a);
                good = good && a.s.cycles == res.cycles && lawful(a, l.depth, l.nodes, l.edges, false);
                bad = a.bad; nodes += a.s.n_nodes;
            }
        printf("overwritten at %u:%u: bad=%llu nodes=%llu%s\n", at[0], at[1], (unsigned long long)bad, (unsigned long long)nodes, good ? "" : "  <- the laws fail");
        ok = ok && good;
    }
    return ok ? 0 : 1;
}
