// Stand-alone driver of the watchpoint search's host rule (csrc/watch.h) for AddressSanitizer / UBSan, on the CPU:
//   make -C dvt_circuits_amd/csrc asan-watch && build/asan/watch_host GUEST.elf [STDIN.bin ...]
// Runs the guest in trace mode (rv32::execute, shards of 2^12 cycles) and feeds every shard's cycle records to
// watch::scan_records with 16 queries of every kind, for K = 0, 1, 7 and 256; then feeds the same records with their fields
// overwritten by a fixed pseudo-random stream (instruction indices outside the text, addresses outside guest memory, unknown
// syscall ids, call arrays that leave guest memory), which the rule must count as bad or test like any other record without
// reading or writing out of bounds.  Exit code 0 when the laws between the search's own outputs hold: the whole-text query
// finds every cycle, the lists are in execution order, the last list ends where the first would if K covered everything, and
// the totals do not depend on K.
#include <cstdio>
#include <fstream>
#include <iterator>

#include "../../dvt_circuits_amd/csrc/watch.h"

using namespace dvt;

static bool read_file(const char *path, std::vector<uint8_t> *out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    out->assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}

static dvt_watch_query query(uint32_t kind, uint32_t flags, uint32_t lo, uint32_t hi, uint32_t mask = 0, uint32_t want = 0) {
    dvt_watch_query q{};
    q.kind = kind; q.flags = flags; q.lo = lo; q.hi = hi; q.mask = mask; q.want = want;
    q.to_shard = q.to_row = 0xffffffffu;
    return q;
}

static std::vector<dvt_watch_query> queries_of(const rv32::Program &prog) {
    const uint32_t tb = prog.text_base, te = tb + 4 * (uint32_t)(prog.instrs.size() - 1), all = DVT_WATCH_LOAD | DVT_WATCH_STORE | DVT_WATCH_PRE_READ | DVT_WATCH_PRE_WRITE;
    std::vector<dvt_watch_query> q{query(DVT_WATCH_PC, 0, tb, te), query(DVT_WATCH_PC, 0, tb + 16, tb + 20), query(DVT_WATCH_REG, 0, 2, 3), query(DVT_WATCH_REG, 0, 5, 6),
                                   query(DVT_WATCH_REG, DVT_WATCH_VALUE, 10, 11, 0xff, 0), query(DVT_WATCH_REG, 0, 31, 32), query(DVT_WATCH_MEM, all, 0, rv32::ADDR_LIMIT),
                                   query(DVT_WATCH_MEM, DVT_WATCH_STORE, 0, rv32::ADDR_LIMIT), query(DVT_WATCH_MEM, DVT_WATCH_LOAD, 0, rv32::ADDR_LIMIT),
                                   query(DVT_WATCH_MEM, DVT_WATCH_PRE_READ, 0, 0xffffffffu), query(DVT_WATCH_MEM, DVT_WATCH_PRE_WRITE, 0, 0xffffffffu),
                                   query(DVT_WATCH_MEM, all | DVT_WATCH_VALUE, 0, rv32::ADDR_LIMIT, 0xff, 0), query(DVT_WATCH_MEM, all, rv32::ADDR_LIMIT - 64, 0xffffffffu),
                                   query(DVT_WATCH_MEM, all, 0, 4), query(DVT_WATCH_PC, 0, tb, te), query(DVT_WATCH_PC, 0, 0, 0xffffffffu)};
    q[14].from_shard = 2; q[14].from_row = 100; q[14].to_shard = 3; q[14].to_row = 7;
    return q;
}

// one search over `shards` with cap K; false when a law fails
static bool run(const rv32::Program &prog, const std::vector<std::vector<rv32::CycleRec>> &shards, uint32_t K, const char *what, std::vector<uint64_t> *totals_out,
                uint64_t *bad_out) {
    const std::vector<dvt_watch_query> qs = queries_of(prog);
    std::string text;
    std::vector<dvt_watch_hit> hits(2 * qs.size() * (size_t)K + 1);
    std::vector<uint64_t> totals(qs.size());
    if (watch::input_error(qs.data(), qs.size(), K, hits.data(), totals.data(), &text)) {
        fprintf(stderr, "%s: the queries are refused: %s\n", what, text.c_str());
        return false;
    }
    watch::Search s(prog, qs.data(), qs.size(), K);
    uint64_t cycles = 0;
    for (size_t k = 0; k < shards.size(); k++) {
        watch::scan_records(prog, shards[k].data(), shards[k].size(), (uint32_t)k + 1, &s);
        cycles += shards[k].size();
    }
    dvt_watch_summary sum{};
    watch::emit(prog, s, (uint32_t)shards.size(), 0.0, hits.data(), totals.data(), &sum);
    bool ok = sum.cycles == cycles && totals[15] + s.bad == cycles && totals[0] == totals[15] && totals[7] + totals[8] <= totals[6];
    for (size_t q = 0; q < qs.size(); q++) {
        const uint64_t n = std::min<uint64_t>(K, totals[q]);
        for (int half = 0; half < 2; half++)
            for (uint64_t i = 0; i < n; i++) {
                const dvt_watch_hit &h = hits[(2 * q + half) * K + i];
                ok = ok && h.query == q && h.kind == qs[q].kind && h.shard >= 1 && h.shard <= shards.size() && h.row < shards[h.shard - 1].size();
                if (i) {
                    const dvt_watch_hit &g = hits[(2 * q + half) * K + i - 1];
                    ok = ok && watch::position(g.shard, g.row) < watch::position(h.shard, h.row);
                }
            }
        if (n && n == totals[q])   // the lists coincide
            for (uint64_t i = 0; i < n; i++) ok = ok && hits[2 * q * K + i].row == hits[(2 * q + 1) * K + i].row && hits[2 * q * K + i].shard == hits[(2 * q + 1) * K + i].shard;
    }
    printf("%s K=%u: cycles=%llu bad=%llu totals", what, K, (unsigned long long)cycles, (unsigned long long)s.bad);
    for (uint64_t t : totals) printf(" %llu", (unsigned long long)t);
    printf("\n");
    if (!totals_out->empty() && *totals_out != totals) { fprintf(stderr, "%s: the totals depend on K\n", what); ok = false; }
    *totals_out = totals;
    *bad_out = s.bad;
    if (!ok) fprintf(stderr, "%s K=%u: the search's outputs disagree\n", what, K);
    return ok;
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: watch_host GUEST.elf [STDIN.bin ...]\n"); return 2; }
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
    bool ok = true;
    std::vector<uint64_t> totals, totals_over;
    uint64_t bad = 0, bad_over = 0;
    for (uint32_t K : {0u, 1u, 7u, 256u}) {
        ok = run(prog, real, K, "as executed", &totals, &bad) && ok;
        ok = run(prog, over, K, "overwritten", &totals_over, &bad_over) && ok;
    }
    if (bad) { fprintf(stderr, "%llu bad records in what the executor wrote\n", (unsigned long long)bad); ok = false; }
    if (totals.empty() || totals[0] != res.cycles) { fprintf(stderr, "the whole-text query did not find every cycle\n"); ok = false; }
    return ok ? 0 : 1;
}
